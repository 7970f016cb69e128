"""Which form of the fused feed-forward tail the lowering asks for (Emitter.row_chain_rows("mlp", ...), the knobs, the
shared-chip table), and that the Python mirror of UPK_MLP_STREAM is the header's."""
import os
import re
from types import SimpleNamespace

from upgpt_amd import _lib as L
from upgpt_amd import knobs
from upgpt_amd.emitter import Emitter
from upgpt_amd.tuning import TUNE_CACHE_LANES


def rows(M):
    return Emitter.row_chain_rows(SimpleNamespace(), "mlp", M, 0)


def test_mlp_rows_come_from_the_knob_or_the_shared_chip_table(monkeypatch):
    monkeypatch.setattr(knobs, "MLP_ROWS", 0)
    monkeypatch.setattr(knobs, "XB_ROWS", 64)  # (the other row-chain kernels' knob does not reach this one)
    monkeypatch.delenv("UPGPT_LANES_TUNING", raising=False)
    monkeypatch.setitem(TUNE_CACHE_LANES.meta, "__mlp_rows__", {"8192": 128})
    assert rows(8192) == 0  # one batch at a time: nothing stored applies, mlp_rows decides as before
    with L.shared_chip(4):
        assert rows(8192) == 128 and rows(2048) == 0
        monkeypatch.setenv("UPGPT_LANES_TUNING", "0")
        assert rows(8192) == 0
        monkeypatch.delenv("UPGPT_LANES_TUNING")
        monkeypatch.setattr(knobs, "MLP_ROWS", 64)
        assert rows(8192) == 64
    assert rows(8192) == 64


def test_shipped_table_lists_supported_mlp_tile_heights():
    by_m = TUNE_CACHE_LANES.meta.get("__mlp_rows__", {})
    assert by_m.get("8192") == 128  # (the bench shape: measured in two sessions)
    assert all(int(m) > 0 and int(r) in (32, 64, 128) for m, r in by_m.items())


def test_stream_flag_mirrors_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "upk.h")) as f:
        m = re.search(r"#define UPK_MLP_STREAM (0x[0-9a-fA-F]+)", f.read())
    assert m and int(m.group(1), 16) == L.MLP_STREAM
    assert L.MLP_STREAM & 255 == 0  # (clear of every tile height)
