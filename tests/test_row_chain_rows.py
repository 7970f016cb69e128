"""Which tile height the lowering asks of the row-chain kernels (Emitter.row_chain_rows): one batch at a time the 32-row
default, with several batches in flight the decision stored with the shared-chip table, and the knobs over both."""
from types import SimpleNamespace

from upgpt_amd import _lib as L
from upgpt_amd import knobs
from upgpt_amd.emitter import Emitter
from upgpt_amd.tuning import TUNE_CACHE_LANES


def rows(kind, M, default=32):
    return Emitter.row_chain_rows(SimpleNamespace(), kind, M, default)


def test_row_chain_rows_come_from_the_shared_chip_table_only_when_the_chip_is_shared(monkeypatch):
    monkeypatch.setattr(knobs, "XB_ROWS", 0)
    monkeypatch.setattr(knobs, "HB_ROWS", 0)
    monkeypatch.delenv("UPGPT_LANES_TUNING", raising=False)
    monkeypatch.setitem(TUNE_CACHE_LANES.meta, "__row_chain_rows__", {"hblock": {"8192": 128}, "xblock": {"8192": 64}})
    assert L.concurrency() == 1
    assert rows("hblock", 8192) == 32 and rows("xblock", 8192) == 32 and rows("xblock", 2048, 16) == 16
    with L.shared_chip(4):
        assert rows("hblock", 8192) == 128 and rows("xblock", 8192) == 64
        assert rows("hblock", 1024) == 32 and rows("xblock", 2048, 16) == 16  # (row counts the table does not list)
        monkeypatch.setenv("UPGPT_LANES_TUNING", "0")
        assert rows("hblock", 8192) == 32 and rows("xblock", 8192) == 32
        monkeypatch.delenv("UPGPT_LANES_TUNING")
        monkeypatch.setattr(knobs, "XB_ROWS", 16)
        assert rows("hblock", 8192) == 16 and rows("xblock", 8192) == 16
        monkeypatch.setattr(knobs, "HB_ROWS", 128)
        assert rows("hblock", 8192) == 128 and rows("xblock", 8192) == 16
    assert L.concurrency() == 1


def test_shipped_table_lists_supported_tile_heights():
    dec = TUNE_CACHE_LANES.meta.get("__row_chain_rows__", {})
    assert set(dec) <= {"hblock", "xblock"}
    for kind, by_m in dec.items():
        for m, r in by_m.items():
            assert int(m) > 0 and int(r) in (16, 32, 64, 128), (kind, m, r)
