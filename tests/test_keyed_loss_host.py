"""Host side of the keyed validation (upk_q_sample_keyed_f32, validation_step(noise_keys=), run_validation(noise_seed=, rank=,
world=), merge_validation): the timestep draw's known answers, the declarations, the shard arithmetic, the merge of
hand-written shard files and the argument checks.  No GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rng_ref  # noqa: E402
import val_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (w0 * 1000) >> 32 of ids 0..7, seed 7: computed with the committed reference (tests/rng_ref.py) on a CPU
T_DRAW0 = [769, 419, 828, 531, 399, 180, 566, 294]
T_DRAW1 = [902, 661, 35, 889, 468, 605, 464, 597]


def test_timestep_known_answers():
    keys = rng_ref.keys_of(7, range(8))
    for draw, want in ((0, T_DRAW0), (1, T_DRAW1)):
        w0 = rng_ref.words(keys, 4, 0, 1, 4, draw)[..., 0].reshape(-1).astype(np.uint64)
        assert ((w0 * np.uint64(1000)) >> np.uint64(32)).tolist() == want
        assert val_ref.timesteps(keys, 1000, draw).tolist() == want
    t = val_ref.timesteps(rng_ref.keys_of(7, range(4096)), 1000)
    assert int(t.min()) == 0 and int(t.max()) == 999


def test_package_names_the_two_streams_and_the_keys_match():
    from upgpt_amd import rng
    assert (rng.STREAM_XT, rng.STREAM_STEP, rng.STREAM_QSAMPLE, rng.STREAM_POSTERIOR) == (0, 1, 2, 3)
    assert (rng.STREAM_TIMESTEP, rng.STREAM_LOSS_NOISE) == (4, 5) == (val_ref.STREAM_TIMESTEP, val_ref.STREAM_LOSS_NOISE)
    # the package's own host Philox gives the same timestep words for NoiseKeys(7, ids)
    k = rng.NoiseKeys(7, range(8)).host
    for draw, want in ((0, T_DRAW0), (1, T_DRAW1)):
        ctr = np.array([[0, 0, rng.STREAM_TIMESTEP, draw]] * 8, dtype=np.uint64)
        w0 = rng.philox4x32_10(ctr, k.astype(np.uint64))[:, 0]
        assert ((w0 * np.uint64(1000)) >> np.uint64(32)).tolist() == want


def test_symbol_declared_and_built():
    from upgpt_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    declared = set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    assert "upk_q_sample_keyed_f32" in declared and "upk_q_sample_keyed_f32" in _lib.SYMBOLS
    assert re.search(r"#define\s+UPK_STREAM_TIMESTEP\s+4\b", header) and re.search(r"#define\s+UPK_STREAM_LOSS_NOISE\s+5\b", header)
    assert os.path.exists(os.path.join(build.CSRC, "philox.h"))
    loss = open(os.path.join(build.CSRC, "loss.hip")).read()
    assert '#include "philox.h"' in loss and '#include "philox.h"' in open(os.path.join(build.CSRC, "rng.hip")).read()
    assert build.FILE_FLAGS["loss.hip"] == ["-ffp-contract=off"] == build.FILE_FLAGS["rng.hip"]
    _lib.load_library()  # (every symbol of SYMBOLS resolves, with its prototype)
    assert callable(getattr(_lib.Context, "q_sample_keyed"))


@pytest.mark.parametrize("n_batches", [0, 1, 5, 8, 13])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 7])
def test_shards_cover_every_batch_once(n_batches, world):
    from upgpt_amd import evaluate
    parts = [evaluate.shard_batches(n_batches, r, world) for r in range(world)]
    assert parts == [val_ref.shard(n_batches, r, world) for r in range(world)]
    assert sorted(j for p in parts for j in p) == list(range(n_batches))
    assert all(p == sorted(p) for p in parts)


def test_shard_work_walks_or_strides():
    """A source without batch_start / batch_step is walked through and counted; one with them is asked for its own batches
    only; both give the same (batch index, first id)."""
    from upgpt_amd import evaluate
    sizes = [3, 3, 3, 3, 2]

    class Plain:
        def batches(self, batch_size):
            for j, n in enumerate(sizes):
                yield {"fname": ["f%d_%d" % (j, i) for i in range(n)]}

    class Strided:
        built = []

        def batches(self, batch_size, batch_start=0, batch_step=1):
            for j in range(batch_start, len(sizes), batch_step):
                self.built.append(j)
                yield {"fname": ["f%d_%d" % (j, i) for i in range(sizes[j])]}

    for world in (1, 2, 3):
        for rank in range(world):
            a = [(j, first, b["fname"]) for j, first, b in evaluate._shard_work(Plain(), 3, rank, world, None)]
            Strided.built = []
            b = [(j, first, b["fname"]) for j, first, b in evaluate._shard_work(Strided(), 3, rank, world, None)]
            assert a == b and [j for j, _, _ in a] == val_ref.shard(5, rank, world)
            assert [first for _, first, _ in a] == [3 * j for j, _, _ in a]
            assert Strided.built == val_ref.shard(5, rank, world)  # (nothing else was built)
    assert [j for j, _, _ in evaluate._shard_work(Plain(), 3, 1, 2, 3)] == [1]  # max_batches counts GLOBAL batches
    assert [j for j, _, _ in evaluate._shard_work(Strided(), 3, 0, 2, 3)] == [0, 2]
    assert [j for j, _, _ in evaluate._shard_work(iter([{"fname": ["a"]}, {"fname": ["b"]}]), 1, 1, 2, None)] == [1]


def test_dataset_batches_stride_builds_only_its_own(monkeypatch):
    from upgpt_amd import data
    built = []
    ds = object.__new__(data.DeepFashionPair)
    monkeypatch.setattr(data.DeepFashionPair, "__len__", lambda self: 11)
    monkeypatch.setattr(data.DeepFashionPair, "_samples", lambda self, idx: list(idx), raising=False)
    monkeypatch.setattr(data.DeepFashionPair, "_assemble", lambda self, s: s, raising=False)
    monkeypatch.setattr(data.DeepFashionPair, "_finish", lambda self, s: built.append(s) or s, raising=False)
    every = list(ds.batches(3))
    assert every == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]
    for world in (2, 3):
        for rank in range(world):
            built.clear()
            got = list(ds.batches(3, batch_start=rank, batch_step=world))
            assert got == every[rank::world] == built
    with pytest.raises(ValueError):
        list(ds.batches(3, batch_step=0))


# ---------------------------------------------------------------- merge_validation on hand-written shard files
HEADER = "id,t,simple,plain,t_ema,simple_ema,plain_ema\n"
ROWS = {0: "0,769,0.5,0.25,902,0.75,0.5", 1: "1,419,0.1,0.2,661,0.30000000000000004,0.4",
        2: "2,828,1.5,1.25,35,2.5,2.25", 3: "3,531,0.125,0.0625,889,1e-3,2e-3", 4: "4,399,3.0,1.0,468,4.0,2.0"}


def _sched(n_t=1000, learn_logvar=False):
    lvlb = [float(np.float32(0.001 * (i + 1))) for i in range(n_t)]
    logvar = [float(np.float32(0.01 * (i % 7) - 0.03)) for i in range(n_t)]
    return {"prefix": "val", "l_simple_weight": 1.0, "original_elbo_weight": 0.25, "learn_logvar": learn_logvar,
            "lvlb_weights": lvlb, "logvar": logvar}


def _write(tmp_path, shards, sched=None):
    for name, ids in shards.items():
        (tmp_path / name).write_text(HEADER + "".join(ROWS[i] + "\n" for i in ids))
    (tmp_path / "val_schedule.json").write_text(json.dumps(_sched() if sched is None else sched))


def test_merge_validation(tmp_path):
    from upgpt_amd import evaluate
    # batch_size 2, world 2: rank 0 has batches 0 and 2 (ids 0, 1, 4), rank 1 batch 1 (ids 2, 3)
    _write(tmp_path, {"val_samples.rank0of2.csv": [0, 1, 4], "val_samples.rank1of2.csv": [2, 3]})
    got = evaluate.merge_validation(tmp_path)
    assert list(got) == ["val/loss_simple", "val/loss_vlb", "val/loss", "val/loss_simple_ema", "val/loss_vlb_ema", "val/loss_ema"]
    table = np.array([[float(c) for c in ROWS[i].split(",")[1:]] for i in range(5)])
    s = _sched()
    want = val_ref.epoch_means(table, s["lvlb_weights"], s["logvar"], 1.0, 0.25)
    for k in got:
        assert abs(got[k] - want[k]) <= 4 * 2.0 ** -52 * abs(want[k]), (k, got[k], want[k])
    assert got["val/loss_simple"] == ((((0.5 + 0.1) + 1.5) + 0.125) + 3.0) / 5  # sample-index order, one addition at a time
    assert json.load(open(tmp_path / "val_metrics.json")) == got
    # the merged table is the world = 1 file, and it reads back to the same doubles
    ids, rows = evaluate._read_val_samples(tmp_path / "val_samples.csv")
    assert ids == list(range(5)) and np.array_equal(np.array(rows), table)
    assert evaluate.validation_means(table, s) == got
    # with learn_logvar the gamma term and the logvar mean are reported as validation_step reports them
    lv = evaluate.validation_means(table, _sched(learn_logvar=True))
    assert list(lv)[:5] == ["val/loss_simple", "val/loss_gamma", "logvar", "val/loss_vlb", "val/loss"]
    assert lv["val/loss"] == got["val/loss"]


@pytest.mark.parametrize("shards, match", [
    ({"val_samples.rank0of2.csv": [0, 1, 4]}, "every rank once"),                                      # a rank is missing
    ({"val_samples.rank0of2.csv": [0, 1], "val_samples.rank1of2.csv": [2, 3]}, None),                    # complete: 4 samples
    ({"val_samples.rank0of2.csv": [0, 1, 4], "val_samples.rank1of2.csv": [3]}, "gaps"),                 # id 2 is missing
    ({"val_samples.rank0of2.csv": [0, 1, 2], "val_samples.rank1of2.csv": [2, 3]}, "more than one row"),  # id 2 twice
    ({"val_samples.rank0of2.csv": [0, 1], "val_samples.rank1of3.csv": [2, 3]}, "different world"),
    ({}, "no val_samples"),
])
def test_merge_validation_refuses_gaps_and_duplicates(tmp_path, shards, match):
    from upgpt_amd import evaluate
    _write(tmp_path, shards)
    if match is None:
        assert len(evaluate._read_val_samples(tmp_path / "val_samples.rank0of2.csv")[0]) == 2
        assert np.isfinite(list(evaluate.merge_validation(tmp_path).values())).all()
        return
    with pytest.raises(ValueError, match=match):
        evaluate.merge_validation(tmp_path)
    assert not (tmp_path / "val_metrics.json").exists()


# ---------------------------------------------------------------- the argument checks (before any device work)
def test_value_errors(tmp_path):
    import torch
    import upgpt_amd
    from upgpt_amd import evaluate, rng
    m = upgpt_amd.build_model("tiny")
    k3 = rng.NoiseKeys(1, [0, 1, 2])
    x = torch.zeros(2, 4, 32, 24)
    t = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="3 keys for a batch of 2"):
        m.p_losses(x, None, t, noise_keys=k3)
    with pytest.raises(ValueError, match="3 keys for a batch of 2"):
        m(x, {"c_crossattn": None}, noise_keys=k3)
    with pytest.raises(ValueError, match="both name the noise"):
        m.p_losses(x, None, t, noise=torch.zeros_like(x), noise_keys=k3[:2])
    with pytest.raises(ValueError, match="3 keys for a batch of 2"):
        m.validation_step({"image": torch.zeros(2, 256, 192, 3)}, 0, noise_keys=k3)
    with pytest.raises(ValueError, match="lanes > 1 needs noise_seed"):
        evaluate.run_validation(m, [], lanes=2, save_dir=tmp_path / "v")
    with pytest.raises(ValueError, match="world > 1 needs noise_seed"):
        evaluate.run_validation(m, [], world=2, rank=1, save_dir=tmp_path / "v")
    with pytest.raises(ValueError, match=r"rank must be in \[0, world\)"):
        evaluate.run_validation(m, [], noise_seed=1, world=2, rank=2, save_dir=tmp_path / "v")
    with pytest.raises(ValueError, match="lanes must be >= 1"):
        evaluate.run_validation(m, [], noise_seed=1, lanes=0)
    with pytest.raises(ValueError, match="lanes > 1 needs noise_seed"):
        evaluate.run_upscale(m, [], tmp_path / "lr", tmp_path / "u", lanes=2)
    assert not (tmp_path / "v").exists() and not (tmp_path / "u").exists()


def test_weight_set_per_thread():
    """The thread-scoped selection takes precedence over the process-wide override and is seen by its own thread alone."""
    import threading

    import upgpt_amd
    m = upgpt_amd.build_model("tiny")
    unet = m.model.diffusion_model
    sel = lambda: (unet._weight_selection() or ("live",))[0]
    seen = {}
    assert sel() == "live"
    with m.ema_scope(local=True):
        assert sel() == "ema" and unet._weight_override is None
        th = threading.Thread(target=lambda: seen.setdefault("other", sel()))
        th.start()
        th.join()
        with m.ema_scope(local=True):  # nests: the previous selection is put back
            assert sel() == "ema"
        assert sel() == "ema"
    assert sel() == "live" and seen == {"other": "live"}
    with m.ema_scope():  # the process-wide form: every thread, unless it selected for itself
        prev = unet.set_weight_local("live")
        assert prev is None and sel() == "live"
        th = threading.Thread(target=lambda: seen.setdefault("wide", sel()))
        th.start()
        th.join()
        unet.set_weight_local(prev)
        assert sel() == "ema"
    assert sel() == "live" and seen["wide"] == "ema" and unet._weight_override is None and m._ema_depth == 0
