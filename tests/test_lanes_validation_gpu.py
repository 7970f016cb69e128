"""evaluate.run_validation / run_upscale with keyed noise over execution lanes and rank shards on a real MI355X: lanes = 2
gives the bits of lanes = 1, two rank shards merged give the bits of the unsharded run, a sample's draws do not depend on
the batch size, and nothing (pool, concurrency, weight selection, files of a refused call) is left behind.

The tree, the model and the dataset wrapper are those of tests/test_lanes_eval_gpu.py: batch_ref.make_tree with 5 pairs at
256 x 192, the tiny model with the style stage on embeddings, batch_size 2 (batches of 2, 2 and 1)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import batch_ref as br
import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import data, evaluate, rng, synth

pytestmark = pytest.mark.gpu
_cache = {}
KEYS = ["val/loss_simple", "val/loss_vlb", "val/loss", "val/loss_simple_ema", "val/loss_vlb_ema", "val/loss_ema"]


def get_model():
    if "m" not in _cache:
        extra = upgpt_amd.model_params("tiny")["extra_cond_stages"]
        extra["style_cond"] = dict(extra["style_cond"], cond_stage_key="style_emb")
        m = upgpt_amd.build_model("tiny", overrides={"extra_cond_stages": extra})
        synth.fill_module_(m)
        synth.fill_ema_(m, salt=1)
        _cache["m"] = m.cuda()
    return _cache["m"]


class WithEmbeddings:
    """tests/test_lanes_eval_gpu.py's wrapper: `txt` and the style embeddings as a function of the sample's index, already on
    the device.  batches() passes batch_start / batch_step on, so a shard builds its own batches only."""

    def __init__(self, ds):
        self.ds, self.built = ds, []

    def batches(self, batch_size, batch_start=0, batch_step=1):
        for k, b in enumerate(self.ds.batches(batch_size, batch_start=batch_start, batch_step=batch_step)):
            j = batch_start + k * batch_step
            self.built.append(j)
            n = len(b["fname"])
            gs = [torch.Generator().manual_seed(100 + j * batch_size + i) for i in range(n)]
            txt = torch.stack([torch.randn(77, 768, generator=g) for g in gs])
            sty = torch.stack([0.45 * torch.randn(9, 768, generator=g) for g in gs])
            yield dict(b, txt=txt.cuda(), style_emb=sty.cuda())


class Walked:
    """The same batches from a source that knows nothing of shards: run_validation walks through it and counts."""

    def __init__(self, ds):
        self.inner = WithEmbeddings(ds)

    def batches(self, batch_size):
        return self.inner.batches(batch_size)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    kw = dict(br.make_tree(tmp_path_factory.mktemp("data"), pic=(256, 192), mask=(256, 256)), input_mask_type="bbox")
    ds = data.DeepFashionPair(**kw)
    assert len(ds) == 5
    return ds


def clean(m):
    unet = m.model.diffusion_model
    return (L.pools_in_flight() == 1 and L.concurrency() == 1 and unet._weight_override is None and
            unet._weight_selection() is None)


def bits(d):
    return {k: np.float64(v).view(np.uint64) for k, v in d.items()}


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def serial(tree, tmp_path_factory):
    """The world = 1, lanes = 1 run with seed 7 on the single-forward tuning table: computed once, shared, left unchanged."""
    root = tmp_path_factory.mktemp("serial")
    means = evaluate.run_validation(get_model(), WithEmbeddings(tree), batch_size=2, noise_seed=7, save_dir=root)
    return root, means


def test_lanes_give_the_bits_of_the_serial_run(tree, tmp_path):
    m = get_model()
    with L.shared_chip(2):  # the serial run on the lanes' tuning table (tests/test_lanes_gpu.py: "a lane changes nothing")
        one = evaluate.run_validation(m, WithEmbeddings(tree), batch_size=2, noise_seed=7, save_dir=tmp_path / "one")
    assert clean(m)
    two = evaluate.run_validation(m, WithEmbeddings(tree), batch_size=2, noise_seed=7, save_dir=tmp_path / "two", lanes=2)
    assert clean(m)
    print("run_validation lanes=1:", one)
    assert list(one) == KEYS == list(two) and all(np.isfinite(v) for v in one.values())
    assert bits(one) == bits(two), (one, two)
    assert sorted(os.listdir(tmp_path / "two")) == ["val_metrics.json", "val_samples.csv", "val_schedule.json"]
    for name in os.listdir(tmp_path / "one"):
        assert read(tmp_path / "one" / name) == read(tmp_path / "two" / name), name
    ids, rows = evaluate._read_val_samples(tmp_path / "two" / "val_samples.csv")
    assert ids == list(range(5)) and np.isfinite(np.array(rows)).all()
    assert all(a != b for a, b in zip(list(one.values())[:3], list(one.values())[3:]))  # (the EMA pass is another weight set)


def test_two_rank_shards_merge_to_the_unsharded_run(tree, serial, tmp_path):
    m = get_model()
    root, want = serial
    built = []
    for r in range(2):  # both ranks one after the other in this process: no collective is involved
        ds = WithEmbeddings(tree)
        part = evaluate.run_validation(m, ds, batch_size=2, noise_seed=7, save_dir=tmp_path, rank=r, world=2)
        built.append(ds.built)
        assert clean(m) and list(part) == KEYS and not (tmp_path / "val_metrics.json").exists()
    assert built == [[0, 2], [1]]  # (a rank decodes its own batches only)
    assert sorted(os.listdir(tmp_path)) == ["val_samples.rank0of2.csv", "val_samples.rank1of2.csv", "val_schedule.json"]
    assert evaluate._read_val_samples(tmp_path / "val_samples.rank0of2.csv")[0] == [0, 1, 4]  # ids stay global
    assert evaluate._read_val_samples(tmp_path / "val_samples.rank1of2.csv")[0] == [2, 3]
    got = evaluate.merge_validation(tmp_path)
    assert bits(got) == bits(want), (got, want)
    assert read(tmp_path / "val_samples.csv") == read(root / "val_samples.csv")
    assert read(tmp_path / "val_metrics.json") == read(root / "val_metrics.json")
    # a source without batch_start / batch_step is walked through: the same shard, the same bits
    walked = evaluate.run_validation(m, Walked(tree), batch_size=2, noise_seed=7, save_dir=tmp_path / "w", rank=1, world=2)
    assert read(tmp_path / "w" / "val_samples.rank1of2.csv") == read(tmp_path / "val_samples.rank1of2.csv")
    assert bits(walked) == bits(part)


def test_a_samples_draws_do_not_depend_on_the_batch_size(tree, serial, tmp_path, monkeypatch):
    """t of both passes and the keyed noise of an id are the same at batch_size 2 and 3.  The loss values are not (other
    GEMM tilings for another batch size), so they are not compared."""
    m = get_model()
    seen = {}
    real = m.validation_step
    shape = (1, m.channels, *m.image_size)

    def recording(batch, batch_idx=0, noise_keys=None):
        for i, sid in enumerate(noise_keys.ids):
            seen[sid] = rng.randn(noise_keys[i:i + 1].fork(1), shape, rng.STREAM_LOSS_NOISE)
        return real(batch, batch_idx, noise_keys=noise_keys)

    monkeypatch.setattr(m, "validation_step", recording, raising=False)
    per_bs = {}
    for bs in (2, 3):
        seen.clear()
        evaluate.run_validation(m, WithEmbeddings(tree), batch_size=bs, noise_seed=7, save_dir=tmp_path / str(bs))
        ids, rows = evaluate._read_val_samples(tmp_path / str(bs) / "val_samples.csv")
        per_bs[bs] = (ids, np.array(rows), dict(seen))
    monkeypatch.undo()
    (ids2, rows2, nz2), (ids3, rows3, nz3) = per_bs[2], per_bs[3]
    assert ids2 == ids3 == list(range(5)) and sorted(nz2) == sorted(nz3) == list(range(5))
    assert np.array_equal(rows2[:, [0, 3]], rows3[:, [0, 3]])
    assert all(torch.equal(nz2[i], nz3[i]) for i in range(5)) and not torch.equal(nz2[0], nz2[1])
    # ... and the batch_size 2 run is the shared serial run, file for file
    assert read(tmp_path / "2" / "val_samples.csv") == read(serial[0] / "val_samples.csv")
    assert rows2[:3, 0].tolist() == [769.0, 419.0, 828.0] and rows2[:3, 3].tolist() == [902.0, 661.0, 35.0]


def test_another_seed_gives_other_values(tree, serial):
    m = get_model()
    other = evaluate.run_validation(m, WithEmbeddings(tree), batch_size=2, noise_seed=8)
    assert list(other) == KEYS and all(other[k] != serial[1][k] for k in KEYS)
    again = evaluate.run_validation(m, WithEmbeddings(tree), batch_size=2, noise_seed=7, max_batches=2)
    ids, rows = evaluate._read_val_samples(serial[0] / "val_samples.csv")
    assert again["val/loss_simple"] == sum(r[1] for r in rows[:4]) / 4  # (max_batches: the first samples, the same draws)


def test_lanes_need_a_noise_seed_and_leave_nothing_behind(tree, tmp_path):
    m = get_model()
    with pytest.raises(ValueError, match="noise_seed"):
        evaluate.run_validation(m, WithEmbeddings(tree), batch_size=2, lanes=2, save_dir=tmp_path / "x")
    assert clean(m) and not (tmp_path / "x").exists()


# ---------------------------------------------------------------- run_upscale
def _files(root):
    out = {}
    for folder in sorted(os.listdir(root)):
        for name in sorted(os.listdir(root / folder)):
            out[folder + "/" + name] = read(root / folder / name)
    return out


def test_run_upscale_lanes_write_the_bytes_of_the_serial_run(tmp_path):
    m = upgpt_amd.build_model("upscale", overrides={"image_size": [32, 24]})
    synth.fill_module_(m)
    m = m.cuda()
    m.crop_size = [128, 88]
    names = ["fashion_%02d" % i for i in range(5)]
    lr_dir = tmp_path / "samples"
    os.makedirs(lr_dir)
    for n, p in zip(names, np.random.default_rng(3).integers(0, 256, (5, 64, 44, 3), dtype=np.uint8)):
        Image.fromarray(p).save(lr_dir / (n + ".jpg"))

    def batches():
        for j in range(0, 5, 2):
            gs = [torch.Generator().manual_seed(300 + i) for i in range(j, min(j + 2, 5))]
            yield {"fname": names[j:j + 2], "image": torch.zeros(len(gs), 128, 96, 3, device="cuda"),
                   "txt": torch.stack([torch.randn(77, 768, generator=g) for g in gs]).cuda(),
                   "styles": torch.stack([0.45 * torch.randn(9, 768, generator=g) for g in gs]).cuda()}

    kw = dict(pad=(2, 0), ddim_steps=2, ddim_eta=1., noise_seed=7)
    with L.shared_chip(2):
        a = _files(evaluate.run_upscale(m, batches(), lr_dir, tmp_path / "serial", **kw))
    b = _files(evaluate.run_upscale(m, batches(), lr_dir, tmp_path / "lanes", lanes=2, **kw))
    assert L.pools_in_flight() == 1 and L.concurrency() == 1
    assert sorted(a) == sorted(b) == sorted(f + "/" + n + ".jpg" for f in ("lr", "upscaled") for n in names)
    diff = [k for k in a if a[k] != b[k]]
    assert not diff, "files that differ between lanes=1 and lanes=2: %s" % diff
    with L.shared_chip(2):
        c = _files(evaluate.run_upscale(m, batches(), lr_dir, tmp_path / "other", **dict(kw, noise_seed=8)))
    assert all(c[k] == a[k] for k in a if k.startswith("lr/")) and all(c[k] != a[k] for k in a if k.startswith("upscaled/"))
    # rank 1 of 2 writes batch 1 alone, with the global ids: the same bytes
    with L.shared_chip(2):
        d = _files(evaluate.run_upscale(m, batches(), lr_dir, tmp_path / "r1", rank=1, world=2, **kw))
    assert sorted(d) == sorted(f + "/" + n + ".jpg" for f in ("lr", "upscaled") for n in names[2:4])
    assert all(d[k] == a[k] for k in d)
    with pytest.raises(ValueError, match="noise_seed"):
        evaluate.run_upscale(m, batches(), lr_dir, tmp_path / "x", lanes=2, pad=(2, 0), ddim_steps=2)
    assert L.pools_in_flight() == 1 and not (tmp_path / "x").exists()
