"""evaluate.run_split over execution lanes with keyed noise on a real MI355X: the files a lanes=2 run writes are, name for
name and byte for byte, those of the lanes=1 run with the same noise_seed; a sample's noise does not depend on the batch
size; the pool is closed and the logger restored afterwards; lanes without a noise_seed are refused.

The tree is tests/batch_ref.make_tree's with 5 pairs.  Its pictures are 256 x 192, not make_tree's default 64 x 48: the
tiny model samples 32 x 24 latents (256 x 192 pictures) and test_step refuses a reconstruction of another size, and a
64 x 48 picture is an 8 x 6 latent, which the UNet's three 2x downsamplings cannot halve — the size
test_run_split_end_to_end (tests/test_batch_gpu.py) uses for the same reason."""
import os

import pytest
import torch

import batch_ref as br
import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import data, evaluate, rng, synth

pytestmark = pytest.mark.gpu
_cache = {}
KW = dict(ddim_steps=2, ddim_eta=1., noise_seed=7)


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
    """The dataset with `txt` replaced by an embedding tensor (the tiny model's text stage is a pass-through) and the style
    embeddings added, both a function of the sample's index alone and already on the device (assembly runs under
    host_io(), so the upload belongs here and not into the lane's test_step)."""

    def __init__(self, ds):
        self.ds = ds

    def batches(self, batch_size):
        seen = 0
        for b in self.ds.batches(batch_size):
            n = len(b["fname"])
            gs = [torch.Generator().manual_seed(100 + seen + i) for i in range(n)]
            seen += n
            txt = torch.stack([torch.randn(77, 768, generator=g) for g in gs])
            sty = torch.stack([0.45 * torch.randn(9, 768, generator=g) for g in gs])
            yield dict(b, txt=txt.cuda(), style_emb=sty.cuda())


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    kw = dict(br.make_tree(tmp_path_factory.mktemp("data"), pic=(256, 192), mask=(256, 256)), input_mask_type="bbox")
    ds = data.DeepFashionPair(**kw)
    assert len(ds) == 5
    return ds


def _files(root):
    out = {}
    for folder in sorted(os.listdir(root)):
        for name in sorted(os.listdir(root / folder)):
            with open(root / folder / name, "rb") as f:
                out[folder + "/" + name] = f.read()
    return out


def test_lanes_write_the_bytes_of_the_serial_run(tree, tmp_path):
    m = get_model()
    # the serial run takes the same tuning table as the lanes (tests/test_lanes_gpu.py): "a lane changes nothing"
    with L.shared_chip(2):
        serial = evaluate.run_split(m, WithEmbeddings(tree), tmp_path / "serial", batch_size=2, **KW)
    lanes = evaluate.run_split(m, WithEmbeddings(tree), tmp_path / "lanes", batch_size=2, lanes=2, **KW)
    assert L.pools_in_flight() == 1 and not hasattr(m, "logger") and L.concurrency() == 1
    a, b = _files(serial), _files(lanes)
    assert sorted(a) == sorted(b) and len(a) == 7 * 5
    assert sorted({k.split("/")[0] for k in a}) == ["concats", "gt", "recon", "samples", "smpl", "src", "styles"]
    diff = [k for k in a if a[k] != b[k]]
    assert not diff, "files that differ between lanes=1 and lanes=2: %s" % diff
    # ... and the noise does something: another seed gives other samples, the same inputs
    with L.shared_chip(2):
        other = _files(evaluate.run_split(m, WithEmbeddings(tree), tmp_path / "other", batch_size=2, ddim_steps=2,
                                          ddim_eta=1., noise_seed=8))
    assert all(other[k] == a[k] for k in a if k.startswith("gt/"))
    assert all(other[k] != a[k] for k in a if k.startswith("samples/"))


def test_a_samples_noise_does_not_depend_on_the_batch_size(tree, tmp_path, monkeypatch):
    """Pictures of different batch sizes come from other GEMM tilings, so the comparison is the keyed x_T of every fname."""
    m = get_model()
    seen = {}
    shape = (1, m.channels, *m.image_size)

    def record(batch, noise_keys=None, **kw):
        for i, fname in enumerate(batch["fname"]):
            seen[fname] = (noise_keys.ids[i], rng.randn(noise_keys[i:i + 1], shape, rng.STREAM_XT))
        raise _Stop()

    class _Stop(Exception):
        pass

    monkeypatch.setattr(m, "log_images", record, raising=False)
    per_bs = {}
    for bs in (2, 3):
        seen.clear()
        for j, batch, keys in evaluate._keyed_batches(m, WithEmbeddings(tree).batches(bs), 7):
            with pytest.raises(_Stop):
                m.log_images(batch, noise_keys=keys)
        per_bs[bs] = dict(seen)
    assert sorted(per_bs[2]) == sorted(per_bs[3]) and len(per_bs[2]) == 5
    for fname, (sid, x_T) in per_bs[2].items():
        assert per_bs[3][fname][0] == sid and torch.equal(per_bs[3][fname][1], x_T), fname
    assert sorted(v[0] for v in per_bs[2].values()) == list(range(5))  # the running index = the dataset index
    xs = [v[1] for v in per_bs[2].values()]
    assert not torch.equal(xs[0], xs[1])


def test_lanes_need_a_noise_seed_and_leave_nothing_behind(tree, tmp_path):
    m = get_model()
    with pytest.raises(ValueError, match="noise_seed"):
        evaluate.run_split(m, WithEmbeddings(tree), tmp_path / "x", batch_size=2, lanes=2, ddim_steps=2, ddim_eta=1.)
    assert not hasattr(m, "logger") and L.pools_in_flight() == 1 and not (tmp_path / "x").exists()


def test_a_lane_threads_exception_ends_the_run_and_is_re_raised(tree, tmp_path):
    m = get_model()

    class Broken(WithEmbeddings):
        def batches(self, batch_size):
            for i, b in enumerate(super().batches(batch_size)):
                if i == 1:
                    raise RuntimeError("the loader failed on batch 1")
                yield b

    m.logger = keep = evaluate.ResultDir(tmp_path / "mine")
    try:
        with pytest.raises(RuntimeError, match="failed on batch 1"):
            evaluate.run_split(m, Broken(tree), tmp_path / "y", batch_size=2, lanes=2, **KW)
        assert m.logger is keep and L.pools_in_flight() == 1
    finally:
        del m.logger
