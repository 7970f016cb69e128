"""LatentDiffusion.test_step on the MI355X: the tiny recipe-weight model and the DeepFashion-shaped batch of the
log_images tests (tests/test_model_gpu.py), extended by the keys test_step reads (src_image, smpl_image, the style
crops, fname).  Everything is compared byte for byte with tests/finish_ref.py applied to the same log dict and batch.

The restated configs feed the style EMBEDDINGS to a DummyModel under batch['styles']; test_step needs the style CROPS
there, as in the reference's dataset, so this model's style stage reads its embeddings from batch['style_emb']."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import finish_ref as fr
import upgpt_amd
from upgpt_amd import evaluate, synth

pytestmark = pytest.mark.gpu
FOLDERS = ["concats", "gt", "recon", "samples", "smpl", "src", "styles"]
S = 2  # style crops per sample
_cache = {}


def get_model():
    if "m" not in _cache:
        extra = upgpt_amd.model_params("tiny")["extra_cond_stages"]
        extra["style_cond"] = dict(extra["style_cond"], cond_stage_key="style_emb")
        m = upgpt_amd.build_model("tiny", overrides={"extra_cond_stages": extra})
        synth.fill_module_(m)
        synth.fill_ema_(m, salt=1)
        _cache["m"] = m.cuda()
    return _cache["m"]


def make_batch(B):
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
             "txt": torch.randn(B, 77, 768, generator=g0), "style_emb": 0.45 * torch.randn(B, 9, 768, generator=g0),
             "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}
    batch["src_image"] = torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1
    batch["smpl_image"] = torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1
    crops = torch.rand(B, S, 3, 224, 224, generator=g0)  # CLIP-normalised [0, 1] crops
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 1, 3, 1, 1)
    batch["styles"] = (crops - mean) / std
    batch["fname"] = ["fashion_%02d" % i for i in range(B)]
    return batch


def cpu_log(log):
    return {k: log[k].detach().cpu() for k in ("samples", "reconstruction")}


def test_finished_arrays_equal_the_reference_expression():
    """All seven pictures of a real log_images result, byte for byte; the concat order and the style strip by position."""
    m = get_model()
    B = 2
    batch = make_batch(B)
    torch.manual_seed(7)
    log = m.log_images(batch, N=len(batch), ddim_steps=5, use_ema=m.use_ema, unconditional_guidance_scale=3.0,
                       unconditional_guidance_label=["txt"])
    assert log["samples"].shape == log["reconstruction"].shape == (B, 3, 256, 192)
    got = evaluate.finished_arrays(m, batch, log)
    want = fr.finished(cpu_log(log), batch, m.crop_size)
    assert sorted(got) == FOLDERS
    for k in FOLDERS:
        w = np.stack(want[k])
        bad = int((got[k] != w).sum()) if got[k].shape == w.shape else -1
        print("%s: shape %s, %d bytes differ" % (k, got[k].shape, bad))
        assert got[k].dtype == np.uint8 and bad == 0, k
    assert got["samples"].shape == (B, 256, 176, 3) and got["concats"].shape == (B, 256, 4 * 176, 3)
    assert got["styles"].shape == (B, 224, S * 224, 3)
    for slot, k in enumerate(("src", "samples", "recon", "smpl")):
        assert np.array_equal(got["concats"][:, :, slot * 176:(slot + 1) * 176], got[k]), k
    for s in range(S):
        assert np.array_equal(got["styles"][1][:, s * 224:(s + 1) * 224], fr.to_pil_array(fr.denorm_value(batch["styles"][1, s])))
    assert len({got[k].tobytes() for k in ("src", "samples", "recon", "smpl", "gt")}) == 5  # (no two pictures alike)


def _jpeg(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return f.getvalue()


@pytest.mark.parametrize("B", [2, 10])
def test_test_step_end_to_end(B, tmp_path):
    """Seeded log_images by hand -> expected pictures -> reseeded test_step: the seven folders hold exactly the expected
    names and every file is the JPEG PIL makes of the expected array.  B = 10 > the batch's 9 keys: the reference's
    N=len(batch) cap leaves 9 per-sample files and 10 style strips."""
    m = get_model()
    batch = make_batch(B)
    assert len(batch) == 9
    n = min(B, len(batch))
    torch.manual_seed(100 + B)
    log = m.log_images(batch, N=len(batch), use_ema=m.use_ema, unconditional_guidance_scale=3.0,
                       unconditional_guidance_label=["txt"], ddim_steps=5)
    assert log["samples"].shape[0] == n
    want = fr.finished(cpu_log(log), batch, m.crop_size)
    m.logger = evaluate.ResultDir(tmp_path)
    try:
        torch.manual_seed(100 + B)
        assert m.test_step(batch, 0, ddim_steps=5) is None
    finally:
        del m.logger
    root = tmp_path / "results"
    assert sorted(os.listdir(root)) == FOLDERS
    for k in FOLDERS:
        count = B if k == "styles" else n
        assert sorted(os.listdir(root / k)) == ["fashion_%02d.jpg" % i for i in range(count)], k
        for i in range(count):
            data = open(root / k / ("fashion_%02d.jpg" % i), "rb").read()
            assert data == _jpeg(want[k][i]), (k, i)
    assert Image.open(root / "concats" / "fashion_00.jpg").size == (4 * 176, 256)
    assert Image.open(root / "styles" / "fashion_00.jpg").size == (S * 224, 224)
    assert batch["image"].shape == (B, 256, 192, 3) and not batch["image"].is_cuda  # (the batch is left as it came)


def test_run_test_loops_over_batches(tmp_path):
    m = get_model()
    a, b = make_batch(2), make_batch(2)
    b["fname"] = ["second_%d" % i for i in range(2)]
    evaluate.run_test(m, [a, b], tmp_path, ddim_steps=2, ddim_eta=0.)
    assert sorted(os.listdir(tmp_path / "results" / "samples")) == ["fashion_00.jpg", "fashion_01.jpg", "second_0.jpg",
                                                                   "second_1.jpg"]
    assert not hasattr(m, "logger")  # (restored: the model had none)


def test_no_fp32_image_reaches_the_host_and_one_uint8_copy_does(monkeypatch):
    """During finished_arrays: any device fp32 image-shaped tensor that is clamped by torch or arrives on the host fails
    the test; exactly one device -> host copy happens, of uint8, behind exactly one synchronise."""
    m = get_model()
    B = 2
    batch = make_batch(B)
    g = torch.Generator().manual_seed(1)
    log = {"samples": torch.randn(B, 3, 256, 192, generator=g).cuda(), "reconstruction": torch.randn(B, 3, 256, 192, generator=g).cuda()}
    want = fr.finished(cpu_log(log), batch, m.crop_size)
    torch.cuda.synchronize()
    image_like = lambda t: torch.is_tensor(t) and t.is_cuda and t.is_floating_point() and t.dim() >= 3
    d2h, syncs = [], []
    T = torch.Tensor

    def moving(name):
        orig = getattr(T, name)

        def f(self, *a, **k):
            out = orig(self, *a, **k)
            if self.is_cuda and not (torch.is_tensor(out) and out.is_cuda):
                assert not image_like(self), "fp32 image copied to the host by Tensor.%s" % name
                d2h.append((name, self.dtype, self.numel()))
            return out
        return f

    def copy_(self, src, *a, **k):
        if torch.is_tensor(src) and src.is_cuda and not self.is_cuda:
            assert not image_like(src), "fp32 image copied to the host by Tensor.copy_"
            d2h.append(("copy_", src.dtype, src.numel()))
        return orig_copy(self, src, *a, **k)

    def no_clamp(name, orig):
        def f(x, *a, **k):
            assert not image_like(x), "torch element-wise op on an fp32 image: %s" % name
            return orig(x, *a, **k)
        return f

    orig_copy = T.copy_
    for name in ("cpu", "to", "numpy", "tolist", "item"):
        monkeypatch.setattr(T, name, moving(name))
    monkeypatch.setattr(T, "copy_", copy_)
    for name in ("clamp", "clamp_", "clip", "mul", "byte"):
        monkeypatch.setattr(T, name, no_clamp(name, getattr(T, name)))
    monkeypatch.setattr(torch, "clamp", no_clamp("torch.clamp", torch.clamp))
    s_sync, g_sync = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), s_sync(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), g_sync(*a, **k))[1])
    got = evaluate.finished_arrays(m, batch, log)
    monkeypatch.undo()
    assert len(d2h) == 1 and d2h[0][1] == torch.uint8, d2h
    assert d2h[0][2] >= sum(int(np.prod(v.shape)) for v in got.values())
    assert len(syncs) == 1, syncs
    for k in FOLDERS:
        assert np.array_equal(got[k], np.stack(want[k])), k


def test_missing_logger_and_small_images_raise(monkeypatch):
    m = get_model()
    batch = make_batch(2)
    assert not hasattr(m, "logger")
    with pytest.raises(ValueError, match="save_dir"):
        m.test_step(batch, 0)
    m.logger = object()  # a logger without save_dir
    try:
        with pytest.raises(ValueError, match="save_dir"):
            m.test_step(batch, 0)
    finally:
        del m.logger
    log = {"samples": torch.zeros(2, 3, 256, 192, device="cuda"), "reconstruction": torch.zeros(2, 3, 256, 192, device="cuda")}
    small = dict(batch, src_image=batch["src_image"][:, :, :170])
    with pytest.raises(ValueError, match="smaller than crop_size"):
        evaluate.finished_arrays(m, small, log)
    monkeypatch.setattr(m, "crop_size", [300, 176])
    with pytest.raises(ValueError, match="smaller than crop_size"):
        evaluate.finished_arrays(m, batch, log)
