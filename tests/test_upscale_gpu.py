"""The upscale stage on the MI355X: the upscale model at a 32 x 24 latent with recipe weights, fed once with the `lr`
conditioning made on the host (tests/resize_ref.py, which is Pillow byte for byte) and once with the pictures through
InferenceModel.upscale / evaluate.run_upscale, which make it on the device.  The kernel's arithmetic is exact, so the
bar is BITWISE equality of lr and, under the same seed, of the samples; there is no tolerance to choose."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import finish_ref as fr
import resize_ref as rr
import upgpt_amd
from upgpt_amd import evaluate, prepare, synth
from upgpt_amd.inference import InferenceModel

pytestmark = pytest.mark.gpu
B, STEPS, PAD, SIZE, F = 2, 4, (2, 0), (32, 24), 4
CROP = [128, 88]
_cache = {}


def get_model():
    if "m" not in _cache:
        m = upgpt_amd.build_model("upscale", overrides={"image_size": [32, 24]})
        synth.fill_module_(m)
        m = m.cuda()
        m.crop_size = CROP  # (the config's [512, 352] belongs to its 128 x 96 latent)
        _cache["m"] = m
    return _cache["m"]


def pictures(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, 64, 44, 3), dtype=np.uint8)


def conditioning():
    g = torch.Generator().manual_seed(8)
    return torch.randn(B, 77, 768, generator=g), 0.45 * torch.randn(B, 9, 768, generator=g)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def verdict(lr_equal, samples_equal):
    """Which side a failure is on: the kernel (lr differs) or the facade around it (lr equal, samples differ)."""
    if not lr_equal:
        return "lr differs from the host-made conditioning: the fault is in the resize kernel / prepare"
    if not samples_equal:
        return "lr is bitwise equal but samples differ: the fault is in the facade, not in the kernel"
    return "ok"


def test_lr_transform_equals_pillow_bitwise():
    pics = pictures()
    lr, lr_image = prepare.lr_transform(torch.from_numpy(pics).cuda(), SIZE, PAD)
    w_lr, w_img, w_u8 = rr.lr_transform(pics, SIZE, PAD)
    for b in range(B):
        padded = np.pad(pics[b], ((0, 0), (PAD[0], PAD[0]), (0, 0)), mode="edge")
        assert np.array_equal(w_u8[b], np.asarray(Image.fromarray(padded).resize((SIZE[1], SIZE[0]), Image.BILINEAR)))
    assert lr.shape == (B, 3, 32, 24) and lr_image.shape == (B, 32, 24, 3)
    assert np.array_equal(bits(lr.cpu().numpy()), bits(w_lr)) and np.array_equal(bits(lr_image.cpu().numpy()), bits(w_img))


def test_upscale_equals_log_images_fed_the_host_made_lr(monkeypatch):
    m = get_model()
    pics = pictures(1)
    txt, styles = conditioning()
    w_lr = rr.lr_transform(pics, SIZE, PAD)[0]
    batch = {"image": torch.zeros(B, F * 32, F * 24, 3), "txt": txt, "styles": styles, "lr": torch.from_numpy(w_lr)}
    torch.manual_seed(11)
    want = m.log_images(batch, ddim_steps=STEPS, use_ema=False, unconditional_guidance_scale=3.,
                        unconditional_guidance_label=[""])["samples"]
    assert want.shape == (B, 3, F * 32, F * 24)  # the output size is f * image_size
    want = torch.clamp(want.detach().cpu(), -1., 1.).permute(0, 2, 3, 1).numpy() * 0.5 + 0.5
    seen = {}
    real = m.log_images
    monkeypatch.setattr(m, "log_images", lambda batch, **kw: (seen.update(batch=batch, kw=kw), real(batch, **kw))[1])
    im = object.__new__(InferenceModel)
    im.model, im.device = m, "cuda"
    torch.manual_seed(11)
    out = im.upscale(torch.from_numpy(pics).cuda(), styles, txt, steps=STEPS, pad=PAD)
    assert seen["kw"]["use_ema"] is False and seen["kw"]["ddim_steps"] == STEPS
    assert sorted(seen["batch"]) == ["image", "lr", "styles", "txt"] and seen["batch"]["lr"].is_cuda
    assert seen["batch"]["image"].shape == (B, F * 32, F * 24, 3)
    lr_equal = np.array_equal(bits(seen["batch"]["lr"].cpu().numpy()), bits(w_lr))
    samples_equal = out["samples"].shape == want.shape and np.array_equal(bits(out["samples"]), bits(want))
    print("upscale: lr bitwise equal %s, samples bitwise equal %s" % (lr_equal, samples_equal))
    assert lr_equal and samples_equal, verdict(lr_equal, samples_equal)
    assert out["samples"].shape == (B, 128, 96, 3) and out["samples"].min() >= 0 and out["samples"].max() <= 1


def _jpeg(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return f.getvalue()


def test_run_upscale_writes_what_log_images_gives_for_the_host_made_lr(tmp_path, monkeypatch):
    m = get_model()
    names = ["fashion_00", "fashion_01"]
    lr_dir = tmp_path / "samples"
    os.makedirs(lr_dir)
    for n, p in zip(names, pictures(2)):
        Image.fromarray(p).save(lr_dir / (n + ".jpg"))
    decoded = np.stack([np.asarray(Image.open(lr_dir / (n + ".jpg")).convert("RGB")) for n in names])
    w_lr, w_img, w_u8 = rr.lr_transform(decoded, SIZE, PAD)
    txt, styles = conditioning()
    batch = {"fname": names, "image": torch.zeros(B, F * 32, F * 24, 3), "txt": txt, "styles": styles}
    log = m.log_images(dict(batch, lr=torch.from_numpy(w_lr), lr_image=torch.from_numpy(w_img)), N=B, use_ema=m.use_ema,
                       unconditional_guidance_scale=3.0, unconditional_guidance_label=["txt"], ddim_steps=STEPS, seed=5)
    samples = log["samples"].detach().cpu()
    want = [fr.to_pil_array(t) for t in fr.sample_value(samples, CROP)]
    seen = {}
    real = m.log_images
    monkeypatch.setattr(m, "log_images", lambda batch, **kw: (seen.update(batch=batch, kw=kw, log=real(batch, **kw)), seen["log"])[1])
    out = evaluate.run_upscale(m, [batch], lr_dir, tmp_path / "run", pad=PAD, ddim_steps=STEPS, seed=5)
    assert str(out) == str(tmp_path / "run" / "results") and sorted(os.listdir(out)) == ["lr", "upscaled"]
    assert seen["kw"]["N"] == B and seen["kw"]["use_ema"] is False and sorted(batch) == ["fname", "image", "styles", "txt"]
    lr_equal = (np.array_equal(bits(seen["batch"]["lr"].cpu().numpy()), bits(w_lr)) and
                np.array_equal(bits(seen["batch"]["lr_image"].cpu().numpy()), bits(w_img)))
    samples_equal = np.array_equal(bits(seen["log"]["samples"].cpu().numpy()), bits(samples.numpy()))
    print("run_upscale: lr bitwise equal %s, samples bitwise equal %s" % (lr_equal, samples_equal))
    assert lr_equal and samples_equal, verdict(lr_equal, samples_equal)
    for i, n in enumerate(names):
        assert sorted(os.listdir(out / "upscaled")) == sorted(os.listdir(out / "lr")) == [v + ".jpg" for v in names]
        assert open(out / "upscaled" / (n + ".jpg"), "rb").read() == _jpeg(want[i]), n
        assert open(out / "lr" / (n + ".jpg"), "rb").read() == _jpeg(w_u8[i]), n
    assert Image.open(out / "upscaled" / "fashion_00.jpg").size == (88, 128)  # f * image_size, centre-cropped
    assert Image.open(out / "lr" / "fashion_00.jpg").size == (24, 32)
    (lr_dir / "fashion_01.jpg").unlink()
    with pytest.raises(ValueError, match="fashion_01.jpg"):
        evaluate.run_upscale(m, [batch], lr_dir, tmp_path / "run2", pad=PAD, ddim_steps=STEPS)
