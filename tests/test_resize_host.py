"""The upscale stage, the parts that need no GPU: tests/resize_ref.py against Pillow itself (byte for byte), the
coefficient tables of upgpt_amd.prepare against the restatement, prepare's validation and refusal rules, the ABI
declaration / binding / build list of upk_resize_bilinear_u8, and the batch InferenceModel.upscale and
evaluate.run_upscale build, with the kernel call replaced by tests/resize_ref.py and log_images by a recording stub."""
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as rr
from upgpt_amd import _lib, build, evaluate, inference, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "upk_resize_bilinear_u8"
# (h, w) -> (oh, ow)
PAIRS = [((256, 192), (128, 96)), ((256, 200), (128, 96)), ((256, 184), (128, 96)), ((37, 53), (16, 24)),
         ((300, 171), (224, 127)), ((20, 30), (40, 60)), ((64, 64), (224, 224)), ((11, 9), (5, 4)),
         ((512, 384), (128, 96)), ((256, 176), (256, 96))]


def _picture(h, w, seed, binary=False):
    rng = np.random.default_rng(seed)
    if binary:
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_the_restatement_is_pillow_byte_for_byte(pair):
    (h, w), (oh, ow) = pair
    img = _picture(h, w, seed=h + w, binary=(h, w) == (37, 53))
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    got = rr.resize(img, (oh, ow))
    print("%s -> %s: %d of %d bytes differ" % ((h, w), (oh, ow), int((got != want).sum()), want.size))
    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("case", [((256, 176), (8, 0), (128, 96)), ((256, 192), (4, 0), (128, 96)), ((13, 7), (3, 2), (6, 5))],
                         ids=["pad8", "pad4", "both_pads"])
def test_the_padded_flow_is_pad_then_resize(case):
    (h, w), (px, py), (oh, ow) = case
    img = _picture(h, w, seed=7 * h + w)
    padded = np.pad(img, ((py, py), (px, px), (0, 0)), mode="edge")
    assert np.array_equal(rr.pad_edge(img, (px, py)), padded)
    want = np.asarray(Image.fromarray(padded).resize((ow, oh), Image.BILINEAR))
    assert np.array_equal(rr.resize(img, (oh, ow), (px, py)), want)
    lr, lr_image, u8 = rr.lr_transform(img[None], (oh, ow), (px, py))
    assert np.array_equal(u8[0], want) and lr.shape == (1, 3, oh, ow) and lr_image.shape == (1, oh, ow, 3)
    t = torch.from_numpy(want.copy()).permute(2, 0, 1).to(torch.float32).div(255) * 2. - 1.  # ToTensor, x * 2. - 1.
    assert lr.dtype == np.float32 and np.array_equal(lr[0].view(np.uint32), t.numpy().view(np.uint32))
    assert np.array_equal(lr_image[0], lr[0].transpose(1, 2, 0))


def test_every_table_up_to_40_equals_the_restatement():
    """1600 (in, out) pairs: bounds, weights and ksize; the weights of a row sum to 2^22 within its tap count."""
    for i in range(1, 41):
        for o in range(1, 41):
            got = prepare.resample_coeffs(i, o)
            if i == o:
                assert got is None
                continue
            wb, wk, wks = rr.coeffs(i, o)
            assert got[2] == wks and got[0].dtype == got[1].dtype == np.int32
            assert np.array_equal(got[0], wb) and np.array_equal(got[1], wk), (i, o)
            n = got[0][:, 1].astype(np.int64)
            assert bool((np.abs(got[1].sum(1, dtype=np.int64) - (1 << 22)) <= n).all()), (i, o)
            assert bool((got[1] >= 0).all())
            prepare.validate_table(got, i, o)


def test_validate_table_refuses_what_the_kernel_must_not_see():
    b, k, ks = prepare.resample_coeffs(20, 8)
    for row, val in ((0, (-1, 2)), (3, (19, 2)), (2, (4, 0)), (1, (0, ks + 1))):
        bad = b.copy()
        bad[row] = val
        with pytest.raises(ValueError):
            prepare.validate_table((bad, k, ks), 20, 8)
    heavy = k.copy()
    heavy[0, 0] += 100
    with pytest.raises(ValueError, match="2\\^22"):
        prepare.validate_table((b, heavy, ks), 20, 8)
    with pytest.raises(ValueError):
        prepare.resample_coeffs(0, 4)


def test_prepare_validation_and_no_cpu_fallback():
    ok = torch.zeros(2, 16, 12, 3, dtype=torch.uint8)
    for fn in (prepare.resize_u8, lambda *a, **k: prepare.lr_transform(*a, **k)):
        with pytest.raises(TypeError, match="uint8"):
            fn(ok.float(), [8, 6])
        with pytest.raises(TypeError):
            fn([[1, 2, 3]], [8, 6])
        with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
            fn(ok[0], [8, 6])
        with pytest.raises(ValueError, match="3-channel"):
            fn(torch.zeros(2, 16, 12, 4, dtype=torch.uint8), [8, 6])
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(2, 0, 12, 3, dtype=torch.uint8), [8, 6])
        for size in ([0, 6], [8, -1], [8, 6, 3]):
            with pytest.raises(ValueError, match="size"):
                fn(ok, size)
        for pad in ((-1, 0), (0, -2), (1,)):
            with pytest.raises(ValueError, match="pad"):
                fn(ok, [8, 6], pad)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(ok, [8, 6])
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(ok.numpy(), [8, 6], (2, 0))


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    proto = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header).group(1)
    assert NAME in _lib.SYMBOLS
    lib = _lib.load_library()
    assert hasattr(lib, NAME) and lib.upk_version() == 100  # additive: the ABI version stays
    assert len(getattr(lib, NAME).argtypes) == len(proto.split(",")) == 23
    doc = header[header.index("/* What the reference does to a generated picture"):header.index("int " + NAME)]
    for needle in ("app.py:93-97", "deepfashion_inshop.py:427-431", "ROUNDED TO uint8", "UPK_ESHAPE", "64 KiB", "acc >> 22",
                   "fl(fl(u / 255) * 2 - 1)", "Never allocates, never synchronises, graph-capturable"):
        assert needle in doc, needle


def test_the_kernel_source_is_built_without_fma_contraction():
    assert "resize.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "resize.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS.get("resize.hip", [])


# ---- the facade on stand-ins: the kernel call is tests/resize_ref.py, log_images records what it receives
def _ref_lr_transform(pictures, size, pad=(0, 0), out_u8=None):
    pics = pictures.cpu().numpy() if torch.is_tensor(pictures) else np.asarray(pictures)
    lr, lr_image, u8 = rr.lr_transform(pics, tuple(size), pad)
    if out_u8 is not None:
        out_u8.copy_(torch.from_numpy(u8))
    return torch.from_numpy(lr), torch.from_numpy(lr_image)


def _ref_finish_images(src, dst, layout, mode, window=None, dst_x=0, denorm=None):
    assert layout == _lib.LAYOUT_NCHW and mode == _lib.FINISH_SAMPLE
    top, left, ch, cw = window
    t = (torch.clamp(src, -1., 1.) + 1.0) / 2.0
    dst[:, :ch, dst_x:dst_x + cw] = t[:, :, top:top + ch, left:left + cw].mul(255).byte().permute(0, 2, 3, 1)


class _Upscaler:
    """What run_upscale and InferenceModel.generate read of the upscale LatentDiffusion."""
    image_size, crop_size, num_downs, use_ema, device = [16, 12], [64, 44], 2, False, torch.device("cpu")

    def __init__(self):
        self.calls = []

    def log_images(self, batch, N=8, **kw):
        self.calls.append((batch, dict(kw, N=N)))
        g = torch.Generator().manual_seed(len(self.calls))
        n = min(N, batch["lr"].shape[0])
        return {"samples": torch.randn(n, 3, 64, 48, generator=g) * 0.8}


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(prepare, "lr_transform", _ref_lr_transform)
    monkeypatch.setattr(evaluate, "finish_images", _ref_finish_images)
    return _Upscaler()


def test_upscale_builds_the_demo_batch(stand_in):
    im = object.__new__(inference.InferenceModel)
    im.model, im.device = stand_in, "cpu"
    B = 2
    pics = np.stack([_picture(32, 22, seed=i) for i in range(B)])
    styles = torch.randn(9, 768)
    out = im.upscale(pics, styles, "a person", steps=7)
    (batch, kw), = stand_in.calls
    assert sorted(batch) == ["image", "lr", "styles", "txt"]
    assert kw == dict(N=8, ddim_steps=7, use_ema=False, unconditional_guidance_scale=3., unconditional_guidance_label=[""])
    want = rr.lr_transform(pics, (16, 12), (4, 0))[0]  # app.py's pad of 4 columns
    assert batch["lr"].dtype == torch.float32 and np.array_equal(batch["lr"].numpy().view(np.uint32), want.view(np.uint32))
    assert batch["styles"].shape == (B, 9, 768) and torch.equal(batch["styles"][1], styles)
    assert batch["txt"] == ["a person"] * B
    assert batch["image"].shape == (B, 64, 48, 3) and batch["image"].dtype == torch.float32 and not batch["image"].any()
    assert sorted(out) == ["samples"] and out["samples"].shape == (B, 64, 48, 3)
    assert out["samples"].min() >= 0 and out["samples"].max() <= 1
    # PIL pictures, per-sample styles and texts, the caller's pad, image and use_ema
    image = torch.ones(B, 64, 48, 3)
    im.upscale([Image.fromarray(p) for p in pics], styles.expand(B, 9, 768), ["a", "b"], pad=(1, 0), use_ema=True, image=image)
    batch, kw = stand_in.calls[1]
    assert kw["use_ema"] is True and kw["ddim_steps"] == 200 and batch["txt"] == ["a", "b"] and batch["image"] is image
    assert np.array_equal(batch["lr"].numpy(), rr.lr_transform(pics, (16, 12), (1, 0))[0])
    with pytest.raises(ValueError, match="2 pictures"):
        im.upscale(pics, styles, ["only one"])


def _jpeg(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return f.getvalue()


def _lr_tree(tmp_path, names, seed=0):
    lr_dir = tmp_path / "lowres"
    os.makedirs(lr_dir)
    for i, n in enumerate(names):
        Image.fromarray(_picture(32, 22, seed=seed + i)).save(lr_dir / (n + ".jpg"))
    return lr_dir


def test_run_upscale_builds_the_dataset_batch_and_writes_the_tree(stand_in, tmp_path):
    names = [["a_0", "a_1", "a_2"], ["b_0"]]
    lr_dir = _lr_tree(tmp_path, sum(names, []))
    batches = [{"fname": ns, "styles": torch.randn(len(ns), 9, 768), "txt": ["t"] * len(ns),
                "image": torch.zeros(len(ns), 64, 48, 3)} for ns in names]
    out = evaluate.run_upscale(stand_in, batches, lr_dir, tmp_path / "run", ddim_steps=5)
    assert str(out) == str(tmp_path / "run" / "results")
    assert sorted(os.listdir(out)) == ["lr", "upscaled"]
    assert sorted(os.listdir(out / "upscaled")) == sorted(os.listdir(out / "lr")) == ["a_0.jpg", "a_1.jpg", "a_2.jpg", "b_0.jpg"]
    assert len(stand_in.calls) == 2
    for idx, ((batch, kw), ns, given) in enumerate(zip(stand_in.calls, names, batches)):
        n = len(ns)
        assert kw == dict(N=n, use_ema=False, unconditional_guidance_scale=3.0, unconditional_guidance_label=["txt"], ddim_steps=5)
        assert sorted(batch) == ["fname", "image", "lr", "lr_image", "styles", "txt"]
        assert sorted(given) == ["fname", "image", "styles", "txt"]  # (the caller's dict is left as it came)
        decoded = np.stack([np.asarray(Image.open(lr_dir / (f + ".jpg")).convert("RGB")) for f in ns])
        lr, lr_image, u8 = rr.lr_transform(decoded, (16, 12), (8, 0))  # the dataset's pad of 8 columns
        assert batch["lr"].shape == (n, 3, 16, 12) and batch["lr_image"].shape == (n, 16, 12, 3)
        assert batch["lr"].dtype == batch["lr_image"].dtype == torch.float32
        assert np.array_equal(batch["lr"].numpy(), lr) and np.array_equal(batch["lr_image"].numpy(), lr_image)
        g = torch.Generator().manual_seed(idx + 1)
        samples = torch.randn(n, 3, 64, 48, generator=g) * 0.8
        want = ((torch.clamp(samples, -1., 1.) + 1.0) / 2.0)[:, :, :, 2:46].mul(255).byte().permute(0, 2, 3, 1).numpy()
        for i, f in enumerate(ns):
            assert open(out / "upscaled" / (f + ".jpg"), "rb").read() == _jpeg(want[i]), f
            assert open(out / "lr" / (f + ".jpg"), "rb").read() == _jpeg(u8[i]), f
    assert Image.open(out / "upscaled" / "a_0.jpg").size == (44, 64) and Image.open(out / "lr" / "a_0.jpg").size == (12, 16)


def test_run_upscale_names_a_missing_or_unreadable_file(stand_in, tmp_path):
    lr_dir = _lr_tree(tmp_path, ["a_0", "a_2"])
    batch = {"fname": ["a_0", "a_1", "a_2"], "styles": torch.zeros(3, 9, 768), "txt": ["t"] * 3, "image": torch.zeros(3, 64, 48, 3)}
    with pytest.raises(ValueError, match="a_1.jpg"):
        evaluate.run_upscale(stand_in, [batch], lr_dir, tmp_path / "run")
    (lr_dir / "a_1.jpg").write_bytes(b"not a picture")
    with pytest.raises(ValueError, match="a_1.jpg"):
        evaluate.run_upscale(stand_in, [batch], lr_dir, tmp_path / "run")
    assert stand_in.calls == []  # (nothing was sampled, nothing substituted)
    Image.fromarray(_picture(30, 22, seed=9)).save(lr_dir / "a_1.jpg")  # another size than its batch
    with pytest.raises(ValueError, match="a_1.jpg"):
        evaluate.run_upscale(stand_in, [batch], lr_dir, tmp_path / "run")
