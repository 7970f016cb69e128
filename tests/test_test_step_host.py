"""LatentDiffusion.test_step, the parts that need no GPU: the centre-crop rule, the DENORM constants, the ABI
declaration / binding / build list of upk_image_finish_u8, and test_step's host logic (folders, names, concat order,
the N=len(batch) cap, the log_kwargs overlay) with the kernel call replaced by tests/finish_ref.py and log_images by a
constant."""
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import finish_ref as fr
from upgpt_amd import _lib, build, evaluate
from upgpt_amd.ddpm import LatentDiffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "upk_image_finish_u8"
FOLDERS = ["concats", "gt", "recon", "samples", "smpl", "src", "styles"]


def test_center_crop_window_follows_torchvisions_rule():
    # hand-checked, .5 cases included: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0, 1.5 -> 2
    assert evaluate.center_crop_window(256, 192, [256, 176]) == (0, 8, 256, 176)
    assert evaluate.center_crop_window(512, 384, [512, 352]) == (0, 16, 512, 352)
    assert evaluate.center_crop_window(37, 47, [32, 40]) == (2, 4, 32, 40)
    assert evaluate.center_crop_window(33, 35, (32, 32)) == (0, 2, 32, 32)
    assert evaluate.center_crop_window(224, 224, 224) == (0, 0, 224, 224)
    assert evaluate.center_crop_window(300, 301, 224) == (38, 38, 224, 224)
    for h in range(20, 45):
        for w in (20, 21, 26, 27, 33, 64):
            for crop in (20, [20, 16], (17, 20), [19], np.int64(18)):
                assert evaluate.center_crop_window(h, w, crop) == fr.center_crop_offsets(h, w, crop), (h, w, crop)


def test_an_image_smaller_than_the_crop_is_refused():
    for h, w in ((255, 192), (256, 175), (10, 10)):
        with pytest.raises(ValueError, match="smaller than crop_size"):
            evaluate.center_crop_window(h, w, [256, 176])


def test_denorm_constants_are_the_references_rounded_once():
    for got, s in zip(evaluate.DENORM_D, (0.226862954, 0.26130258, 0.27577711)):
        assert isinstance(got, np.float32) and got == np.float32(1 / s)
    for got, m in zip(evaluate.DENORM_M, (0.48145466, 0.4578275, 0.40821073)):
        assert isinstance(got, np.float32) and got == np.float32(-m)
    # ... and they are what T.Normalize makes of the reference's lists
    assert torch.equal(torch.as_tensor(fr.DENORM_STD_1, dtype=torch.float32), torch.tensor([float(v) for v in evaluate.DENORM_D]))
    assert torch.equal(torch.as_tensor(fr.DENORM_MEAN_2, dtype=torch.float32), torch.tensor([float(v) for v in evaluate.DENORM_M]))


def test_the_saturating_restatement_is_the_plain_one_where_byte_is_defined():
    g = torch.Generator().manual_seed(0)
    t = torch.rand(3, 64, 64, generator=g) * (256.9 / 255) - (0.9 / 255)  # t * 255 in (-1, 256)
    assert np.array_equal(fr.to_pil_array(t), fr.to_pil_array(t, saturate=True))
    wild = torch.tensor([float("nan"), float("-inf"), float("inf"), -2.0, 2.0]).view(1, 1, 5)
    assert fr.to_pil_array(wild, saturate=True).reshape(-1).tolist() == [0, 0, 255, 0, 255]


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    assert NAME in set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    proto = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header).group(1)
    assert NAME in _lib.SYMBOLS
    lib = _lib.load_library()
    assert hasattr(lib, NAME) and lib.upk_version() == 100  # additive: the ABI version stays
    assert len(getattr(lib, NAME).argtypes) == len(proto.split(",")) == 18
    doc = header[header.index("/* What LatentDiffusion.test_step does"):header.index("int " + NAME)]
    for needle in ("ddpm.py:1352-1357", "ddpm.py:1371-1376", "UPK_FINISH_SAMPLE", "UPK_FINISH_INPUT", "UPK_FINISH_DENORM",
                   "SATURATES", "Never allocates, never synchronises, graph-capturable"):
        assert needle in doc, needle
    for name, val in (("UPK_LAYOUT_NCHW", _lib.LAYOUT_NCHW), ("UPK_LAYOUT_NHWC", _lib.LAYOUT_NHWC),
                      ("UPK_FINISH_SAMPLE", _lib.FINISH_SAMPLE), ("UPK_FINISH_INPUT", _lib.FINISH_INPUT),
                      ("UPK_FINISH_DENORM", _lib.FINISH_DENORM)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == val


def test_the_kernel_source_is_built_without_fma_contraction():
    assert "image.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "image.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS.get("image.hip", [])


def test_finish_images_refuses_host_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.finish_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), _lib.LAYOUT_NCHW,
                               _lib.FINISH_SAMPLE)


# ---- test_step's host logic on a stand-in model
class _Model:
    crop_size, use_ema, device = [32, 24], True, torch.device("cpu")
    test_step = LatentDiffusion.test_step

    def __init__(self, log):
        self.log, self.calls = log, []

    def log_images(self, batch, N=8, **kw):
        self.calls.append(dict(kw, N=N))
        return {k: v[:N] for k, v in self.log.items()}


def _ref_finish_images(src, dst, layout, mode, window=None, dst_x=0, denorm=None):
    """evaluate.finish_images' contract on CPU tensors through tests/finish_ref.py."""
    x = src.permute(0, 3, 1, 2) if layout == _lib.LAYOUT_NHWC else src
    t = {_lib.FINISH_SAMPLE: lambda v: (torch.clamp(v, -1., 1.) + 1.0) / 2.0, _lib.FINISH_INPUT: lambda v: (v + 1.0) / 2.0,
         _lib.FINISH_DENORM: fr.denorm_value}[mode](x)
    top, left, ch, cw = (0, 0, x.shape[2], x.shape[3]) if window is None else window
    for b in range(x.shape[0]):
        dst[b, :ch, dst_x:dst_x + cw] = torch.from_numpy(fr.to_pil_array(t[b, :, top:top + ch, left:left + cw]))


def _batch(B, g):
    img = lambda: torch.rand(B, 36, 32, 3, generator=g) * 2 - 1
    styles = (torch.rand(B, 2, 3, 16, 16, generator=g) - 0.45) / 0.27
    return {"image": img(), "src_image": img(), "smpl_image": img(), "styles": styles, "txt": ["a person"] * B,
            "fname": ["img_%02d" % i for i in range(B)]}


def _jpeg(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return f.getvalue()


def _tree(root):
    return {d: sorted(os.listdir(os.path.join(root, d))) for d in sorted(os.listdir(root))}


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(evaluate, "finish_images", _ref_finish_images)
    g = torch.Generator().manual_seed(1)
    B = 8
    batch = _batch(B, g)
    log = {"samples": torch.randn(B, 3, 36, 32, generator=g), "reconstruction": torch.randn(B, 3, 36, 32, generator=g)}
    return _Model(log), batch, log


def test_test_step_writes_the_references_tree(stand_in, tmp_path):
    m, batch, log = stand_in
    B, n = 8, len(batch)  # 6 keys < 8 samples: the reference's N=len(batch) cap shows
    assert n == 6
    m.logger = evaluate.ResultDir(tmp_path)
    assert m.test_step(batch, 0) is None
    assert m.calls == [dict(N=n, use_ema=True, unconditional_guidance_scale=3.0, unconditional_guidance_label=["txt"])]
    tree = _tree(tmp_path / "results")
    assert sorted(tree) == FOLDERS
    for k in FOLDERS:
        count = B if k == "styles" else n  # the styles loop is not capped
        assert tree[k] == ["img_%02d.jpg" % i for i in range(count)], k
    want = fr.finished({k: v[:n] for k, v in log.items()}, batch, m.crop_size)
    for k in FOLDERS:
        for i, name in enumerate(tree[k]):
            assert open(tmp_path / "results" / k / name, "rb").read() == _jpeg(want[k][i]), (k, name)
    assert set(batch) == {"image", "src_image", "smpl_image", "styles", "txt", "fname"}
    assert batch["image"].shape == (B, 36, 32, 3)  # (the batch is not rewritten in place)


def test_finished_arrays_layout_by_position(stand_in):
    m, batch, log = stand_in
    arr = evaluate.finished_arrays(m, batch, log)
    assert sorted(arr) == FOLDERS
    cw = 24
    assert arr["concats"].shape == (8, 32, 4 * cw, 3) and arr["styles"].shape == (8, 16, 2 * 16, 3)
    for slot, k in enumerate(("src", "samples", "recon", "smpl")):
        assert arr[k].shape == (8, 32, cw, 3) and arr[k].dtype == np.uint8
        assert np.array_equal(arr["concats"][:, :, slot * cw:(slot + 1) * cw], arr[k]), k
    want = fr.finished(log, batch, m.crop_size)
    for k in FOLDERS:
        assert np.array_equal(arr[k], np.stack(want[k])), k
    for s in range(2):  # crop s of the strip is the de-normalised crop s, uncropped
        assert np.array_equal(arr["styles"][3][:, s * 16:(s + 1) * 16], fr.to_pil_array(fr.denorm_value(batch["styles"][3, s])))
    # the centre crop is a crop: rows 2..34, columns 4..28 of the 36 x 32 source
    assert np.array_equal(arr["gt"][0], fr.to_pil_array(((batch["image"][0].permute(2, 0, 1) + 1.0) / 2.0)[:, 2:34, 4:28]))


def test_log_kwargs_are_laid_over_the_references_arguments(stand_in, tmp_path):
    m, batch, _ = stand_in
    m.logger = evaluate.ResultDir(tmp_path)
    m.test_step(batch, 3, ddim_steps=5, ddim_eta=0., unconditional_guidance_scale=1.5, N=3)
    assert m.calls == [dict(N=3, use_ema=True, unconditional_guidance_scale=1.5, unconditional_guidance_label=["txt"],
                            ddim_steps=5, ddim_eta=0.)]
    tree = _tree(tmp_path / "results")
    assert len(tree["samples"]) == len(tree["concats"]) == 3 and len(tree["styles"]) == 8


def test_run_test_sets_the_logger_and_restores_it(stand_in, tmp_path):
    m, batch, _ = stand_in
    second = dict(batch, fname=["other_%d" % i for i in range(8)])
    out = evaluate.run_test(m, [batch, second], tmp_path, ddim_steps=5)
    assert str(out) == str(tmp_path / "results")
    assert [c["ddim_steps"] for c in m.calls] == [5, 5]
    assert len(os.listdir(tmp_path / "results" / "styles")) == 16 and len(os.listdir(tmp_path / "results" / "gt")) == 12
    assert not hasattr(m, "logger")
    with pytest.raises(ValueError, match="save_dir"):
        m.test_step(batch, 0)


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "upk_image_finish_u8" in design and "per-lane generators" in design
    assert "run_test" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "test_step" in open(os.path.join(ROOT, "README.md")).read()
