"""SSIM / MS-SSIM, the parts that need no GPU: the ABI declaration / binding / build list of upk_ssim_u8, analytic anchors
of the restatement tests/ssim_ref.py, that the GPU test's tolerance tells the algorithm from its near misses, and
run_metrics' host logic with the kernel call replaced by the fp64 restatement."""
import csv
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import ssim_ref as sr
from upgpt_amd import _lib, build, evaluate, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = 0.01 ** 2


def test_header_declares_and_library_exports_both_symbols():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    declared = set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load_library()
    for name, ret, nargs in (("upk_ssim_ws_bytes", "size_t", 4), ("upk_ssim_u8", "int", 15)):
        assert name in declared and name in _lib.SYMBOLS
        proto = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(proto.split(",")) == nargs
    assert lib.upk_version() == 100  # additive: the ABI version stays
    assert "Never allocates, never synchronises, graph-capturable" in header[header.index("SSIM / MS-SSIM moments"):header.index("int upk_ssim_u8")]


def test_metrics_hip_is_built():
    assert "metrics.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "metrics.hip"))


def test_ws_bytes_needs_no_device_and_refuses_bad_shapes():
    lib = _lib.load_library()
    assert lib.upk_ssim_ws_bytes(2, 256, 176, 5) > 0 and lib.upk_ssim_ws_bytes(1, 11, 11, 1) > 0
    assert lib.upk_ssim_ws_bytes(100, 256, 176, 5) > lib.upk_ssim_ws_bytes(2, 256, 176, 5)
    for bad in ((0, 64, 64, 1), (1, 10, 64, 1), (1, 64, 64, 0), (1, 64, 64, 6), (1, 160, 200, 5)):
        assert lib.upk_ssim_ws_bytes(*bad) == 0, bad


def test_the_module_constants_are_the_algorithms():
    assert metrics.MS_WEIGHTS == sr.MS_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert metrics.level_sizes(176, 161, 5) == [(176, 161), (88, 81), (44, 41), (22, 21), (11, 11)]
    assert "oracle" not in open(os.path.join(ROOT, "upgpt_amd", "metrics.py")).read()


# ---- analytic anchors of the restatement
def test_constant_images_have_the_closed_form():
    p, q = 200, 37
    a = np.full((1, 176, 192, 3), p, dtype=np.uint8)
    b = np.full((1, 176, 192, 3), q, dtype=np.uint8)  # (multiples of 16: even at every level, the zero padding never enters)
    lv, s, ms = sr.metrics(a, b, 5)
    want = (2 * (p / 255) * (q / 255) + C1) / ((p / 255) ** 2 + (q / 255) ** 2 + C1)
    assert torch.allclose(lv[..., 1], torch.ones_like(lv[..., 1]), rtol=0, atol=1e-12)  # cs = 1
    assert torch.allclose(lv[..., 0], torch.full_like(lv[..., 0], want), rtol=0, atol=1e-12)
    assert abs(float(s) - want) < 1e-12 and abs(float(ms) - want ** 0.1333) < 1e-12


def test_identical_images_give_exactly_one():
    a, _ = sr.make_pair("noise", 2, 176, 161)
    for dtype in (torch.float32, torch.float64):
        lv, s, ms = sr.metrics(a, a.copy(), 5, dtype)
        assert bool((lv == 1).all()) and bool((s == 1).all()) and bool((ms == 1).all())


def test_level_sizes_of_161_and_the_first_pooled_pixel():
    x = torch.rand(1, 3, 161, 161, dtype=torch.float64)
    sizes = []
    for _ in range(5):
        sizes.append(x.shape[3])
        x = sr.pool(x)
    assert sizes == [161, 81, 41, 21, 11]
    x = torch.rand(1, 1, 5, 6, dtype=torch.float64)
    x[0, 0, 0, :] = 0.75  # odd H, even W, a constant first row: 1-d pooling of the H axis, x0 / 2
    assert sr.pool(x).shape == (1, 1, 3, 3) and torch.allclose(sr.pool(x)[0, 0, 0], torch.full((3,), 0.375, dtype=torch.float64))
    y = torch.rand(1, 1, 5, 7, dtype=torch.float64)  # both odd: x00 / 4
    assert sr.pool(y).shape == (1, 1, 3, 4) and float(sr.pool(y)[0, 0, 0, 0]) == float(y[0, 0, 0, 0]) / 4
    for t in (x, y):  # ... and it is torch's own avg_pool2d with the reference's arguments
        want = F.avg_pool2d(t, 2, 2, padding=(t.shape[2] % 2, t.shape[3] % 2), count_include_pad=True)
        assert torch.allclose(sr.pool(t), want, rtol=0, atol=1e-15)


def test_the_window_is_the_stated_gaussian():
    g = sr.window(torch.float64)
    e = [math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)]
    assert g.numel() == 11 and abs(float(g.sum()) - 1) < 1e-15
    assert max(abs(float(g[i]) - e[i] / sum(e)) for i in range(11)) < 1e-16


WRONG = {"sigma_1.0": dict(sigma=1.0), "9_taps": dict(taps=9), "same_padding": dict(same=True)}


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("shape", sr.SHAPES)
def test_the_tolerance_tells_the_algorithm_from_its_near_misses(shape, kind):
    """On the GPU test's own inputs: another sigma, another window length or "same" padding moves at least one checked
    quantity by more than 100 x its bound.  (`same` cannot tell: every variant gives 1; `flat` has the widest bound,
    the fp32 restatement itself being 1e-4 off there.)"""
    h, w, L = shape
    a, b = sr.make_pair(kind, 2, h, w)
    r64, e32, tol = sr.tolerance(a, b, L)
    for name, kw in WRONG.items():
        v = sr.metrics(a, b, L, torch.float64, **kw)
        ratio = max(float((x - y).abs().max()) / t for x, y, t in zip(v, r64, tol) if t is not None)
        print(shape, kind, name, "moves a quantity by %.0f x its bound" % ratio)
        assert ratio > 100, (name, ratio)


def test_the_tolerance_tells_the_pooling_rule():
    """Odd-axis pooling that drops the last column instead of padding in front: 161 -> 80 -> 40 -> 20 (-> 10, where it
    has no window left, so 4 levels are compared) moves a raw value by more than 100 x its bound on `noise`.  The wrong
    rule shifts BOTH pooled pictures by half a pixel, which re-draws every pooled pixel of `noise`.  A known limit of the
    `smooth` input: only its 12-level noise part is re-drawn, the sinusoid (period > 30 pixels) barely moves, and the
    figure there is 70 x; it is printed, not asserted."""
    for kind in ("noise", "smooth"):
        a, b = sr.make_pair(kind, 2, 176, 161)
        r64, e32, tol = sr.tolerance(a, b, 4)
        lv = sr.levels(a, b, 4, torch.float64, pool_pad=False)
        assert bool((lv[:, 0] == r64[0][:, 0]).all())  # (level 0 is not pooled)
        ratio = float((lv - r64[0]).abs().max()) / tol[0]
        print(kind, "dropped padding moves a raw value by %.0f x its bound" % ratio)
        if kind == "noise":
            assert ratio > 100


# ---- run_metrics' host logic
def _ref_ssim_levels(a, b, levels):
    return sr.levels(a.cpu().numpy(), b.cpu().numpy(), levels, torch.float64)


def _png(path, arr):
    Image.fromarray(arr).save(str(path), "PNG")


@pytest.fixture
def tree(tmp_path, monkeypatch):
    monkeypatch.setattr(metrics, "ssim_levels", _ref_ssim_levels)
    res = tmp_path / "results"
    (res / "gt").mkdir(parents=True)
    (res / "samples").mkdir()
    pics = {}
    small = sr.make_pair("smooth", 3, 64, 48, seed=1)   # min side <= 160: MSSIM is NaN
    big = sr.make_pair("smooth", 2, 176, 161, seed=2)
    for i in range(3):
        pics["s_%d.png" % i] = (small[0][i], small[1][i])
    for i in range(2):
        pics["b_%d.png" % i] = (big[0][i], big[1][i])
    for name, (g, s) in pics.items():
        _png(res / "gt" / name, g)
        _png(res / "samples" / name, s)
    return res, pics


def _read(res):
    with open(str(res / "metrics.csv"), newline="") as f:
        rows = list(csv.reader(f))
    txt = open(str(res / "metrics.txt")).read().splitlines()
    return rows, txt


def test_run_metrics_writes_the_table(tree):
    res, pics = tree
    out = evaluate.run_metrics(res, batch_size=2)
    rows, txt = _read(res)
    assert rows[0] == ["name", "SSIM", "MSSIM"]
    assert [r[0] for r in rows[1:]] == sorted(pics)  # two sizes in one directory, every picture once, in name order
    assert out["n"] == 5 and out["skipped"] == []
    for name, s, m in rows[1:]:
        g, smp = pics[name]
        lv, ws, wm = sr.metrics(smp[None], g[None], 5 if name.startswith("b_") else 1)
        assert abs(float(s) - float(ws)) < 1e-12, name
        if name.startswith("b_"):
            assert abs(float(m) - float(wm)) < 1e-12, name
        else:
            assert math.isnan(float(m)), name  # 64 x 48
    s_mean = np.mean([float(r[1]) for r in rows[1:]])
    m_mean = np.mean([float(r[2]) for r in rows[1:] if not math.isnan(float(r[2]))])  # the mean ignores the NaNs
    assert len(txt) == 2 and txt[0].startswith("SSIM: ") and txt[1].startswith("MSSIM: ")
    assert abs(float(txt[0].split(": ")[1]) - s_mean) < 1e-12 and abs(float(txt[1].split(": ")[1]) - m_mean) < 1e-12
    assert abs(out["SSIM"] - s_mean) < 1e-12 and abs(out["MSSIM"] - m_mean) < 1e-12


def test_run_metrics_pairs_by_name_and_skips_what_has_no_ground_truth(tree):
    res, pics = tree
    os.remove(str(res / "gt" / "s_1.png"))                       # missing
    _png(res / "gt" / "s_2.png", pics["b_0.png"][0])             # another size
    (res / "gt" / "b_1.png").write_bytes(b"not a picture")       # unreadable
    _png(res / "gt" / "unpaired.png", pics["s_0.png"][0])        # a ground truth without a sample is not a row
    (res / "samples" / "notes.txt").write_text("ignored")
    out = evaluate.run_metrics(res)
    rows, _ = _read(res)
    assert [r[0] for r in rows[1:]] == ["b_0.png", "s_0.png"] and out["n"] == 2
    assert out["skipped"] == ["b_1.png", "s_1.png", "s_2.png"]  # left out, NOT replaced by their neighbours
    g, smp = pics["s_0.png"]
    assert abs(float(rows[2][1]) - float(sr.metrics(smp[None], g[None], 1)[1])) < 1e-12


def test_run_metrics_takes_the_two_directories_and_writes_next_to_the_samples(tree, tmp_path):
    res, pics = tree
    other = tmp_path / "elsewhere" / "samples"
    other.mkdir(parents=True)
    _png(other / "s_0.png", pics["s_0.png"][1])
    out = evaluate.run_metrics(gt_dir=res / "gt", sample_dir=other)
    assert out["n"] == 1 and os.path.exists(str(tmp_path / "elsewhere" / "metrics.csv"))
    assert os.path.exists(str(tmp_path / "elsewhere" / "metrics.txt")) and not os.path.exists(str(res / "metrics.csv"))
    assert math.isnan(out["MSSIM"])
    with pytest.raises(ValueError):
        evaluate.run_metrics()


def test_host_tensors_are_refused():
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    for fn in (metrics.ssim, metrics.ms_ssim, lambda x, y: metrics.ssim_levels(x, y, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 17" in design and "upk_ssim_u8" in design
    assert "run_metrics" in open(os.path.join(ROOT, "README.md")).read()
    assert "eval_metrics.py" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
