"""LPIPS (VGG16), the parts that need no GPU: the ABI declaration / binding / build list of the three entry points, closed
forms that pin the restatement tests/lpips_ref.py, the key mapping of the two public weight files, that the GPU tests'
tolerances tell the algorithm from its near misses, and that run_metrics without weights writes what it wrote before."""
import csv
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import lpips_ref as lr
import ssim_ref as sr
from upgpt_amd import _lib, build, evaluate, metrics, synth
from upgpt_amd.lpips import LPIPS, SCALE, SHIFT, param_shapes, state_from_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (("upk_lpips_input_f16", "int", 13), ("upk_relu_pool_nhwc_f16", "int", 10), ("upk_lpips_ws_bytes", "size_t", 3),
       ("upk_lpips_layer_f16", "int", 14))


@pytest.fixture(scope="module")
def sd():
    return synth.synthetic_lpips_state(0)


def test_header_declares_and_library_exports_the_symbols():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    lib = _lib.load_library()
    for name, ret, nargs in NEW:
        assert name in _lib.SYMBOLS
        proto = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(proto.split(",")) == nargs, name
    assert lib.upk_version() == 100  # additive: the ABI version stays
    section = header[header.index("LPIPS (VGG16) of picture pairs"):header.index("int upk_lpips_layer_f16")]
    assert "never allocate, never synchronise, are graph-capturable" in section and 'class "other"' in section
    assert "lpips.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lpips.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS.get("lpips.hip", [])


def test_ws_bytes_needs_no_device_and_refuses_bad_arguments():
    lib = _lib.load_library()
    assert lib.upk_lpips_ws_bytes(1, 1, 64) == 16 and lib.upk_lpips_ws_bytes(3, 176, 512) > 0
    assert lib.upk_lpips_ws_bytes(100, 45056, 64) > lib.upk_lpips_ws_bytes(2, 45056, 64) > 0
    for bad in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (1, 16, 96), (1, 16, 1024), (-1, 16, 512)):
        assert lib.upk_lpips_ws_bytes(*bad) == 0, bad


# ---- closed forms of the restatement
def test_identical_pictures_give_exactly_zero_and_the_value_is_symmetric(sd):
    a, b = lr.make_pairs(2, 20, 17)
    x, y = lr.to_unit(a), lr.to_unit(b)
    for mode in ("ref64", "emu16"):
        assert bool((lr.lpips_layers(sd, x, x.clone(), mode=mode) == 0).all())
        v, vt = lr.lpips_layers(sd, x, y, mode=mode), lr.lpips_layers(sd, y, x, mode=mode)
        assert bool((v > 0).all()) and torch.equal(v, vt)
    assert torch.equal(lr.lpips(sd, x, y), lr.lpips_layers(sd, x, y).sum(1))


def test_zero_conv_weights_give_constant_features_and_zero(sd):
    z = {k: (torch.zeros_like(v) if k.startswith("net.") and k.endswith(".weight") else v.clone()) for k, v in sd.items()}
    a, b = lr.make_pairs(2, 16, 16)
    v = lr.lpips_layers(z, lr.to_unit(a), lr.to_unit(b))  # every feature is relu(bias): the same in both pictures
    assert bool((v == 0).all())


def test_one_layer_by_hand():
    """Two pixels, two channels (the kernel's C is not needed for the formula): f0 = (3, 4), (0, 0); f1 = (0, 5), (1, 0);
    w = (0.5, 0.25).  Pixel 0: f^0 = (.6, .8), f^1 = (0, 1): .5 * .36 + .25 * .04 = .19.  Pixel 1: f^0 = 0 (0 / (0 + eps)),
    f^1 = (1, 0): .5.  Mean: .345.  With the eps inside the root the numbers are the same to 1e-10; a pixel of norm 1e-6
    is what tells the two: 1e-6 / (1e-6 + 1e-10) against 1e-6 / sqrt(1e-12 + 1e-10)."""
    f0 = torch.tensor([[[3.0, 4.0], [0.0, 0.0]]]).permute(0, 2, 1).unsqueeze(-1)
    f1 = torch.tensor([[[0.0, 5.0], [1.0, 0.0]]]).permute(0, 2, 1).unsqueeze(-1)
    w = torch.tensor([0.5, 0.25])
    assert abs(float(lr.layer_distance(f0, f1, w)) - 0.345) < 1e-9
    g0, g1 = torch.tensor([1e-6, 0.0]).view(1, 2, 1, 1), torch.tensor([0.0, 1.0]).view(1, 2, 1, 1)
    out = float(lr.layer_distance(g0, g1, w))
    want = 0.5 * (1e-6 / (1e-6 + 1e-10)) ** 2 + 0.25 * (1 / (1 + 1e-10)) ** 2
    assert abs(out - want) < 1e-12
    inside = float(lr.layer_distance(g0, g1, w, eps_inside=True))
    assert abs(inside - (0.5 * (1e-6 / (1.01e-10) ** 0.5) ** 2 + 0.25 * (1 / (1 + 1e-10) ** 0.5) ** 2)) < 1e-9 and inside < 0.26 < out


def test_the_scaling_layer_and_the_floor_pool_are_the_stated_ones(sd):
    assert SHIFT == (-.030, -.088, -.188) and SCALE == (.458, .448, .450)
    assert sd["scaling_layer.shift"].flatten().tolist() == [np.float32(v) for v in SHIFT]
    assert lr.SLICES == ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28)) and lr.CHANNELS == (64, 128, 256, 512, 512)
    x = torch.arange(35.0).view(1, 1, 5, 7)
    p = torch.nn.functional.max_pool2d(x, 2, 2)
    assert p.shape == (1, 1, 2, 3) and float(p[0, 0, 1, 2]) == 26.0  # rows 2..3, columns 4..5: row 4 and column 6 are dropped


# ---- key mapping
def _files(tmp_path, sd, alias=False, drop=None):
    vgg = {"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4)}
    for k, v in sd.items():
        if k.startswith("net."):
            _, _, i, leaf = k.split(".")
            vgg["features.%s.%s" % (i, leaf)] = v
    lin = {(k.replace("lin", "lins.", 1) if alias else k): v for k, v in sd.items() if k.startswith("lin")}
    for d in (vgg, lin):
        d.pop(drop, None)
    torch.save(vgg, str(tmp_path / "vgg16.pth"))
    torch.save(lin, str(tmp_path / "vgg_lin.pth"))
    return tmp_path / "vgg16.pth", tmp_path / "vgg_lin.pth"


def test_the_two_files_load_into_the_tensors_of_the_lpips_style_dict(tmp_path, sd):
    assert set(sd) == set(LPIPS().state_dict()) and len(param_shapes()) == 31
    direct = LPIPS()
    full = dict(sd)
    full.update({k.replace("lin", "lins.", 1): v for k, v in sd.items() if k.startswith("lin")})  # lpips' own dict has both
    direct.load_state_dict(full)
    for alias in (False, True):
        m = LPIPS.from_files(*_files(tmp_path, sd, alias=alias))
        got, want = m.state_dict(), direct.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]) and torch.equal(got[k], sd[k]), k
    only_alias = {(k.replace("lin", "lins.", 1) if k.startswith("lin") else k): v for k, v in sd.items()}
    m = LPIPS()
    m.load_state_dict(only_alias)
    assert torch.equal(m.state_dict()["lin3.model.1.weight"], sd["lin3.model.1.weight"])


def test_a_missing_key_raises(tmp_path, sd):
    with pytest.raises(KeyError, match="features.14.bias"):
        LPIPS.from_files(*_files(tmp_path, sd, drop="features.14.bias"))
    with pytest.raises(KeyError, match="lin2"):
        LPIPS.from_files(*_files(tmp_path, sd, drop="lin2.model.1.weight"))
    part = {k: v for k, v in sd.items() if k != "net.slice4.19.weight"}
    with pytest.raises(RuntimeError, match="net.slice4.19.weight"):
        LPIPS().load_state_dict(part)
    with pytest.raises(KeyError, match="net.slice4.19.weight"):
        LPIPS().load_state_dict(part, strict=False)
    with pytest.raises(RuntimeError, match="classifier"):
        LPIPS().load_state_dict(dict(sd, **{"classifier.0.weight": torch.zeros(1)}))


# ---- the tolerances tell the algorithm from its near misses
def test_the_end_to_end_tolerance_tells_the_near_misses(sd):
    """On the GPU test's own cases, with its tolerance 4 * gap: the input mapped to [-1, 1], no scaling layer, taps before
    the ReLU and ceil-mode pooling each move a checked value by more than the tolerance.  The fifth near miss, the eps
    inside the square root, moves nothing end to end (1e-10 against norms of order 1: 1e-10 relative); it is told by
    the layer kernel's own cases and bound, see the next test."""
    cases, gap = lr.case_refs(sd)
    print("gap = %.3e, tolerance = %.3e" % (gap, 4 * gap))
    assert 0 < gap < 0.05
    for name in ("pm1", "no_scaling", "pre_relu", "ceil_pool"):
        moved = 0.0
        for a, b, r64, _ in cases:
            v = lr.lpips_layers(sd, lr.to_unit(a), lr.to_unit(b), **{name: True})
            moved = max(moved, float(((v - r64).abs() / r64).max()))
        print("%-10s moves a value by %.3e = %.1f x the tolerance" % (name, moved, moved / (4 * gap)))
        assert moved > 4 * gap, (name, moved, gap)
    for a, b, r64, _ in cases:
        assert bool((r64 > 1e-7).all())  # well away from 0: the comparison is relative


def test_the_layer_bound_tells_where_the_eps_stands():
    """The layer kernel's cases with 15 and 176 pixels hold pixels whose norm is of the order of the eps (exact fp16
    subnormals): sqrt(s + eps) instead of sqrt(s) + eps moves every such case by more than 5 x its bound."""
    for c in lr.LAYER_C:
        for hw in (15, 176):
            f0, f1, w = lr.layer_features(c, hw)
            r, m = lr.layer_ref(f0, f1, w), lr.layer_ref(f0, f1, w, eps_inside=True)
            ratio = float(((m - r).abs() / r).min()) / lr.layer_bound(c, hw)
            print("C = %d hw = %d: eps inside the root moves d by %.0f x the bound" % (c, hw, ratio))
            assert ratio > 5, (c, hw, ratio)
            assert bool(torch.isfinite(r).all()) and bool((r > 0).all())


# ---- run_metrics without weights: what it wrote before
def test_run_metrics_without_weights_writes_the_three_columns_and_two_lines(tmp_path, monkeypatch):
    monkeypatch.setattr(metrics, "ssim_levels", lambda a, b, levels: sr.levels(a.cpu().numpy(), b.cpu().numpy(), levels, torch.float64))
    monkeypatch.delenv("UPGPT_LPIPS_VGG", raising=False)
    monkeypatch.delenv("UPGPT_LPIPS_LIN", raising=False)
    res = tmp_path / "results"
    (res / "gt").mkdir(parents=True)
    (res / "samples").mkdir()
    g, s = sr.make_pair("smooth", 2, 64, 48, seed=1)
    for i in range(2):
        Image.fromarray(g[i]).save(str(res / "gt" / ("p%d.png" % i)))
        Image.fromarray(s[i]).save(str(res / "samples" / ("p%d.png" % i)))
    out = evaluate.run_metrics(res)
    assert sorted(out) == ["MSSIM", "SSIM", "n", "skipped"]
    with open(str(res / "metrics.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["name", "SSIM", "MSSIM"] and all(len(r) == 3 for r in rows)
    want = sr.metrics(s, g, 1)[1]
    assert [r[1] for r in rows[1:]] == [repr(float(v)) for v in want]
    txt = open(str(res / "metrics.txt")).read()
    assert txt == "SSIM: %r\nMSSIM: nan\n" % float(np.mean([float(v) for v in want]))
    monkeypatch.setenv("UPGPT_LPIPS_VGG", "only_one.pth")
    with pytest.raises(ValueError, match="UPGPT_LPIPS_LIN"):
        evaluate.run_metrics(res)


def test_host_tensors_are_refused(sd):
    net = LPIPS()
    net.load_state_dict(sd)
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    x = torch.zeros(1, 3, 16, 16)
    for fn in (lambda: metrics.lpips(a, a, net), lambda: metrics.lpips_layers(a, a, net), lambda: net.pairs_u8(a, a),
               lambda: net(x, x), lambda: net(x, x, normalize=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    with pytest.raises(TypeError):
        metrics.lpips(a, a, None)


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 17" in design and "## 18" in design and "upk_lpips_layer_f16" in design
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "LPIPS and FID are not computed" not in text and "FID is not computed" in text, doc
    assert "FID is not computed" in evaluate.run_metrics.__doc__
