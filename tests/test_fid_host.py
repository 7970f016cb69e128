"""FID (InceptionV3), the parts that need no GPU: the ABI declaration / binding / build list of the four entry points, the
architecture tables against the restatement tests/fid_ref.py, the conditions the synthetic weights must meet, that the GPU
tests' tolerance tells the algorithm from its near misses, the host statistics (fid_stats, FidStats, fid_from_stats) against
closed forms with derived bounds, the state-dict handling, and that run_metrics without weights does not reach for any.
Every comparison prints its figures before it asserts."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as fr
from upgpt_amd import _lib, build, evaluate, metrics, synth
from upgpt_amd.fid import FIDInception, filter_state, param_shapes
from upgpt_amd.packing import fold_batchnorm, inception_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (("upk_conv2d_rect_f16", 20), ("upk_pool3_nhwc_f16", 12), ("upk_fid_input_f16", 14), ("upk_avgpool_global_f32", 8))


@pytest.fixture(scope="module")
def sd():
    return synth.synthetic_fid_state(0)


@pytest.fixture(scope="module")
def refs(sd):
    return fr.case_refs(sd)


def test_header_declares_and_library_exports_the_symbols():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    lib = _lib.load_library()
    for name, nargs in NEW:
        assert name in _lib.SYMBOLS
        proto = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(proto.split(",")) == nargs, name
    assert lib.upk_version() == 100  # additive: the ABI version stays
    section = header[header.index("FID features: InceptionV3"):header.index("int upk_avgpool_global_f32")]
    assert "never allocate, never synchronise and are graph-capturable" in section and "count_include_pad = False" in section
    assert "inception.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "inception.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS.get("inception.hip", [])


# ---- architecture
def test_param_shapes_are_the_public_files():
    shapes = param_shapes()
    assert shapes == fr.expected_shapes()  # (two tables written independently)
    convs = [k for k in shapes if k.endswith(".conv.weight")]
    assert len(convs) == 94 == len(inception_units()) and len(shapes) == 94 * 5
    for key, shape in (("Conv2d_1a_3x3", (32, 3, 3, 3)), ("Conv2d_3b_1x1", (80, 64, 1, 1)), ("Mixed_5b.branch5x5_2", (64, 48, 5, 5)),
                       ("Mixed_5b.branch_pool", (32, 192, 1, 1)), ("Mixed_5c.branch_pool", (64, 256, 1, 1)),
                       ("Mixed_6a.branch3x3", (384, 288, 3, 3)), ("Mixed_6b.branch7x7dbl_2", (128, 128, 7, 1)),
                       ("Mixed_6b.branch7x7_2", (128, 128, 1, 7)), ("Mixed_6e.branch7x7dbl_5", (192, 192, 1, 7)),
                       ("Mixed_7a.branch3x3_2", (320, 192, 3, 3)), ("Mixed_7b.branch3x3_2b", (384, 384, 3, 1)),
                       ("Mixed_7c.branch3x3dbl_1", (448, 2048, 1, 1))):
        assert shapes[key + ".conv.weight"] == shape, key
        assert shapes[key + ".bn.running_var"] == (shape[0],)
    m = FIDInception()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes


def test_reference_map_sizes(sd):
    tr = {}
    with torch.no_grad():
        out = fr.features(sd, torch.rand(1, 3, 20, 17, dtype=torch.float64), trace=tr)
    print("trunk sizes at 299:", tr["sizes"])
    assert tr["sizes"] == [149, 147, 147, 73, 73, 71, 35, 35, 35, 35, 17, 17, 17, 17, 17, 8, 8, 8]
    assert out.shape == (1, 2048)
    with torch.no_grad():
        out = fr.features(sd, torch.rand(2, 3, 75, 75, dtype=torch.float64), resize=False, trace=tr)
    print("trunk sizes at 75:", tr["sizes"])
    assert out.shape == (2, 2048) and tr["sizes"][-1] == 1
    with pytest.raises(RuntimeError):  # 74 x 74 leaves no pixel after Mixed_7a
        fr.features(sd, torch.rand(1, 3, 74, 74, dtype=torch.float64), resize=False)


def test_reference_resize_is_torchs_bilinear():
    x = torch.rand(2, 3, 44, 28, dtype=torch.float64)
    for size in ((299, 299), (31, 23), (13, 9), (44, 28)):
        for ac in (False, True):
            want = F.interpolate(x, size=size, mode="bilinear", align_corners=ac)
            err = float((fr.resize_bilinear(x, *size, align_corners=ac) - want).abs().max())
            print("resize", size, "align_corners", ac, "max |diff|", err)
            assert err <= 1e-12
    assert torch.equal(fr.resize_bilinear(x, 44, 28), x)  # equal sizes: a copy


# ---- conditions on the synthetic weights, from the reference alone
def test_synthetic_weights_stay_inside_fp16_and_keep_the_features_alive(refs):
    cases, gap = refs
    for name, (u8, r, e, amax) in cases.items():
        alive = (r > 1e-3 * r.amax(1, keepdim=True)).double().mean(1)
        print("%s: largest fp64 activation %.2f, features above 1e-3 of the picture's largest: %s" % (name, amax, alive.tolist()))
        assert amax < 2048  # a factor 32 inside fp16
        assert bool((alive >= 0.5).all())
    print("gap = max e(emu16) = %.3e" % gap)
    assert 0 < gap < 0.05


# ---- discrimination
@pytest.mark.parametrize("miss", [n for n, _ in fr.NEAR_MISSES])
def test_tolerance_tells_the_algorithm_from_its_near_misses(sd, refs, miss):
    cases, gap = refs
    tol = fr.MARGIN * gap
    kw = dict(fr.NEAR_MISSES)[miss]
    # align_corners acts in the resize, and Mixed_7c's pool tells max from average only on a map of more than one pixel (8 x 8
    # at 299; the unresized cases end at 1 x 1): the resized case, its first picture.  The others on the unresized small maps,
    # where a padding or divisor mistake is a large share of every output
    name = "44x28_resized" if miss in ("align_corners", "avg_7c") else "75x75"
    u8, r, _, _ = cases[name]
    n = 1 if name == "44x28_resized" else len(u8)
    with torch.no_grad():
        wrong = fr.features(sd, fr.to_unit(u8[:n]), resize=name == "44x28_resized", **kw)
    e = fr.picture_error(wrong, r[:n])
    print("%s on %s: e = %s = %s x tolerance (tolerance %.3e = %d x gap)" % (miss, name, e.tolist(), (e / tol).tolist(), tol, fr.MARGIN))
    assert bool((e > tol).all())


# ---- fid_from_stats
def test_fid_from_stats_commuting_covariances():
    """S_i = Q D_i Q^T: FID = |mu1 - mu2|^2 + sum (sqrt d1 - sqrt d2)^2.  The eigenvalue error is at most n^2 eps |A| ~ 4e-12
    |A| for n = 64, and sqrt is 1-Lipschitz above 0.25: bound 1e-9 (tr S1 + tr S2)."""
    rng = np.random.RandomState(3)
    n = 64
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d1, d2 = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    mu1, mu2 = rng.standard_normal(n), rng.standard_normal(n)
    s1, s2 = (q * d1) @ q.T, (q * d2) @ q.T
    want = float(((mu1 - mu2) ** 2).sum() + ((np.sqrt(d1) - np.sqrt(d2)) ** 2).sum())
    got = metrics.fid_from_stats(mu1, s1, mu2, s2)
    print("commuting: got %.15g, closed form %.15g, |diff| %.3e, bound %.3e" % (got, want, abs(got - want), 1e-9 * (d1.sum() + d2.sum())))
    assert abs(got - want) <= 1e-9 * (d1.sum() + d2.sum())
    assert abs(metrics.fid_from_stats(mu1, s1, mu1, s1)) <= 1e-9 * 2 * d1.sum()


def test_fid_from_stats_rank_deficient_sets():
    """N = 8 in dimension 32: 24 null eigenvalues, each perturbed by at most n eps |A|, contribute at most sqrt(32 * 2.2e-16) |S|
    ~ 8.4e-8 |S| each; times 48 that is 4e-6 |S|: |FID(X, X)| <= 1e-5 tr(S)."""
    rng = np.random.RandomState(5)
    x = rng.standard_normal((8, 32)) * rng.uniform(0.5, 2.0, 32)
    mu, s = metrics.fid_stats(x)
    v = metrics.fid_from_stats(mu, s, mu, s)
    print("rank-deficient: FID(X, X) = %.3e, bound %.3e" % (v, 1e-5 * np.trace(s)))
    assert abs(v) <= 1e-5 * np.trace(s)


def test_fid_stats_bookkeeping():
    rng = np.random.RandomState(7)
    x = np.abs(rng.standard_normal((11, 48))) * rng.uniform(0.1, 3.0, 48)
    mu, s = metrics.fid_stats(torch.from_numpy(x).float())  # (features arrive as fp32)
    x32 = x.astype(np.float32).astype(np.float64)
    wm, ws = np.mean(x32, 0), np.cov(x32, rowvar=False)
    e_mu, e_s = np.abs(mu - wm).max() / np.abs(wm).max(), np.abs(s - ws).max() / np.abs(ws).max()
    print("fid_stats against np.mean / np.cov: %.3e, %.3e" % (e_mu, e_s))
    assert e_mu <= 1e-12 and e_s <= 1e-12
    for cut in (1, 3, 11):
        acc = metrics.FidStats(48)
        for i in range(0, 11, cut):
            acc.add(torch.from_numpy(x32[i:i + cut]).float())
        am, a_s = acc.stats()
        e_mu, e_s = np.abs(am - wm).max() / np.abs(wm).max(), np.abs(a_s - ws).max() / np.abs(ws).max()
        print("accumulated in cuts of %d: %.3e, %.3e" % (cut, e_mu, e_s))
        assert acc.count == 11 and e_mu <= 1e-12 and e_s <= 1e-12
        assert np.array_equal(am, mu) and np.array_equal(a_s, s)  # (the order of the rows fixes every bit, not the cuts)
    big = np.abs(rng.standard_normal((150, 48))).astype(np.float32)  # more than two blocks of FidStats.CHUNK
    whole = metrics.fid_stats(big)
    e_s = np.abs(whole[1] - np.cov(big.astype(np.float64), rowvar=False)).max() / np.abs(whole[1]).max()
    print("150 rows against np.cov: %.3e" % e_s)
    assert e_s <= 1e-12
    for cut in (1, 7, 64, 100):
        acc = metrics.FidStats(48)
        for i in range(0, 150, cut):
            acc.add(big[i:i + cut])
        assert acc.count == 150 and all(np.array_equal(a, b) for a, b in zip(acc.stats(), whole)), cut
    one = metrics.FidStats(48).add(x32[:1]).stats()
    assert np.isnan(one[0]).all() and np.isnan(one[1]).all()
    assert np.isnan(metrics.fid_from_stats(*one, wm, ws))
    assert np.isnan(metrics.fid_stats(x32[:1])[1]).all()


# ---- state dicts
def test_state_dict_extras_are_ignored_and_a_missing_leaf_raises(sd, tmp_path):
    full = dict(sd)
    full["fc.weight"] = torch.zeros(1008, 2048)
    full["fc.bias"] = torch.zeros(1008)
    full["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    full["Mixed_6b.branch7x7dbl_3.bn.num_batches_tracked"] = torch.tensor(0)
    assert set(filter_state(full)) == set(param_shapes())
    m = FIDInception()
    m.load_state_dict(full)
    assert torch.equal(m.state_dict()["Mixed_6b.branch7x7dbl_3.bn.running_var"], sd["Mixed_6b.branch7x7dbl_3.bn.running_var"])
    path = tmp_path / "pt_inception.pth"
    torch.save(full, str(path))
    m2 = FIDInception.from_file(path, pictures_per_pass=2)
    assert m2.pictures_per_pass == 2 and all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    for gone in ("Mixed_6b.branch7x7dbl_3.bn.running_var", "Conv2d_1a_3x3.conv.weight"):
        part = {k: v for k, v in full.items() if k != gone}
        with pytest.raises(KeyError, match=re.escape(gone)):
            FIDInception().load_state_dict(part)
        with pytest.raises(KeyError):
            FIDInception().load_state_dict(part, strict=False)
    with pytest.raises(RuntimeError):  # host tensors: no CPU fallback
        m.features_u8(torch.zeros(1, 20, 20, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 80, 80))


def test_batchnorm_folding_equals_the_unfolded_unit(sd):
    u8 = fr.make_pictures(1, 75, 75)
    with torch.no_grad():
        a = fr.features(sd, fr.to_unit(u8), resize=False)
        b = fr.features(sd, fr.to_unit(u8), resize=False, folded=True)
    e = float(fr.picture_error(b, a).max())
    print("folded against unfolded BatchNorm, fp64: e = %.3e" % e)
    assert e <= 1e-12
    # the packer's fold is the reference's
    name = "Mixed_6b.branch7x7dbl_2"
    w, bias = fold_batchnorm(sd[name + ".conv.weight"], *[sd[name + "." + l] for l in ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")])
    rw, rb = fr.fold(sd, name)
    assert torch.equal(w, rw) and torch.equal(bias, rb)


# ---- run_metrics without weights
def test_run_metrics_without_fid_weights_does_not_reach_for_them(monkeypatch):
    monkeypatch.delenv("UPGPT_FID_INCEPTION", raising=False)
    assert evaluate._fid_net(None, torch.device("cpu")) is None
    with pytest.raises(TypeError):
        evaluate._fid_net(3, torch.device("cpu"))
    assert ".jpeg" in evaluate.FID_SUFFIXES and ".webp" in evaluate.FID_SUFFIXES and len(evaluate.FID_SUFFIXES) == 9
