"""upk_ssim_u8 / upgpt_amd.metrics / evaluate.run_metrics on the MI355X against tests/ssim_ref.py in fp64.

Tolerance, from the reference alone: per case and quantity (the raw [L, 3, 2] values, SSIM, MS-SSIM) e32 = max |fp32
restatement - fp64 restatement|, and the device must satisfy |device - fp64| <= 4 * e32 + 5e-6 (4: the same arithmetic
class in another summation order; 5e-6: 1 / 20 of the fourth decimal papers report, which is what `same` is held to,
its e32 being 0).  tests/test_metrics_host.py shows that this bound tells the algorithm from its near misses.
Every comparison prints case, e32 and the device's error before it asserts."""
import csv

import numpy as np
import pytest
import torch
from PIL import Image

import ssim_ref as sr
from upgpt_amd import _lib, evaluate, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
_REF = {}


def case(kind, n, h, w, levels):
    """(a, b, fp64 results, e32, bounds), computed once per case and shared."""
    key = (kind, n, h, w, levels)
    if key not in _REF:
        a, b = sr.make_pair(kind, n, h, w)
        _REF[key] = (a, b) + sr.tolerance(a, b, levels)
    return _REF[key]


def dev(x):
    return torch.from_numpy(x).to(DEV)


def check(tag, lv, r64, e32, tol):
    """lv: the device's raw [N, L, 3, 2]; compares raw, SSIM and MS-SSIM."""
    lv = lv.cpu()
    got = (lv.double(), metrics.ssim_from_levels(lv), metrics.ms_ssim_from_levels(lv) if lv.shape[1] == 5 else None)
    errs = []
    for name, g, want, e, t in zip(("raw", "SSIM", "MS-SSIM"), got, r64, e32, tol):
        if want is None:
            continue
        err = float((g - want).abs().max())
        print("%-28s %-8s e32 = %.2e  bound = %.2e  device error = %.2e" % (tag, name, e, t, err))
        errs.append((name, err, t))
    for name, err, t in errs:
        assert err <= t, (tag, name, err, t)


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_against_the_fp64_restatement(shape, kind):
    h, w, levels = shape
    a, b, r64, e32, tol = case(kind, 2, h, w, levels)
    lv = metrics.ssim_levels(dev(a), dev(b), levels)
    check("%s %s B=2" % (shape, kind), lv, r64, e32, tol)


def test_batch_of_five_and_the_public_functions():
    a, b, r64, e32, tol = case("smooth", 5, 176, 161, 5)
    da, db = dev(a), dev(b)
    lv = metrics.ssim_levels(da, db, 5)
    check("(176, 161, 5) smooth B=5", lv, r64, e32, tol)
    s, m = metrics.ssim(da, db), metrics.ms_ssim(da, db)
    assert s.shape == m.shape == (5,) and s.is_cuda and m.is_cuda
    assert float((s.cpu().double() - r64[1]).abs().max()) <= tol[1]
    assert float((m.cpu().double() - r64[2]).abs().max()) <= tol[2]
    # determinism: a rerun is bit-identical, and sample k alone gives the bits it has inside the batch
    assert torch.equal(metrics.ssim_levels(da, db, 5), lv)
    for k in range(5):
        assert torch.equal(metrics.ssim_levels(da[k:k + 1], db[k:k + 1], 5)[0], lv[k]), k
    with pytest.raises(ValueError):
        metrics.ms_ssim(da[:, :160], db[:, :160])
    with pytest.raises(ValueError):
        metrics.ssim_levels(da, db, 6)
    with pytest.raises(ValueError):
        metrics.ssim_levels(da[:, :10], db[:, :10], 1)


@pytest.mark.parametrize("shape", [(23, 37, 1), (176, 161, 5)], ids=lambda s: "%dx%dx%d" % s)
def test_strided_windows_give_the_bits_of_dense_copies(shape):
    """a and b as two column windows of one strip (pitch 4 * 3 * w), and b as a view whose sample stride is larger than
    one picture."""
    h, w, levels = shape
    a, b = case("smooth", 2, h, w, levels)[:2]
    dense = metrics.ssim_levels(dev(a), dev(b), levels)
    strip = torch.full((2, h, 4 * w, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    strip[:, :, w:2 * w] = dev(a)
    strip[:, :, 3 * w:] = dev(b)
    va, vb = strip[:, :, w:2 * w], strip[:, :, 3 * w:]
    assert va.stride(1) == 4 * 3 * w and not va.is_contiguous()
    assert torch.equal(metrics.ssim_levels(va, vb, levels), dense)
    wide = torch.full((2, 3, h, w, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    wide[:, 1] = dev(b)
    assert wide[:, 1].stride(0) == 3 * h * w * 3
    assert torch.equal(metrics.ssim_levels(dev(a), wide[:, 1], levels), dense)


def _raw_call(ctx, a, b, n, h, w, levels, out, ws, ws_bytes, override=None):
    """upk_ssim_u8 on dense pictures; override: arguments of Context.ssim_u8 to replace."""
    args = dict(a=a, a_pitch=3 * w, a_ss=3 * w * h, b=b, b_pitch=3 * w, b_ss=3 * w * h, batch=n, h=h, w=w, levels=levels,
                out=out, ws=ws, ws_bytes=ws_bytes)
    args.update(override or {})
    ctx.ssim_u8(**args)


@pytest.mark.parametrize("shape", [(12, 27, 1), (176, 161, 5)], ids=lambda s: "%dx%dx%d" % s)
def test_nothing_outside_out_and_ws_is_written(ctx, shape):
    h, w, levels = shape
    n = 2
    a, b, r64, e32, tol = case("noise", n, h, w, levels)
    nbytes = ctx.ssim_ws_bytes(n, h, w, levels)
    assert nbytes > 0
    slack = 4096
    ws = torch.full((nbytes + slack,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = torch.full((n * levels * 6 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    _raw_call(ctx, dev(a), dev(b), n, h, w, levels, out, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == SENTINEL).all())
    assert bool(torch.isnan(out[n * levels * 6:]).all()) and not bool(torch.isnan(out[:n * levels * 6]).any())
    check("%s noise raw ABI" % (shape,), out[:n * levels * 6].view(n, levels, 3, 2), r64, e32, tol)


def test_error_codes(ctx):
    h, w, n = 32, 48, 2
    a = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=DEV)
    b = torch.zeros_like(a)
    nbytes = ctx.ssim_ws_bytes(n, h, w, 1)
    ws = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n * 2 * 6 + 4, dtype=torch.float32, device=DEV)
    _raw_call(ctx, a, b, n, h, w, 1, out, ws, nbytes)  # (the baseline is valid)
    torch.cuda.synchronize()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
    bad = [(dict(a=None), EINVAL), (dict(b=None), EINVAL), (dict(out=None), EINVAL), (dict(ws=None), EINVAL),
           (dict(batch=0), EINVAL), (dict(h=0), EINVAL), (dict(w=-1), EINVAL), (dict(levels=0), EINVAL), (dict(levels=6), EINVAL),
           (dict(a_pitch=3 * w - 1), EINVAL), (dict(b_pitch=3 * w - 1), EINVAL),
           (dict(a_ss=3 * w * h - 1), EINVAL), (dict(b_ss=0), EINVAL),  # overlapping samples
           (dict(out=out.data_ptr() + 2), EINVAL), (dict(ws=ws.data_ptr() + 4), EINVAL),  # misaligned
           (dict(levels=3), ESHAPE), (dict(h=10), ESHAPE), (dict(w=10, a_pitch=30, b_pitch=30), ESHAPE),  # 32 x 48 -> 8 x 12
           (dict(levels=2), EWORKSPACE),  # (16 x 24 is a level, but ws holds one level only)
           (dict(ws_bytes=nbytes - 1), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE)]
    before = ctx.lib.upk_kernel_launches(ctx.h, 0)
    for kw, code in bad:
        with pytest.raises(_lib.UpkError) as e:
            _raw_call(ctx, a, b, n, h, w, 1, out, ws, nbytes, override=kw)
        assert e.value.code == code, (kw, e.value.code)
        assert (ctx.lib.upk_last_error(ctx.h) or b"") != b"", kw
    assert ctx.lib.upk_kernel_launches(ctx.h, 0) == before  # a refused call launches nothing
    _raw_call(ctx, a, b, n, h, w, 1, out, ws, nbytes)
    assert ctx.lib.upk_kernel_launches(ctx.h, 0) == before + 2  # level kernel + final pass
    torch.cuda.synchronize()


def test_graph_replay_follows_the_inputs(ctx):
    h, w, levels, n = 176, 161, 5, 2
    a, b = case("smooth", n, h, w, levels)[:2]
    a2, b2 = case("noise", n, h, w, levels)[:2]
    direct1 = metrics.ssim_levels(dev(a), dev(b), levels)
    direct2 = metrics.ssim_levels(dev(a2), dev(b2), levels)
    da, db = dev(a), dev(b)
    nbytes = ctx.ssim_ws_bytes(n, h, w, levels)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((n, levels, 3, 2), float("nan"), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.graph_begin()
        _raw_call(ctx, da, db, n, h, w, levels, out, ws, nbytes)
        g = ctx.graph_end()
        s.synchronize()
        assert bool(torch.isnan(out).all())  # (captured, not run)
        ctx.graph_launch(g)
        s.synchronize()
        first = out.clone()
        da.copy_(dev(a2))  # the pictures are overwritten in place
        db.copy_(dev(b2))
        ctx.graph_launch(g)
        s.synchronize()
        second = out.clone()
    s.synchronize()
    ctx.graph_destroy(g)
    assert torch.equal(first, direct1) and torch.equal(second, direct2) and not torch.equal(first, second)


def test_run_metrics_end_to_end(tmp_path):
    res = tmp_path / "results"
    (res / "gt").mkdir(parents=True)
    (res / "samples").mkdir()
    pics = {}
    for tag, (h, w) in (("big", (176, 161)), ("small", (64, 48))):
        gt, smp = case("smooth", 2, h, w, 5 if tag == "big" else 1)[:2]
        for i in range(2):
            pics["%s_%d.png" % (tag, i)] = (gt[i], smp[i])
    for name, (g, s) in pics.items():  # PNG: lossless, the decoded files are these arrays
        Image.fromarray(g).save(str(res / "gt" / name))
        Image.fromarray(s).save(str(res / "samples" / name))
    Image.fromarray(pics["small_0.png"][1]).save(str(res / "samples" / "orphan.png"))
    out = evaluate.run_metrics(res, batch_size=100)
    assert out["n"] == 4 and out["skipped"] == ["orphan.png"]
    with open(str(res / "metrics.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["name", "SSIM", "MSSIM"] and [r[0] for r in rows[1:]] == sorted(pics)
    for name, s, m in rows[1:]:
        g, smp = pics[name]
        levels = 5 if name.startswith("big") else 1
        r64, e32, tol = sr.tolerance(smp[None], g[None], levels)
        err = abs(float(s) - float(r64[1]))
        print("%-12s SSIM    e32 = %.2e  bound = %.2e  device error = %.2e" % (name, e32[1], tol[1], err))
        assert err <= tol[1]
        if levels == 5:
            err = abs(float(m) - float(r64[2]))
            print("%-12s MS-SSIM e32 = %.2e  bound = %.2e  device error = %.2e" % (name, e32[2], tol[2], err))
            assert err <= tol[2]
        else:
            assert np.isnan(float(m))
    txt = open(str(res / "metrics.txt")).read().splitlines()
    s_mean = np.mean([float(r[1]) for r in rows[1:]])
    m_mean = np.mean([float(r[2]) for r in rows[1:] if not np.isnan(float(r[2]))])
    assert txt[0].startswith("SSIM: ") and abs(float(txt[0][6:]) - s_mean) < 1e-12
    assert txt[1].startswith("MSSIM: ") and abs(float(txt[1][7:]) - m_mean) < 1e-12
    assert abs(out["SSIM"] - s_mean) < 1e-12 and abs(out["MSSIM"] - m_mean) < 1e-12
