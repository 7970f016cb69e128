"""upk_lpips_input_f16 / upk_relu_pool_nhwc_f16 / upk_lpips_layer_f16, upgpt_amd.lpips.LPIPS, metrics.lpips and run_metrics'
LPIPS column on the MI355X, against tests/lpips_ref.py.  All weights are synth.synthetic_lpips_state.

End-to-end tolerance, from the reference alone: gap = max over the cases of |emu16 - ref64| / ref64 (emu16: the fp16
storage of the device pipeline, restated on the CPU), and every pair's every layer value must satisfy |device - ref64| /
ref64 <= 4 * gap; the factor 4 is the margin for what emu16 does not model, the MFMA accumulation order and fp16 split-K
slabs, each a rounding of the size of emu16's own.  Measured (one MI355X run): gap = 5.13e-3, max |device - ref64| / ref64 = 6.2e-3
(1.2 x gap).  tests/test_lpips_host.py shows that this tolerance tells the algorithm from its near misses.  Every comparison prints its figures before it asserts."""
import csv
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import lpips_ref as lr
from upgpt_amd import _lib, evaluate, metrics, synth
from upgpt_amd.lpips import LPIPS, SCALE, SHIFT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def sd():
    return synth.synthetic_lpips_state(0)


@pytest.fixture(scope="module")
def net(sd):
    m = LPIPS()
    m.load_state_dict(sd)
    return m.to(DEV)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


# ---- input kernel
def _scaled(x, normalize):
    """torch's fp32 expression of the scaling layer (lpips: normalize, then (x - shift) / scale), then .half()."""
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    if normalize:
        x = 2 * x - 1
    return ((x - shift) / scale).half()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("source", ["u8", "f32"])
@pytest.mark.parametrize("window", [False, True], ids=["20x17", "44x28_in_strip"])
def test_input_kernel_is_bit_exact(ctx, window, source, normalize):
    n = 2
    h, w = (44, 28) if window else (20, 17)
    g = torch.Generator().manual_seed(h + 2 * int(normalize))
    if source == "u8":
        if window:  # a window at odd offsets of a wider, taller strip
            strip = torch.randint(0, 256, (n, h + 5, 3 * w + 7, 3), generator=g, dtype=torch.uint8)
            pic = strip[:, 3:3 + h, 5:5 + w]
        else:
            strip = pic = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        want = _scaled(pic.permute(0, 3, 1, 2).float() / 255, normalize)
        dstrip = strip.to(DEV)
        src = dstrip[:, 3:3 + h, 5:5 + w] if window else dstrip
        args = (src, False, src.stride(1), src.stride(0))
    else:
        x = torch.rand(n, 3, h, w, generator=g) * 1.2 - 0.1
        want = _scaled(x, normalize)
        big = torch.full((n, 2, 3, h, w), 7.0)
        big[:, 0] = x
        dbig = big.to(DEV)
        src = dbig[:, 0] if window else x.to(DEV)  # (window: a sample stride larger than one sample)
        args = (src, True, 0, src.stride(0))
    y = torch.full((n, 2, h * w, 32), -3.0, dtype=torch.float16, device=DEV)  # interleaved: sample i at y[i, 0]
    ctx.lpips_input(*args, n, h, w, normalize, SHIFT + SCALE, y, 2 * h * w * 32)
    torch.cuda.synchronize()
    got = y[:, 0].cpu()
    assert torch.equal(bits(got[..., :3]), bits(want.permute(0, 2, 3, 1).reshape(n, h * w, 3)))
    assert bool((got[..., 3:] == 0).all()) and bool((bits(got[..., 3:]) == 0).all())  # pad channels: +0
    assert bool((y[:, 1] == -3.0).all())  # the other picture's slots are not touched


def test_input_kernel_refuses_bad_arguments(ctx):
    y = torch.empty(2, 16 * 16, 32, dtype=torch.float16, device=DEV)
    a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    ok = (a, False, 48, 768, 2, 16, 16, False)
    for bad in ((a, False, 47, 768, 2, 16, 16, False, SHIFT + SCALE, y, 16 * 16 * 32),     # pitch < 3 w
                (a, False, 48, 700, 2, 16, 16, False, SHIFT + SCALE, y, 16 * 16 * 32),     # samples overlap
                ok + (SHIFT + (0.0, 1.0, 1.0), y, 16 * 16 * 32),                           # scale 0
                ok + (SHIFT + SCALE, y, 16 * 16 * 32 - 8),                                 # outputs overlap
                (a, False, 48, 768, 2, 0, 16, False, SHIFT + SCALE, y, 16 * 16 * 32)):
        with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
            ctx.lpips_input(*bad)


# ---- ReLU / pool kernel
@pytest.mark.parametrize("shape", [(2, 11, 7, 64, 64), (1, 5, 3, 512, 512), (2, 11, 7, 64, 96)], ids=["2x11x7x64", "1x5x3x512", "ld96"])
def test_relu_pool_is_bit_exact(ctx, shape):
    b, h, w, c, ld = shape
    g = torch.Generator().manual_seed(h * w + c)
    x = (torch.randn(b, h, w, ld, generator=g) * 3).half()
    x[torch.rand(b, h, w, ld, generator=g) < 0.1] = 0  # negative, zero and positive values, no inf
    want = F.relu(x[..., :c].float()).half()
    want_p = F.max_pool2d(want.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).half()
    dx = x.to(DEV)
    ldp = c + 8
    pooled = torch.full((b, h // 2, w // 2, ldp), -3.0, dtype=torch.float16, device=DEV)
    ctx.relu_pool(dx, ld, b, h, w, c, pooled, ldp)
    torch.cuda.synchronize()
    assert torch.equal(bits(dx[..., :c]), bits(want))
    assert torch.equal(bits(dx[..., c:]), bits(x[..., c:]))  # the gap of ld > c is untouched
    assert torch.equal(bits(pooled[..., :c]), bits(want_p)) and bool((pooled[..., c:] == -3.0).all())
    # the dropped odd row / column has no influence on the pooled values; without `pooled` only the ReLU happens
    x2 = x.clone()
    x2[:, h - 1] = 100.0
    x2[:, :, w - 1] = 100.0
    dx2, pooled2 = x2.to(DEV), torch.empty_like(pooled)
    ctx.relu_pool(dx2, ld, b, h, w, c, pooled2, ldp)
    dx3 = x.to(DEV)
    ctx.relu_pool(dx3, ld, b, h, w, c)
    torch.cuda.synchronize()
    assert torch.equal(bits(pooled2[..., :c]), bits(want_p)) and torch.equal(bits(dx3), bits(dx))
    with pytest.raises(_lib.UpkError, match="UPK_ESHAPE"):
        ctx.relu_pool(dx, ld, b, h, w, c - 4, pooled, ldp)
    with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
        ctx.relu_pool(dx, c - 8, b, h, w, c, pooled, ldp)


# ---- layer kernel
def _layer(ctx, f0, f1, w, layer=0):
    n, hw, c = f0.shape
    both = torch.stack([f0, f1], 1).to(DEV)  # [n, 2, hw, c]: the pictures of a pair next to each other, as LpipsPlan lays them
    nbytes = ctx.lpips_ws_bytes(n, hw, c)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((n, 5), -1.0, dtype=torch.float32, device=DEV)
    ctx.lpips_layer(both, both[0, 1], c, 2 * hw * c, n, hw, c, w.to(DEV), layer, out, ws, nbytes)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("hw", lr.LAYER_HW)
@pytest.mark.parametrize("c", lr.LAYER_C)
def test_layer_kernel_against_fp64_on_the_same_fp16_inputs(ctx, c, hw):
    f0, f1, w = lr.layer_features(c, hw)
    want, bound = lr.layer_ref(f0, f1, w), lr.layer_bound(c, hw)
    layer = (c // 64 + hw) % 5
    out = _layer(ctx, f0, f1, w, layer)
    got = out[:, layer].double()
    err = float(((got - want).abs() / want).max())
    print("C = %d hw = %d: relative error %.2e, bound %.2e" % (c, hw, err, bound))
    assert bool(torch.isfinite(got).all()) and err <= bound
    others = [l for l in range(5) if l != layer]
    assert bool((out[:, others] == -1.0).all())  # only column `layer` is written
    # reruns are bit-identical; pair 1 alone has the bits it has inside the batch
    assert torch.equal(_layer(ctx, f0, f1, w, layer), out)
    assert torch.equal(_layer(ctx, f0[1:2], f1[1:2], w, layer)[0, layer], out[1, layer])


def test_layer_kernel_zero_pixels_and_refusals(ctx):
    z = torch.zeros(2, 15, 64, dtype=torch.float16)
    w = torch.full((64,), 1.0 / 64)
    assert bool((_layer(ctx, z, z, w)[:, 0] == 0).all())  # all-zero pixels: 0, not NaN
    f0, _, _ = lr.layer_features(64, 15)
    one = _layer(ctx, f0, z[:1].expand(3, -1, -1).contiguous(), w)[:, 0]  # against zero features: mean_p sum_c w f^0_c^2
    assert bool(torch.isfinite(one).all())
    d = f0.to(DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    out = torch.empty(3, 5, device=DEV)
    with pytest.raises(_lib.UpkError, match="UPK_ESHAPE"):
        ctx.lpips_layer(d, d, 96, 15 * 96, 1, 10, 96, w.to(DEV), 0, out, ws, 64)
    with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
        ctx.lpips_layer(d, d, 64, 15 * 64, 3, 15, 64, w.to(DEV), 5, out, ws, 64)
    with pytest.raises(_lib.UpkError, match="UPK_EWORKSPACE"):
        ctx.lpips_layer(d, d, 64, 15 * 64, 3, 15, 64, w.to(DEV), 0, out, ws, 8)


# ---- end to end
def _check(tag, got, r64, gap):
    rel = ((got.double().cpu() - r64).abs() / r64)
    print("%-34s gap = %.3e  tolerance = %.3e  max |device - ref64| / ref64 = %.3e (per layer: %s)" % (
        tag, gap, 4 * gap, float(rel.max()), " ".join("%.1e" % v for v in rel.max(0).values.tolist())))
    assert bool(torch.isfinite(got).all()) and float(rel.max()) <= 4 * gap, (tag, float(rel.max()), gap)


def test_end_to_end_against_the_fp64_restatement(net, sd):
    cases, gap = lr.case_refs(sd)
    for a, b, r64, _ in cases:
        da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        lv = net.pairs_u8(da, db)
        assert lv.shape == (a.shape[0], 5) and lv.dtype == torch.float32 and lv.is_cuda
        _check("pairs_u8 %s" % (a.shape,), lv, r64, gap)
        assert torch.equal(net.pairs_u8(da, db), lv)  # a rerun is bit-identical
        tot = metrics.lpips(da, db, net)
        assert tot.shape == (a.shape[0],) and torch.equal(tot, lv.double().sum(1).float())
        assert torch.equal(metrics.lpips_layers(da, db, net), lv)


def test_forward_on_floats_and_normalize(net, sd):
    cases, gap = lr.case_refs(sd)
    a, b, r64, _ = cases[0]
    x, y = lr.to_unit(a, torch.float32), lr.to_unit(b, torch.float32)
    out = net(x.to(DEV), y.to(DEV))
    assert out.shape == (a.shape[0], 1, 1, 1) and out.dtype == torch.float32
    _check("forward(u / 255)", net.layers(x.to(DEV), y.to(DEV)), r64, gap)
    tot = net.pairs_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).double().sum(1)
    rel = float(((out.flatten().double() - tot).abs() / tot).max())
    print("forward against pairs_u8(...).sum(1): %.3e" % rel)
    assert rel <= 4 * gap
    rn = lr.lpips_layers(sd, lr.to_unit(a), lr.to_unit(b), normalize=True)
    _check("forward(normalize=True)", net.layers(x.to(DEV), y.to(DEV), normalize=True), rn, gap)
    with pytest.raises(ValueError):
        net(x[:, :, :15].to(DEV), y[:, :, :15].to(DEV))


def test_passes_do_not_change_a_bit(sd):
    a, b = lr.make_pairs(3, 44, 28)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    outs = []
    for ppp in (2, 16):
        m = LPIPS(pairs_per_pass=ppp)
        m.load_state_dict(sd)
        outs.append(m.to(DEV).pairs_u8(da, db))
    assert torch.equal(outs[0], outs[1])


def test_strided_windows_give_the_bits_of_dense_copies(net):
    a, b = lr.make_pairs(2, 44, 28)
    dense = net.pairs_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).clone()
    strip = torch.full((2, 44, 4 * 28, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    strip[:, :, 28:56] = torch.from_numpy(a).to(DEV)
    strip[:, :, 84:112] = torch.from_numpy(b).to(DEV)
    assert torch.equal(net.pairs_u8(strip[:, :, 28:56], strip[:, :, 84:112]), dense)


# ---- run_metrics with synthetic weight files
def test_run_metrics_writes_the_lpips_column(tmp_path, sd, net):
    vgg = {"features.%s.%s" % tuple(k.split(".")[2:]): v for k, v in sd.items() if k.startswith("net.")}
    vgg["classifier.6.bias"] = torch.zeros(3)
    torch.save(vgg, str(tmp_path / "vgg16.pth"))
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, str(tmp_path / "lin.pth"))
    res = tmp_path / "results"
    (res / "gt").mkdir(parents=True)
    (res / "samples").mkdir()
    pics = {}
    for tag, (n, h, w) in (("a", (3, 44, 28)), ("b", (2, 12, 12))):
        s, g = lr.make_pairs(n, h, w, seed=3)
        for i in range(n):
            pics["%s%d.png" % (tag, i)] = (g[i], s[i])
            Image.fromarray(g[i]).save(str(res / "gt" / ("%s%d.png" % (tag, i))))
            Image.fromarray(s[i]).save(str(res / "samples" / ("%s%d.png" % (tag, i))))
    out = evaluate.run_metrics(res, batch_size=2, device=0, lpips=(tmp_path / "vgg16.pth", tmp_path / "lin.pth"))
    with open(str(res / "metrics.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["name", "SSIM", "LPIPS", "MSSIM"] and [r[0] for r in rows[1:]] == sorted(pics)
    vals = []
    for name, _, lp, _ in rows[1:]:
        g, s = pics[name]
        if name.startswith("b"):
            assert math.isnan(float(lp)), name  # 12 x 12: below the 16-pixel minimum
            continue
        want = metrics.lpips(torch.from_numpy(s[None]).to(DEV), torch.from_numpy(g[None]).to(DEV), net)
        assert float(lp) == float(want.double()[0]) or abs(float(lp) - float(want[0])) <= 1e-7 * float(want[0]), name
        vals.append(float(lp))
    txt = open(str(res / "metrics.txt")).read().splitlines()
    assert len(txt) == 3 and txt[0].startswith("SSIM: ") and txt[1].startswith("MSSIM: ") and txt[2].startswith("LPIPS: ")
    assert abs(float(txt[2].split(": ")[1]) - np.mean(vals)) < 1e-12 and abs(out["LPIPS"] - np.mean(vals)) < 1e-12
    again = evaluate.run_metrics(res, batch_size=100, device=0, lpips=net)  # an instance, one batch per size
    assert again["LPIPS"] == out["LPIPS"] and again["n"] == 5
