"""upk_conv2d_rect_f16 / upk_pool3_nhwc_f16 / upk_fid_input_f16 / upk_avgpool_global_f32, upgpt_amd.fid.FIDInception and
run_metrics' FID line on the MI355X, against tests/fid_ref.py.  All weights are synth.synthetic_fid_state.

Kernel bounds (each derived where it is used): the convolution |device - ref64| <= 2^-11 |ref64| + K 2^-24 conv(|x|, |w|), the
average pool 2^-11 |ref64| + 9 * 2^-24 |ref64|, the input 2^-12 + 2^-20 absolute, the global mean (hw + 2) 2^-24 relative.
End to end, from the reference alone: the error of a picture is e = max_c |device_c - ref64_c| / max_c |ref64_c|, gap = max
over the cases of e(emu16) (emu16: the fp16 storage of the device pipeline, restated on the CPU), and every picture must
satisfy e(device) <= 4 gap; the factor 4 is the margin for what emu16 does not model, the MFMA accumulation order, each a
rounding of the size of emu16's own.  tests/test_fid_host.py shows that this tolerance tells the algorithm
from its near misses.  Measured (one MI355X run): gap = 1.295e-3, max e(device) = 1.02e-3 = 0.79 gap.  Every comparison
prints its figures before it asserts."""
import csv
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import fid_ref as fr
from upgpt_amd import _lib, evaluate, metrics, synth
from upgpt_amd.fid import FIDInception

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -3.0


@pytest.fixture(scope="module")
def sd():
    return synth.synthetic_fid_state(0)


@pytest.fixture(scope="module")
def refs(sd):
    return fr.case_refs(sd)


@pytest.fixture(scope="module")
def net(sd):
    m = FIDInception()
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.fixture(scope="module")
def dev_feats(net, refs):
    """{case: device features [n, 2048] on the host}: features_u8 for the resized case, forward(resize_input=False) else."""
    out = {}
    for name, n, h, w, resize in fr.CASES:
        u8 = refs[0][name][0]
        if resize:
            out[name] = net.features_u8(torch.from_numpy(u8).to(DEV)).cpu()
        else:
            out[name] = net(fr.to_unit(u8, torch.float32).to(DEV), resize_input=False).cpu()
    return out


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).cpu()


# ---- convolution
def _conv_operands(kh, kw, cin, cout, b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    cp = (cin + 31) // 32 * 32
    x = torch.zeros(b, h, w, cp, dtype=torch.float16)
    x[..., :cin] = torch.randn(b, h, w, cin, generator=g).half()  # both signs; the pad channels are zero, as in the network
    wt = (torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (kh * kw * cin))).half()
    bias = (0.3 * torch.randn(cout, generator=g)).float()
    return x, wt, bias, cp


def _run_conv(ctx, x, packed, n_pad, bias_d, geom, cout, cp, off=16, extra=48):
    kh, kw, s, ph, pw = geom
    b, h, w, _ = x.shape
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    y = torch.full((b * ho * wo, cout + extra), SENT, dtype=torch.float16, device=DEV)
    ctx.conv2d_rect(x, cp, b, h, w, cp, kh, kw, s, ph, pw, packed, cout, n_pad, bias_d, True, y.data_ptr() + 2 * off, y.shape[1])
    torch.cuda.synchronize()
    return y, ho, wo


@pytest.mark.parametrize("case", fr.conv_cases(), ids=lambda c: "k%dx%d_s%d_p%d%d_%dx%d_b%d_%d-%d" % c)
def test_conv2d_rect_against_fp64(ctx, case):
    kh, kw, s, ph, pw, h, w, b, cin, cout = case
    x, wt, bias, cp = _conv_operands(kh, kw, cin, cout, b, h, w, seed=fr.conv_cases().index(case))
    xn = x[..., :cin].permute(0, 3, 1, 2).double()
    pre = F.conv2d(xn, wt.double(), bias.double(), stride=s, padding=(ph, pw))
    ref = F.relu(pre)
    absref = F.conv2d(xn.abs(), wt.double().abs(), None, stride=s, padding=(ph, pw))
    bound = fr.conv_bound(ref, absref, kh * kw * cp)  # one fp16 rounding + fp32 accumulation of K = kh kw cin_pad terms
    packed, n_pad = ctx.pack_weight(wt.float().contiguous().to(DEV), cin_packed=cp)
    bias_d = torch.zeros(n_pad, dtype=torch.float32, device=DEV)
    bias_d[:cout] = bias.to(DEV)
    xd = x.to(DEV)
    y, ho, wo = _run_conv(ctx, xd, packed, n_pad, bias_d, (kh, kw, s, ph, pw), cout, cp)
    got = y[:, 16:16 + cout].cpu().double().view(b, ho, wo, cout).permute(0, 3, 1, 2)
    err = (got - ref).abs()
    cut = float((pre < 0).double().mean())
    print("conv %s: M = %d, K = %d, ReLU cuts %.0f %%, max |diff| %.3e, max diff / bound %.3f" % (
        case, b * ho * wo, kh * kw * cp, 100 * cut, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert 0.2 < cut < 0.8  # the ReLU cuts
    assert bool((err <= bound).all())
    assert bool((y[:, :16] == SENT).all()) and bool((y[:, 16 + cout:] == SENT).all())  # the neighbouring slices are untouched
    y2, _, _ = _run_conv(ctx, xd, packed, n_pad, bias_d, (kh, kw, s, ph, pw), cout, cp)
    assert torch.equal(bits(y2), bits(y))  # a rerun
    y1, _, _ = _run_conv(ctx, xd[1:2].contiguous(), packed, n_pad, bias_d, (kh, kw, s, ph, pw), cout, cp)
    hw = ho * wo
    assert torch.equal(bits(y1[:, 16:16 + cout]), bits(y[hw:2 * hw, 16:16 + cout]))  # picture 1 alone has the bits it has in the batch


def test_conv2d_rect_refusals(ctx):
    x = torch.zeros(2, 9, 7, 32, dtype=torch.float16, device=DEV)
    wt = torch.zeros(32, 32, 3, 3, device=DEV)
    packed, n_pad = ctx.pack_weight(wt, cin_packed=32)
    bias = torch.zeros(n_pad, device=DEV)
    y = torch.zeros(2 * 9 * 7, 64, dtype=torch.float16, device=DEV)

    def call(x_=x, ldx=32, h=9, w=7, cp=32, kh=3, kw=3, s=1, ph=1, pw=1, n_out=32, y_=y, ldy=64):
        ctx.conv2d_rect(x_, ldx, 2, h, w, cp, kh, kw, s, ph, pw, packed, n_out, n_pad, bias, True, y_, ldy)

    call()  # the arguments the refusals below vary are accepted
    for kw_ in (dict(kh=8), dict(kw=0), dict(s=3), dict(ph=4), dict(pw=-1), dict(cp=48, ldx=48), dict(n_out=n_pad + 1, ldy=128)):
        with pytest.raises(_lib.UpkError, match="UPK_ESHAPE"):
            call(**kw_)
    for kw_ in (dict(ldy=24), dict(x_=x.data_ptr() + 2), dict(y_=y.data_ptr() + 2), dict(ldx=24), dict(h=2, ph=0),
                dict(w=1, pw=0), dict(ldy=66)):
        with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
            call(**kw_)
    torch.cuda.synchronize()


# ---- pooling
POOL_SHAPES = ((2, 9, 7, 64, 64), (1, 8, 8, 288, 288), (2, 17, 17, 96, 128))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["2x9x7x64", "1x8x8x288", "2x17x17x96_ld128"])
def test_pool3_max_is_bit_exact_and_avg_within_bound(ctx, shape, stride):
    b, h, w, c, ld = shape
    g = torch.Generator().manual_seed(h * w + c + stride)
    pad = 1 if stride == 1 else 0
    ho, wo = (h, w) if stride == 1 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    ldy = c + 8
    for mode in (_lib.POOL_MAX, _lib.POOL_AVG):
        x = (torch.randn(b, h, w, ld, generator=g) * 3).half()
        if mode == _lib.POOL_AVG:
            x = x.abs()  # what the network's pools read is behind a ReLU; with one sign 9 * 2^-24 |ref| bounds the fp32 sum
        y = torch.full((b, ho, wo, ldy), SENT, dtype=torch.float16, device=DEV)
        ctx.pool3(x.to(DEV), ld, b, h, w, c, mode, stride, y, ldy)
        torch.cuda.synchronize()
        xn = x[..., :c].permute(0, 3, 1, 2)
        got = y[..., :c].cpu()
        assert bool((y[..., c:] == SENT).all())  # the gap of ld > c is untouched
        if mode == _lib.POOL_MAX:
            want = F.max_pool2d(xn.float(), 3, stride, pad).permute(0, 2, 3, 1).half()
            assert torch.equal(bits(got), bits(want))
            continue
        ref = F.avg_pool2d(xn.double(), 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1)
        err = (got.double() - ref).abs()
        bound = (2.0 ** -11 + 9 * 2.0 ** -24) * ref.abs()  # fp32 sum of at most 9 terms of one sign, one division, one fp16 rounding
        print("avg pool %s stride %d: max |diff| %.3e, max diff / bound %.3f" % (shape, stride, float(err.max()),
                                                                                 float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all())
        if stride == 1:  # the in-picture divisor, explicitly: 4 taps in a corner, 6 on an edge
            xd = x[..., :c].double()
            for (oy, ox), (ys, xs), div in ((((0, 0)), (slice(0, 2), slice(0, 2)), 4), ((0, w - 1), (slice(0, 2), slice(w - 2, w)), 4),
                                            ((h - 1, 0), (slice(h - 2, h), slice(0, 2)), 4),
                                            ((h - 1, w - 1), (slice(h - 2, h), slice(w - 2, w)), 4),
                                            ((0, 3), (slice(0, 2), slice(2, 5)), 6), ((h - 1, 3), (slice(h - 2, h), slice(2, 5)), 6),
                                            ((3, 0), (slice(2, 5), slice(0, 2)), 6), ((3, w - 1), (slice(2, 5), slice(w - 2, w)), 6)):
                want = xd[:, ys, xs].sum((1, 2)) / div
                e = (got[:, oy, ox].double() - want).abs()
                assert bool((e <= (2.0 ** -11 + 9 * 2.0 ** -24) * want).all()), (oy, ox, div)
                assert float(want.min()) > 0 and bool(((got[:, oy, ox].double() - want * div / 9).abs() > e).any())  # not / 9


def test_pool3_refusals(ctx):
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV)
    y = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV)
    for bad in ((x, 64, 1, 8, 8, 60, 0, 1, y, 64), (x, 64, 1, 8, 8, 64, 0, 3, y, 64), (x, 64, 1, 2, 8, 64, 0, 2, y, 64)):
        with pytest.raises(_lib.UpkError, match="UPK_ESHAPE"):
            ctx.pool3(*bad)
    for bad in ((x, 56, 1, 8, 8, 64, 0, 1, y, 64), (x, 64, 1, 8, 8, 64, 2, 1, y, 64), (x, 64, 0, 8, 8, 64, 0, 1, y, 64),
                (x, 64, 1, 8, 8, 64, 0, 1, y.data_ptr() + 8, 64)):
        with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
            ctx.pool3(*bad)


# ---- input
INPUT_SIZES = ((20, 17, 299, 299), (44, 28, 31, 23), (40, 40, 13, 13), (16, 16, 16, 16))


@pytest.mark.parametrize("source", ["u8", "u8_window", "f32"])
@pytest.mark.parametrize("size", INPUT_SIZES, ids=["20x17_to_299", "44x28_to_31x23", "40x40_to_13", "16x16_copy"])
def test_fid_input_within_bound(ctx, size, source):
    h, w, oh, ow = size
    n = 2
    g = torch.Generator().manual_seed(h + ow + len(source))
    if source == "f32":
        x = torch.rand(n, 3, h, w, generator=g)
        src = x.to(DEV)
        args = (src, True, 0, src.stride(0))
        x64 = x.double()
    else:
        if source == "u8_window":  # a window at odd offsets of a wider, taller strip
            strip = torch.randint(0, 256, (n, h + 5, 3 * w + 7, 3), generator=g, dtype=torch.uint8)
            pic = strip[:, 3:3 + h, 5:5 + w]
            dstrip = strip.to(DEV)
            src = dstrip[:, 3:3 + h, 5:5 + w]
        else:
            pic = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
            src = pic.to(DEV)
        args = (src, False, src.stride(1), src.stride(0))
        x64 = pic.permute(0, 3, 1, 2).double() / 255
    ref = (2 * fr.resize_bilinear(x64, oh, ow) - 1).permute(0, 2, 3, 1).reshape(n, oh * ow, 3)
    y = torch.full((n, 2, oh * ow, 32), SENT, dtype=torch.float16, device=DEV)  # interleaved: sample i at y[i, 0]
    ctx.fid_input(*args, n, h, w, oh, ow, True, y, 2 * oh * ow * 32)
    torch.cuda.synchronize()
    got = y[:, 0].cpu()
    err = float((got[..., :3].double() - ref).abs().max())
    bound = 2.0 ** -12 + 2.0 ** -20  # half an fp16 ulp below 1, plus fp32 roundings of the operations on values of magnitude <= 1
    print("fid_input %s %s: max |diff| %.3e (bound %.3e)" % (size, source, err, bound))
    assert err <= bound
    assert bool((got[..., 3:] == 0).all()) and bool((bits(got[..., 3:]) == 0).all())  # pad channels: +0
    assert bool((y[:, 1] == SENT).all())  # the neighbouring slots are untouched
    if (h, w) == (oh, ow) and source != "f32":  # the copy: exactly fp16(2 (u / 255) - 1) in fp32
        assert torch.equal(bits(got[..., :3]), bits((2 * (pic.float() / 255) - 1).half().reshape(n, oh * ow, 3)))


def test_fid_input_refusals(ctx):
    a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    y = torch.empty(2, 8 * 8, 32, dtype=torch.float16, device=DEV)
    ctx.fid_input(a, False, 48, 768, 2, 16, 16, 8, 8, True, y, 8 * 8 * 32)
    for bad in ((a, False, 47, 768, 2, 16, 16, 8, 8, True, y, 8 * 8 * 32),      # pitch < 3 w
                (a, False, 48, 700, 2, 16, 16, 8, 8, True, y, 8 * 8 * 32),      # samples overlap
                (a, False, 48, 768, 2, 16, 16, 0, 8, True, y, 8 * 8 * 32),      # a zero output size
                (a, False, 48, 768, 2, 16, 16, 8, 0, True, y, 8 * 8 * 32),
                (a, False, 48, 768, 2, 16, 16, 8, 8, True, y, 8 * 8 * 32 - 8)):  # outputs overlap
        with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
            ctx.fid_input(*bad)
    torch.cuda.synchronize()


# ---- global mean
@pytest.mark.parametrize("c", [64, 2048])
@pytest.mark.parametrize("hw", [1, 9, 64])
def test_avgpool_global(ctx, hw, c):
    g = torch.Generator().manual_seed(hw + c)
    n, ld = 3, c + 8
    x = (torch.relu(torch.randn(n, hw, ld, generator=g)) * 2).half()  # post-ReLU values: one sign, about half of them zero
    ref = x[..., :c].double().mean(1)
    xd = x.to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((n, c), SENT, dtype=torch.float32, device=DEV)
        ctx.avgpool_global(xd, ld, n, hw, c, out)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    err = (outs[0].double() - ref).abs()
    bound = (hw + 2) * 2.0 ** -24 * ref  # fp32 sum of hw terms of one sign in a fixed order, one division
    print("global mean hw %d C %d: max |diff| %.3e, max diff / bound %.3f" % (hw, c, float(err.max()),
                                                                             float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    with pytest.raises(_lib.UpkError, match="UPK_EINVAL"):
        ctx.avgpool_global(xd, c - 8, n, hw, c, out)


# ---- end to end
def test_features_within_four_gaps_of_fp64(refs, dev_feats):
    cases, gap = refs
    tol = fr.MARGIN * gap
    worst = 0.0
    for name, (u8, r, e16, _) in cases.items():
        e = fr.picture_error(dev_feats[name], r)
        worst = max(worst, float(e.max()))
        print("%s: e(device) = %s, e(emu16) = %s" % (name, ["%.3e" % v for v in e.tolist()],
                                                      ["%.3e" % v for v in fr.picture_error(e16, r).tolist()]))
    print("gap = %.3e, tolerance 4 gap = %.3e, max e(device) = %.3e = %.2f gap" % (gap, tol, worst, worst / gap))
    for name, (u8, r, _, _) in cases.items():
        assert bool((fr.picture_error(dev_feats[name], r) <= tol).all()), name
        assert dev_feats[name].shape == (len(u8), 2048) and dev_feats[name].dtype == torch.float32


def test_forward_of_unit_floats_agrees_with_features_u8(net, refs, dev_feats):
    cases, gap = refs
    u8, r, _, _ = cases["44x28_resized"]
    got = net(fr.to_unit(u8, torch.float32).to(DEV)).cpu()
    e = fr.picture_error(got, r)
    e2 = fr.picture_error(got, dev_feats["44x28_resized"])
    print("forward(u / 255): e against ref64 %s, against features_u8 %s (tolerance %.3e)" % (e.tolist(), e2.tolist(), fr.MARGIN * gap))
    assert bool((e <= fr.MARGIN * gap).all()) and bool((e2 <= fr.MARGIN * gap).all())
    raw = net(fr.to_unit(u8, torch.float32).to(DEV) * 2 - 1, normalize_input=False).cpu()  # the caller's own 2 x - 1
    assert bool((fr.picture_error(raw, r) <= fr.MARGIN * gap).all())
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 74, 80, device=DEV), resize_input=False)
    with pytest.raises(TypeError):
        net(torch.zeros(1, 3, 80, 80, dtype=torch.uint8, device=DEV))


def test_features_are_bit_identical_across_reruns_passes_windows_and_batches(net, sd, refs, dev_feats):
    u8 = refs[0]["44x28_resized"][0]
    want = dev_feats["44x28_resized"]
    x = torch.from_numpy(u8).to(DEV)
    assert torch.equal(bits(net.features_u8(x)), bits(want))  # a rerun
    small = FIDInception(pictures_per_pass=2)
    small.load_state_dict(sd)
    small = small.to(DEV)
    assert torch.equal(bits(small.features_u8(x)), bits(want))  # passes of 2 + 1 against one pass of 3
    n, h, w = u8.shape[:3]
    strip = torch.full((n, h + 5, 3 * w + 7, 3), 9, dtype=torch.uint8, device=DEV)
    strip[:, 3:3 + h, 5:5 + w] = x
    assert torch.equal(bits(net.features_u8(strip[:, 3:3 + h, 5:5 + w])), bits(want))  # a strided window against its dense copy
    for i in range(n):
        assert torch.equal(bits(net.features_u8(x[i:i + 1])), bits(want[i:i + 1])), i  # picture i alone against picture i in the batch
    u75 = refs[0]["75x75"][0]
    one = net(fr.to_unit(u75[1:2], torch.float32).to(DEV), resize_input=False)
    assert torch.equal(bits(one), bits(dev_feats["75x75"][1:2]))
    with pytest.raises(RuntimeError):
        net.features_u8(torch.from_numpy(u8))  # host tensors raise


# ---- run_metrics
def _tree(tmp_path, sd):
    root = tmp_path / "results"
    (root / "gt").mkdir(parents=True)
    (root / "samples").mkdir()
    gt, smp = fr.make_pictures(5, 44, 28, seed=3), fr.make_pictures(5, 44, 28, seed=4)
    for i in range(5):
        Image.fromarray(gt[i]).save(str(root / "gt" / ("p%d.png" % i)))
        Image.fromarray(smp[i]).save(str(root / "samples" / ("p%d.png" % i)))
    for i, im in enumerate(fr.make_pictures(2, 12, 12, seed=5)):  # one set only: FID is unpaired
        Image.fromarray(im).save(str(root / "gt" / ("a_small%d.png" % i)))
    full = dict(sd)
    full["fc.weight"] = torch.zeros(1008, 2048)
    wpath = tmp_path / "pt_inception.pth"
    torch.save(full, str(wpath))
    return root, wpath


def _expected_fid(net, root):
    """fid_from_stats of fid_stats of features_u8 of the same files, in run_metrics' documented (height, width, name) order."""
    stats = []
    for d in ("gt", "samples"):
        files = sorted((root / d).iterdir(), key=lambda p: (evaluate._decode(p).shape[:2], p.name))
        feats = [net.features_u8(torch.from_numpy(np.array(evaluate._decode(p))[None]).to(DEV)).cpu() for p in files]
        stats.append(metrics.fid_stats(torch.cat(feats)))
    return metrics.fid_from_stats(*stats[0], *stats[1]), [len(list((root / d).iterdir())) for d in ("gt", "samples")]


def test_run_metrics_fid_line(tmp_path, sd, net, monkeypatch, capsys):
    monkeypatch.delenv("UPGPT_FID_INCEPTION", raising=False)
    for k in ("UPGPT_LPIPS_VGG", "UPGPT_LPIPS_LIN"):
        monkeypatch.delenv(k, raising=False)
    root, wpath = _tree(tmp_path, sd)
    plain = evaluate.run_metrics(str(root), batch_size=2)  # fid=None, the variable unset: what the parent commit writes
    txt0, csv0 = (root / "metrics.txt").read_bytes(), (root / "metrics.csv").read_bytes()
    assert "FID" not in plain and txt0.startswith(b"SSIM: ") and txt0.count(b"\n") == 2
    want, counts = _expected_fid(net, root)
    assert counts == [7, 5]
    vals = {}
    for bs in (2, 100):
        res = evaluate.run_metrics(str(root), batch_size=bs, fid=str(wpath))
        lines = (root / "metrics.txt").read_text().splitlines()
        assert lines[0].startswith("FID:  ") and lines[0] == "FID:  %r" % res["FID"]
        assert "\n".join(lines[1:]).encode() + b"\n" == txt0  # the SSIM / MSSIM lines follow unchanged
        assert (root / "metrics.csv").read_bytes() == csv0    # metrics.csv is not touched by FID
        vals[bs] = float(lines[0][len("FID:  "):])
        print("batch_size %d: FID %r, expected %r, relative difference %.3e" % (bs, vals[bs], want, abs(vals[bs] - want) / abs(want)))
        assert res["SSIM"] == plain["SSIM"] and res["n"] == 5
    assert all(abs(v - want) <= 1e-9 * abs(want) for v in vals.values()) and want > 0
    assert abs(vals[2] - vals[100]) <= 1e-9 * abs(want)
    inst = evaluate.run_metrics(str(root), batch_size=3, fid=net)  # an instance instead of a path
    assert abs(inst["FID"] - want) <= 1e-9 * abs(want)
    capsys.readouterr()
    assert evaluate.main(["--dir", str(root), "--fid_inception", str(wpath)]) == 0  # the command line prints FID first
    first = capsys.readouterr().out.splitlines()[0]
    assert first.startswith("FID:  ") and abs(float(first[len("FID:  "):]) - want) <= 1e-9 * abs(want)
    monkeypatch.setenv("UPGPT_FID_INCEPTION", str(wpath))
    assert abs(evaluate.run_metrics(str(root))["FID"] - want) <= 1e-9 * abs(want)
    monkeypatch.delenv("UPGPT_FID_INCEPTION")
    evaluate.run_metrics(str(root), batch_size=2)
    assert (root / "metrics.txt").read_bytes() == txt0 and (root / "metrics.csv").read_bytes() == csv0
    with open(str(root / "metrics.csv")) as f:
        assert next(csv.reader(f)) == ["name", "SSIM", "MSSIM"]


def test_run_metrics_set_of_one_picture_gives_nan(tmp_path, sd, net):
    root = tmp_path / "results"
    (root / "gt").mkdir(parents=True)
    (root / "samples").mkdir()
    pics = fr.make_pictures(3, 44, 28, seed=6)
    Image.fromarray(pics[0]).save(str(root / "samples" / "p0.png"))
    for i in range(3):
        Image.fromarray(pics[i]).save(str(root / "gt" / ("p%d.png" % i)))
    res = evaluate.run_metrics(str(root), fid=net)
    assert math.isnan(res["FID"]) and res["n"] == 1
    assert (root / "metrics.txt").read_text().splitlines()[0] == "FID:  nan"
