"""The HIP kernels across the fp16 range: inputs scaled by 1, 2^6, 2^10 and 2^13 (up to ~3e4), against the fp64
references of tests/range_ref.py with their derived per-element bound (max |got - ref| / bound <= 1, printed per case),
exact power-of-two scaling of the linear family, and the behaviour at the edge of the range."""

import ctypes as C

import pytest
import torch

import range_ref as R
from test_ops_gpu import _phase_weights, geglu_row_map, make_desc
from test_xblock_gpu import head_cols
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)


def report(what, s, r):
    print("range %-34s scale %-5g max err/bound %.3f" % (what, s, r))
    return r


def families(ctx):
    """First-come order of the configurations of each family of upk_conv_config_name.  The names mirror the tables that
    build them: "bt..." bigtile.hip's BTCFG rows, "as..." astat.hip's ASCFG rows, and in igemm.hip's table a "w<n>" suffix
    marks the wave-specialised kernels (of which "...x1x1k<n>" are the K-split ones), no "w" the classic ones."""
    fam = {}
    for i in range(ctx.lib.upk_conv_num_configs()):
        n = ctx.lib.upk_conv_config_name(i).decode()
        key = "bt" if n.startswith("bt") else "as" if n.startswith("as") else "ksplit" if "x1x1k" in n else \
            "ws" if "w" in n else "classic"
        fam.setdefault(key, []).append(i)
    return fam


def run_conv(ctx, o, cfg=-1, sk=1):
    """Launches conv_case's operands; -> [B, Ho, Wo, N] on the CPU (fp16, or fp32 for the fp32 outputs).  Raises UpkError
    when the configuration refuses the launch."""
    B, N, Ho, Wo = o["B"], o["cout"], o["Ho"], o["Wo"]
    flags = {None: 0, "silu": L.F_SILU, "quickgelu": L.F_QUICKGELU}[o["act"]]
    flags |= (L.F_UPSAMPLE2X if o["ups"] else 0) | (L.F_PAD_ASYM if o["asym"] else 0)
    w = o["w"].to(DEV).contiguous()
    if o["out"] == "nchw_f32":
        y = torch.full((B, N, Ho, Wo), float("nan"), device=DEV)
        flags |= L.F_OUT_NCHW_F32
    else:
        y = torch.full((B, Ho, Wo, N), float("nan"), device=DEV, dtype=torch.float16)
    rv = o["rv"].to(DEV) if o["rowvec"] else None
    step = torch.tensor([o["rv_step"]], dtype=torch.int32, device=DEV) if o["rowvec"] else None
    d = make_desc(ctx, nhwc(o["x1"]), w, o["bias"].to(DEV), y, x2=nhwc(o["x2"]) if o["x2"] is not None else None,
                  stride=o["stride"], flags=flags, residual=o["resid"].to(DEV) if o["res"] else None, rowvec=rv,
                  rv_bs=N, rv_ss=B * N, step=step)
    keep = []
    if o["out"] == "nchw_f32":
        d.ldy = 0
    if o["phased"]:
        wph, n_pad = _phase_weights(ctx, w)
        assert n_pad == d.n_pad
        d.w_phase = wph.data_ptr()
        keep.append(wph)
    if o["seg"]:
        wp1, n1 = ctx.pack_weight(w)
        wp2, n2 = ctx.pack_weight(o["w2"].to(DEV).contiguous())
        assert n1 == n2
        wp = torch.cat([wp1.reshape(-1), wp2.reshape(-1)])
        x3 = nhwc(o["x3"])
        d.w_packed = wp.data_ptr()
        d.x3, d.c3, d.ld3 = x3.data_ptr(), x3.shape[-1], x3.shape[-1]
        keep += [wp, x3]
        if o["x4"] is not None:
            x4 = nhwc(o["x4"])
            d.x4, d.c4, d.ld4 = x4.data_ptr(), x4.shape[-1], x4.shape[-1]
            keep.append(x4)
    try:
        ctx.conv_override(cfg, sk)
        ctx.conv(d)
        torch.cuda.synchronize()
    finally:
        ctx.conv_override(-1, 0)
    out = y.cpu()
    return out.permute(0, 2, 3, 1) if o["out"] == "nchw_f32" else out


def run_gemm(ctx, o, sk=1, with_res=True, f32=False):
    M, K, N = o["M"], o["K"], o["N"]
    a = o["a"].to(DEV)
    geglu = o["act"] == "geglu"
    n_out = N // 2 if geglu else N
    rm = geglu_row_map(n_out).to(DEV) if geglu else None
    wp, n_pad = ctx.pack_weight(o["w"].to(DEV).contiguous(), row_map=rm)
    b = o["bias"].to(DEV)
    bp = torch.zeros(n_pad, device=DEV)
    bp[:N] = b[rm.long()] if geglu else b
    res = o["resid"].to(DEV) if (with_res and o["resid"] is not None) else None
    y = torch.full((M, n_out), float("nan"), device=DEV, dtype=torch.float32 if f32 else torch.float16)
    flags = {None: 0, "silu": L.F_SILU, "quickgelu": L.F_QUICKGELU, "geglu": L.F_GEGLU}[o["act"]] | (L.F_OUT_F32 if f32 else 0)
    try:
        ctx.conv_override(-1, sk)
        ctx.gemm(a, K, M, K, wp, n_out, n_pad, bp, res, n_out if res is not None else 0, y, n_out, flags)
        torch.cuda.synchronize()
    finally:
        ctx.conv_override(-1, 0)
    return y.cpu()


def configs_for(ctx, o):
    """The cost-model default plus the first configuration of each family that accepts the launch (unsplit)."""
    outs = {"default": None}
    for key, cfgs in families(ctx).items():
        for cfg in cfgs:
            try:
                run_conv(ctx, o, cfg, 1)
            except L.UpkError:
                continue
            outs[key] = cfg
            break
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# A. exact power-of-two scaling
def _assert_scaled(y0, yk, k, what, exact=True):
    y0, yk = y0.to(F64), yk.to(F64)
    assert torch.isfinite(yk).all(), what
    live = y0.abs() >= 2.0 ** -14  # (fp16-subnormal base outputs are excluded: they gain bits when scaled)
    assert float((~live).double().mean()) <= 1e-3, what
    want = y0 * 2.0 ** k
    if exact:
        bad = (yk != want) & live
        assert not bad.any(), "%s: %d elements are not 2^%d times the base output" % (what, int(bad.sum()), k)
    else:
        assert ((yk - want).abs() <= R.u16(want))[live].all(), what


@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_conv_scales_exactly_by_powers_of_two(ctx, name):
    base = R.conv_case(name, 1)
    cfgs = configs_for(ctx, base)
    assert len(cfgs) >= 2, cfgs
    for key, cfg in cfgs.items():
        y0 = run_conv(ctx, base, -1 if cfg is None else cfg, 1)
        for k in (6, 10, 12):
            yk = run_conv(ctx, R.conv_case(name, 2 ** k), -1 if cfg is None else cfg, 1)
            _assert_scaled(y0, yk, k, "%s %s k=%d" % (name, key, k))
    ran = 0
    for sk in (2, 3):
        try:
            y0 = run_conv(ctx, base, -1, sk)
        except L.UpkError:
            continue
        for k in (6, 10, 12):
            _assert_scaled(y0, run_conv(ctx, R.conv_case(name, 2 ** k), -1, sk), k, "%s sk=%d k=%d" % (name, sk, k),
                           exact=False)
        ran += 1
    assert ran >= 1, "%s: neither split-K 2 nor 3 was accepted" % name
    print("range %-34s families %s, split-K launches %d" % (name, sorted(cfgs), ran))


@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_scales_exactly_by_powers_of_two(ctx, name):
    base = R.gemm_case(name, 1)
    for f32 in (False, True):
        y0 = run_gemm(ctx, base, 1, with_res=not f32, f32=f32)
        for k in (6, 10, 12):
            yk = run_gemm(ctx, R.gemm_case(name, 2 ** k), 1, with_res=not f32, f32=f32)
            _assert_scaled(y0, yk, k, "%s f32=%s k=%d" % (name, f32, k))
    for sk in (2, 3):
        y0 = run_gemm(ctx, base, sk)
        for k in (6, 10, 12):
            _assert_scaled(y0, run_gemm(ctx, R.gemm_case(name, 2 ** k), sk), k, "%s sk=%d k=%d" % (name, sk, k), exact=False)


# ---------------------------------------------------------------------------------------------------------------------
# B. fp64 parity with the derived bound
@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_conv_against_fp64(ctx, name, s):
    o = R.conv_case(name, s)
    split = 0
    for sk in (1, 2, 3):
        try:
            got = run_conv(ctx, o, -1, sk)
        except L.UpkError:
            assert sk > 1, name
            continue
        split += sk > 1
        ref, bound = R.conv_case_ref(o, splitk=sk)
        assert float(ref.abs().max()) < 6e4
        r = R.ratio(got, ref, bound)
        if o["phased"]:
            # the launch must have taken the four-phase form: its reference reads the phase weights (fp16 of the summed
            # taps), the 3x3 form's reference the 3x3 weights; the other form's ratio is printed for comparison only
            print("      (against the 3x3 form's reference: %.3f)" % R.ratio(got, *R.conv_case_ref(dict(o, phased=False), splitk=sk)))
        assert report("%s sk=%d" % (name, sk), s, r) <= 1
    assert split >= 1, "%s: neither split-K 2 nor 3 was accepted" % name


@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("act", ["silu", "quickgelu"])
def test_conv_and_gemm_activations_against_fp64(ctx, act, s):
    o = R.conv_case("c3x3_64_224", s, act=act)
    ref, bound = R.conv_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    pre, _ = R.conv_case_ref(dict(o, act=None))
    assert float(pre.min()) < -2.5 * s and float(pre.max()) > 2.5 * s  # both tails of the sigmoid
    for key, cfg in configs_for(ctx, o).items():
        assert report("conv %s %s" % (act, key), s, R.ratio(run_conv(ctx, o, -1 if cfg is None else cfg, 1), ref, bound)) <= 1
    g = R.gemm_case("g96_896_224", s, act=act)
    ref, bound = R.gemm_case_ref(g)
    assert float(ref.abs().max()) < 6e4
    assert report("gemm %s" % act, s, R.ratio(run_gemm(ctx, g), ref, bound)) <= 1


@pytest.mark.parametrize("s", R.SCALES)
def test_gemm_against_fp64(ctx, s):
    for name in R.GEMM_CASES:
        o = R.gemm_case(name, s)
        for sk in (1, 2, 3):
            ref, bound = R.gemm_case_ref(o, splitk=sk)
            assert float(ref.abs().max()) < 6e4
            assert report("%s sk=%d" % (name, sk), s, R.ratio(run_gemm(ctx, o, sk), ref, bound)) <= 1
        ref, bound = R.gemm_case_ref(o, out="f32", with_res=False)
        assert report("%s fp32 out" % name, s, R.ratio(run_gemm(ctx, o, 1, with_res=False, f32=True), ref, bound)) <= 1
    o = R.gemm_case("geglu96_224", s, act="geglu", shape=(96, 224, 2 * 896), value_gain=R.GEGLU_VALUE_GAIN / s)
    ref, bound = R.gemm_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    assert report("geglu96_224", s, R.ratio(run_gemm(ctx, o), ref, bound)) <= 1


@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("name", list(R.GN_CASES))
def test_groupnorm_against_fp64(ctx, name, s):
    c = R.gn_case(name, s)
    B, hw, Cc = c["x"].shape
    c1, c2 = c["c1"], c["c2"]
    xa = c["x"][..., :c1].contiguous().to(DEV)
    xb = c["x"][..., c1:].contiguous().to(DEV) if c2 else None
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    ws = torch.zeros(ctx.groupnorm_ws_bytes(B, hw) // 4, device=DEV)
    # per-(row block, channel) partials as a producer's epilogue leaves them: fp32 sums of the fp16 values, 3 blocks of 16
    nblk = 3
    def partials(x):
        xf = x.float().view(B, nblk, hw // nblk, x.shape[-1])
        return torch.stack([xf.sum(2), (xf * xf).sum(2)], 2).contiguous()  # [B][nblk][2][c]
    pa, pb = partials(xa), (partials(xb) if c2 else None)
    d64 = lambda t: t.to(F64)
    for eps in (1e-5, 1e-6):
        for silu in (False, True):
            ref, bound = R.groupnorm_ref(d64(c["x"]), 32, d64(c["gamma"]), d64(c["beta"]), eps, silu)
            tag = "%s eps=%g silu=%d" % (name, eps, silu)
            y = torch.full((B, hw, Cc), float("nan"), device=DEV, dtype=torch.float16)
            ctx.groupnorm(xa, c1, c1, xb, c2, c2, B, hw, 32, gamma, beta, eps, silu, y, Cc, ws)
            torch.cuda.synchronize()
            assert report(tag + " one call", s, R.ratio(y.cpu(), ref, bound)) <= 1
            if not c2:
                y.fill_(float("nan"))
                ctx._chk(ctx.lib.upk_groupnorm_stats_nhwc_f16(ctx.h, xa.data_ptr(), c1, c1, None, 0, 0, B, hw, 32,
                                                              ws.data_ptr(), ctx._s()))
                ctx._chk(ctx.lib.upk_groupnorm_apply_nhwc_f16(ctx.h, xa.data_ptr(), c1, c1, None, 0, 0, B, hw, 32,
                                                              gamma.data_ptr(), beta.data_ptr(), eps, int(silu),
                                                              y.data_ptr(), Cc, ws.data_ptr(), 1, 0, 0, None, 0, 0, ctx._s()))
                torch.cuda.synchronize()
                assert report(tag + " stats+apply", s, R.ratio(y.cpu(), ref, bound)) <= 1
            y.fill_(float("nan"))
            ctx._chk(ctx.lib.upk_groupnorm_apply_nhwc_f16(
                ctx.h, xa.data_ptr(), c1, c1, xb.data_ptr() if c2 else None, c2, c2, B, hw, 32, gamma.data_ptr(),
                beta.data_ptr(), eps, int(silu), y.data_ptr(), Cc, pa.data_ptr(), 2, nblk, c1,
                pb.data_ptr() if c2 else None, nblk if c2 else 0, c2, ctx._s()))
            torch.cuda.synchronize()
            assert report(tag + " partials", s, R.ratio(y.cpu(), ref, bound)) <= 1


@pytest.mark.parametrize("s", R.SCALES)
def test_layernorm_and_folded_layernorm_gemm_against_fp64(ctx, s):
    d64 = lambda t: t.to(F64)
    for rows, d in R.LN_ROWS:
        c = R.ln_case(rows, d, s)
        y = torch.full((rows, d), float("nan"), device=DEV, dtype=torch.float16)
        ctx.layernorm(c["x"].to(DEV), d, rows, d, c["gamma"].to(DEV), c["beta"].to(DEV), 1e-5, y, d)
        torch.cuda.synchronize()
        ref, bound = R.layernorm_ref(d64(c["x"]), d64(c["gamma"]), d64(c["beta"]), 1e-5)
        assert report("layernorm %dx%d" % (rows, d), s, R.ratio(y.cpu(), ref, bound)) <= 1
    for name in R.LNGEMM_CASES:
        o = R.lngemm_case(name, s)
        M, d, N, geglu = o["M"], o["d"], o["N"], o["act"] == "geglu"
        n_out = N // 2 if geglu else N
        rm = geglu_row_map(n_out).to(DEV) if geglu else None
        wp, n_pad = ctx.pack_weight(o["wf"].to(DEV).contiguous(), row_map=rm)
        bf, u = o["bf"].to(DEV), o["u"].to(DEV)
        if geglu:
            bf, u = bf[rm.long()], u[rm.long()]
        bp = torch.zeros(n_pad, device=DEV); bp[:N] = bf
        up = torch.zeros(n_pad, device=DEV); up[:N] = u
        x = o["x"].to(DEV)
        y = torch.full((M, n_out), float("nan"), device=DEV, dtype=torch.float16)
        dsc = L.ConvDesc()
        dsc.x1 = x.data_ptr(); dsc.c1 = d; dsc.ld1 = d; dsc.batch = 1; dsc.in_h = M; dsc.in_w = 1
        dsc.ksize = 1; dsc.stride = 1; dsc.w_packed = wp.data_ptr(); dsc.n_out = n_out; dsc.n_pad = n_pad
        dsc.bias = bp.data_ptr(); dsc.y = y.data_ptr(); dsc.ldy = n_out; dsc.flags = L.F_GEGLU if geglu else 0
        dsc.ln_colsum = up.data_ptr(); dsc.ln_eps = o["eps"]; dsc.ln_dim = d
        ctx.conv(dsc)
        torch.cuda.synchronize()
        ref, bound = R.lngemm_case_ref(o)
        assert float(ref.abs().max()) < 6e4
        assert report(name, s, R.ratio(y.cpu(), ref, bound)) <= 1


@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_against_fp64(ctx, name, s):
    o = R.attn_case(name, s)
    B, heads, d, nq, nkv = o["B"], o["heads"], o["d"], o["nq"], o["nkv"]
    q, k = o["q"].to(DEV), o["k"].to(DEV)
    vt_ld = (nkv + 31) // 32 * 32
    vt = torch.zeros(B, heads, d, vt_ld, device=DEV, dtype=torch.float16)
    vt[..., :nkv] = o["v"].to(DEV).view(B, nkv, heads, d).permute(0, 2, 3, 1)
    out = torch.full((B, nq, heads * d), float("nan"), device=DEV, dtype=torch.float16)
    a = (q, heads * d, nq * heads * d, k, heads * d, nkv * heads * d, vt, vt_ld, out, heads * d, nq * heads * d, B, heads)
    if o["causal"]:
        ctx.attention_causal(*a, nq, d, o["scale"])
    else:
        ctx.attention(*a, nq, nkv, d, o["scale"])
    torch.cuda.synchronize()
    ref, bound = R.attn_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    got = out.cpu().view(B, nq, heads, d).transpose(1, 2)
    assert report(name, s, R.ratio(got, ref, bound)) <= 1


def _dev(o, *names):
    return [o[n].to(DEV) for n in names]


def _vec(*parts):
    v = torch.cat(parts)
    return torch.cat([v, v.new_zeros(-v.numel() % 256)]).contiguous()


@pytest.mark.parametrize("s", R.SCALES)
def test_attention_with_query_projection_inside_against_fp64(ctx, s):
    from upgpt_amd.packing import qproj_pack
    o = R.qproj_case(s)
    B, Cc, heads, dh, nq, nkv = o["B"], o["C"], o["heads"], o["dh"], o["nq"], o["nkv"]
    dp = R.DP
    x, = _dev(o, "x")
    k = torch.zeros(B, nkv, heads, dp, device=DEV, dtype=torch.float16)
    k[..., :dh] = o["k"].to(DEV)
    vt_ld = (nkv + 31) // 32 * 32
    vt = torch.zeros(B, heads, dp, vt_ld, device=DEV, dtype=torch.float16)
    vt[:, :, :dh, :nkv] = o["v"].to(DEV).permute(0, 2, 3, 1)
    wq, wu, wb = qproj_pack(o["w"].to(DEV), o["gamma"].to(DEV), o["beta"].to(DEV), heads, dh, dp, Cc, DEV)
    out = torch.full((B, nq, heads * dp), float("nan"), device=DEV, dtype=torch.float16)
    ctx._chk(ctx.lib.upk_attention_qproj_f16(ctx.h, x.data_ptr(), Cc, nq * Cc, Cc, Cc, o["eps"], wq.data_ptr(), wu.data_ptr(),
                                             wb.data_ptr(), k.data_ptr(), heads * dp, nkv * heads * dp, vt.data_ptr(),
                                             vt_ld, out.data_ptr(), heads * dp, nq * heads * dp, B, heads, nq, nkv, dp,
                                             o["scale"], ctx._s()))
    torch.cuda.synchronize()
    ref, bound = R.qproj_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    got = out.cpu().view(B, nq, heads, dp)
    assert not got[..., dh:].any()
    assert report("attention qproj", s, R.ratio(got[..., :dh].transpose(1, 2), ref, bound)) <= 1


def launch_head_block(ctx, o, rows=16):
    """One upk_head_block_f16 launch on head_case's operands at `rows` rows per workgroup; (t0, q | k, v) on the CPU, the
    padded head columns taken out."""
    B, hw, c = o["B"], o["hw"], o["c"]
    heads, dh, dp = R.HEADS, R.DH, R.DP
    M, hd, inner = B * hw, heads * dp, heads * dh
    x, wi, bi, gamma, beta, wqkv = _dev(o, "x", "wi", "bi", "gamma", "beta", "wqkv")
    cols = head_cols(heads, dh, dp).to(DEV)
    rows3 = torch.cat([torch.where(cols >= 0, cols + i * inner, cols) for i in range(3)]).to(torch.int32)
    real3 = rows3 >= 0
    wf = (wqkv * gamma[None, :]).half().float()
    w1p, n1 = ctx.pack_weight(wi.contiguous())
    w2p, n2 = ctx.pack_weight((wqkv * gamma[None, :]).contiguous(), row_map=rows3)
    assert n1 == c and n2 == 3 * hd
    u2 = torch.zeros(3 * hd, device=DEV); u2[real3] = wf.sum(dim=1)
    b2 = torch.zeros(3 * hd, device=DEV); b2[real3] = wqkv @ beta
    vec = _vec(bi, u2, b2)
    vt_ld = (hw + 31) // 32 * 32
    t0o = torch.full((M, c), float("nan"), device=DEV, dtype=torch.float16)
    qk = torch.full((M, 2 * hd), float("nan"), device=DEV, dtype=torch.float16)
    vt = torch.zeros(B, heads, dp, vt_ld, device=DEV, dtype=torch.float16)
    d = L.HblockDesc()
    d.x, d.ldx, d.m, d.c, d.heads, d.d = x.data_ptr(), c, M, c, heads, dp
    d.w_in, d.w_qkv, d.vec, d.ln_eps, d.ln_dim = w1p.data_ptr(), w2p.data_ptr(), vec.data_ptr(), o["eps"], c
    d.t0, d.ld_t0, d.qk, d.ld_qk, d.vt, d.vt_ld = t0o.data_ptr(), c, qk.data_ptr(), 2 * hd, vt.data_ptr(), vt_ld
    d.hw, d.rows_per_wg = hw, rows
    assert ctx.lib.upk_head_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_head_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    real = (cols >= 0).cpu()
    got_qk = qk.cpu().view(M, 2, hd)[:, :, real].reshape(M, 2 * inner)
    got_v = vt.cpu()[..., :hw].permute(0, 3, 1, 2).reshape(M, hd)[:, real]
    return t0o.cpu(), got_qk, got_v


@pytest.mark.parametrize("s", R.SCALES)
def test_head_block_against_fp64(ctx, s):
    o = R.head_case(s)
    inner = R.HEADS * R.DH
    t0o, got_qk, got_v = launch_head_block(ctx, o)
    (t0, dt0), (qkv, dqkv) = R.head_case_ref(o)
    assert float(t0.abs().max()) < 6e4 and float(qkv.abs().max()) < 6e4
    assert report("head block t0", s, R.ratio(t0o, t0, dt0)) <= 1
    assert report("head block q | k", s, R.ratio(got_qk, qkv[:, :2 * inner], dqkv[:, :2 * inner])) <= 1
    assert report("head block v", s, R.ratio(got_v, qkv[:, 2 * inner:], dqkv[:, 2 * inner:])) <= 1


def launch_cross_block(ctx, o, rows=16):
    """One upk_cross_block_f16 launch on cross_case's operands at `rows` rows per workgroup; y on the CPU."""
    B, hw, c, nkv = o["B"], o["hw"], o["c"], o["nkv"]
    heads, dh, dp = R.HEADS, R.DH, R.DP
    M, hd, inner = B * hw, heads * dp, heads * dh
    t0, wo1, bo1, gamma, beta, wq, wo2, bo2 = _dev(o, "t0", "wo1", "bo1", "gamma", "beta", "wq", "wo2", "bo2")
    cols = head_cols(heads, dh, dp).to(DEV)
    real = cols >= 0

    def padded(x):
        out = torch.zeros(*x.shape[:-1], hd, device=DEV, dtype=torch.float16)
        out[..., real] = x.to(DEV)
        return out

    a1 = padded(o["a1"])
    kc = padded(o["k"]).reshape(B * nkv, hd).contiguous()
    vt_ld = 96
    vt = torch.zeros(B, heads, dp, vt_ld, device=DEV, dtype=torch.float16)
    vt[:, :, :dh, :nkv] = o["v"].to(DEV).reshape(B, nkv, heads, dh).permute(0, 2, 3, 1)
    wqf = (wq * gamma[None, :]).half().float()
    w1p, n1 = ctx.pack_weight(wo1.contiguous(), col_map=cols)
    w3p, n3 = ctx.pack_weight(wo2.contiguous(), col_map=cols)
    wqp, nq = ctx.pack_weight((wq * gamma[None, :]).contiguous(), row_map=cols)
    assert n1 == c and n3 == c and nq == hd
    uq = torch.zeros(hd, device=DEV); uq[real] = wqf.sum(dim=1)
    bq = torch.zeros(hd, device=DEV); bq[real] = wq @ beta
    vec = _vec(bo1, uq, bq, bo2)
    y = torch.full((M, c), float("nan"), device=DEV, dtype=torch.float16)
    d = L.XblockDesc()
    d.a1, d.lda, d.m, d.c, d.heads, d.d = a1.data_ptr(), hd, M, c, heads, dp
    d.t0, d.ld_t0 = t0.data_ptr(), c
    d.w_out1, d.w_q, d.w_out2, d.vec = w1p.data_ptr(), wqp.data_ptr(), w3p.data_ptr(), vec.data_ptr()
    d.ln_eps, d.ln_dim = o["eps"], c
    d.k_ctx, d.ldk, d.n_kv = kc.data_ptr(), hd, nkv
    d.vt_ctx, d.vt_ld, d.scale = vt.data_ptr(), vt_ld, o["scale"]
    d.y, d.ldy, d.hw, d.rows_per_wg = y.data_ptr(), c, hw, rows
    assert ctx.lib.upk_cross_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_cross_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("s", R.SCALES)
def test_cross_block_against_fp64(ctx, s):
    o = R.cross_case(s)
    y = launch_cross_block(ctx, o)
    ref, bound = R.cross_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    assert report("cross block", s, R.ratio(y, ref, bound)) <= 1


def launch_mlp_tail(ctx, o, rows_per_wg=None):
    """One upk_geglu_mlp_f16 launch on mlp_case's operands (rows_per_wg: the descriptor's value, default o["rows"]);
    (y, partials [B, nblk, 2, n_pad] or None) on the CPU."""
    M, rows, hw, c, inner = o["M"], o["rows"], o["hw"], o["c"], o["inner"]
    x, res, gamma, beta, w1, b1, w2h, w2x, b2 = _dev(o, "x", "res", "gamma", "beta", "w1", "b1", "w2h", "w2x", "b2")
    rm = geglu_row_map(inner).to(DEV)
    w1p, n1 = ctx.pack_weight((w1 * gamma[None, :]).contiguous(), row_map=rm)
    b1p = (b1 + w1 @ beta)[rm.long()].contiguous()
    u1p = (w1 * gamma[None, :]).half().float().sum(dim=1)[rm.long()].contiguous()
    w2a, n_pad = ctx.pack_weight(w2h.contiguous())
    w2b, _ = ctx.pack_weight(w2x.contiguous())
    w2p = torch.cat([w2a.reshape(-1), w2b.reshape(-1)]).contiguous()
    b2p = torch.zeros(n_pad, device=DEV); b2p[:c] = b2
    y = torch.full((M, c), float("nan"), device=DEV, dtype=torch.float16)
    d = L.MlpDesc()
    d.x, d.ldx, d.m, d.c, d.inner = x.data_ptr(), c, M, c, inner
    d.w1, d.b1, d.u1, d.ln_eps, d.ln_dim = w1p.data_ptr(), b1p.data_ptr(), u1p.data_ptr(), o["eps"], c
    d.w2, d.b2, d.n_out, d.n_pad = w2p.data_ptr(), b2p.data_ptr(), c, n_pad
    d.residual, d.ld_res, d.y, d.ldy = res.data_ptr(), c, y.data_ptr(), c
    d.rows_per_wg, d.hw = rows if rows_per_wg is None else rows_per_wg, hw
    if hw:
        B = M // hw
        sws = torch.full((ctx.gn_stats_floats(B, n_pad),), float("nan"), device=DEV)
        d.gn_stats_ws = sws.data_ptr()
    assert ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_geglu_mlp_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    if not hw:
        return y.cpu(), None
    return y.cpu(), sws[: B * (hw // rows) * 2 * n_pad].reshape(B, hw // rows, 2, n_pad).cpu()


def check_mlp_tail(o, y, part, what, s):
    """y against mlp_case_ref, and the GroupNorm partials against the fp64 sums of y."""
    M, rows, hw, c = o["M"], o["rows"], o["hw"], o["c"]
    ref, bound = R.mlp_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    assert report(what, s, R.ratio(y, ref, bound)) <= 1
    if hw:
        # the GroupNorm partials it leaves: per (row block, channel) fp32 sums of its OWN fp16 output, n = rows terms
        # each, so off from the fp64 sums by at most n e32 sum|y| (n e32 sum y^2, plus e32 per square)
        B, nblk = M // hw, hw // rows
        part = part.to(F64)
        yb = y.to(F64).reshape(B, nblk, rows, c)
        r1 = R.ratio(part[:, :, 0, :c], yb.sum(2), rows * R.E32H * yb.abs().sum(2))
        r2 = R.ratio(part[:, :, 1, :c], (yb * yb).sum(2), (rows + 1) * R.E32H * (yb * yb).sum(2))
        assert report(what + " GroupNorm partials", s, max(r1, r2)) <= 1


@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("name", list(R.MLP_CASES))
def test_mlp_tail_against_fp64(ctx, name, s):
    o = R.mlp_case(name, s)
    check_mlp_tail(o, *launch_mlp_tail(ctx, o), "mlp tail %s" % name, s)


# ---------------------------------------------------------------------------------------------------------------------
# C. the edge of the range
def _edge_checks(got, ref, bound, what):
    got = got.to(F64)
    assert not torch.isnan(got).any(), what
    inside = ref.abs() <= 6e4
    r = ((got - ref).abs() / bound)[inside]
    assert torch.isfinite(got[inside]).all() and float(r.max()) <= 1, (what, float(r.max()))
    over = ref.abs() > 65520
    assert over.any() and inside.any()
    g, sgn = got[over], torch.sign(ref[over])
    assert (((g.abs() == float("inf")) | (g.abs() == 65504.0)) & (torch.sign(g) == sgn)).all(), what
    return float(r.max())


def test_edge_of_the_range_conv_and_gemm(ctx):
    o = R.conv_case("edge_conv", R.EDGE_SCALE, spec=R.EDGE_CONV)
    ref, bound = R.conv_case_ref(o)
    unsplit = run_conv(ctx, o, -1, 1)
    report("edge conv unsplit", R.EDGE_SCALE, _edge_checks(unsplit, ref, bound, "conv"))
    # split-K 2: the partials saturate at +-65504 (igemm_common.h slab_store); no NaN, and the elements whose partials
    # stayed in range still meet the split-K bound; the unsplit launch above is unaffected
    split = run_conv(ctx, o, -1, 2).to(F64)
    assert not torch.isnan(split).any()
    A = R.im2col(o["x1"].to(F64), 1)
    W = R.wmat(R.q16(o["w"].to(F64)))
    h = A.shape[-1] // 2
    parts_ok = ((A[..., :h] @ W[:, :h].t()).abs() < 65504) & ((A[..., h:] @ W[:, h:].t()).abs() < 65504) & (ref.abs() <= 6e4)
    assert (~parts_ok & (ref.abs() <= 6e4)).any()  # some partials do saturate where the sum is in range
    ref2, bound2 = R.conv_case_ref(o, splitk=2)
    r = ((split - ref2).abs() / bound2)[parts_ok]
    assert parts_ok.any() and float(r.max()) <= 1, float(r.max())
    report("edge conv split-K 2 (in-range partials)", R.EDGE_SCALE, float(r.max()))
    g = R.gemm_case("edge_gemm", R.EDGE_SCALE, shape=R.EDGE_GEMM, wgain=4.0)
    ref, bound = R.gemm_case_ref(g, with_res=False)
    report("edge gemm unsplit", R.EDGE_SCALE, _edge_checks(run_gemm(ctx, g, 1, with_res=False), ref, bound, "gemm"))


# ---------------------------------------------------------------------------------------------------------------------
# D. one model-level probe
def test_tiny_unet_with_residual_streams_of_1e3(ctx):
    """The tiny UNet (B = 2, 32x24, t = [981, 401]) on recipe weights whose residual-producing convs and proj_out carry a
    gain of 128: the fp64 oracle's taps report max |h| = 2.4e3.  Reference: the live oracle in fp64.  Tolerance from the
    reference side only: the same oracle with every layer output rounded to fp16 is off by a relative MSE of
    E_seam = 5.05e-6 (computed on the CPU, tests/test_dynamic_range_host.py recomputes it); the HIP path has more fp16
    seams than layer boundaries (t0, t1, h, q/k/v), hence the margin of 4.  A second gain of 512 (max |h| 9.8e3, oracle
    E_seam 4.70e-6) is run and reported only.  Measured on an MI355X: 5.01e-6 = 0.99 x E_seam at gain 128; finite and
    5.50e-6 at gain 512."""
    import upgpt_amd
    from upgpt_amd import synth
    inp, t = R.probe_inputs()
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    out = {}
    for g in (R.PROBE_GAIN, R.PROBE_GAIN_REPORT):
        model = upgpt_amd.build_model("tiny")
        sd = synth.fill_module_(model)
        model.load_state_dict(R.stress_state(sd, g), strict=False)
        model = model.cuda()
        eps = model.apply_model(inp["x_T"].cuda(), t.cuda(), cond).float().cpu()
        ref, hmax = R.probe_oracle(sd, g)
        finite = bool(torch.isfinite(eps).all())
        e = R.rel_mse(eps, ref) if finite else float("nan")
        out[g] = (finite, e)
        print("range tiny UNet gain %-5g max|h| %.3g finite %s rel MSE %.3e = %.2f x E_seam" % (g, hmax, finite, e, e / R.E_SEAM))
        del model
    finite, e = out[R.PROBE_GAIN]
    assert finite and e <= 4 * R.E_SEAM, (finite, e, R.E_SEAM)
