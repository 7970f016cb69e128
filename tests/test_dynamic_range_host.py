"""The fp64 references and the derived bound of tests/range_ref.py have teeth (CPU only): each reference agrees with
torch's own fp64 op, a faithful emulation of the kernels' arithmetic (fp16 operands, fp32 accumulation, the same fp16
seams) passes the bound at every scale, three emulated defects do not, and the generators keep the input conditions
the GPU tests rely on."""

import pytest
import torch
import torch.nn.functional as F

import range_ref as R

F64 = torch.float64
D = lambda t: t.to(F64)


def _conv_operands(o):
    x = D(o["x1"]) if o["x2"] is None else torch.cat([D(o["x1"]), D(o["x2"])], 1)
    return x, R.q16(D(o["w"]))


def _torch_conv(o):
    """F.conv2d in fp64 on the same operands -> [B, Ho, Wo, N]."""
    x, w = _conv_operands(o)
    if o["ups"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if o["asym"]:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, D(o["bias"]), stride=2)
    else:
        y = F.conv2d(x, w, D(o["bias"]), stride=o["stride"], padding=o["ks"] // 2)
    if o["seg"]:
        xs = D(o["x3"]) if o["x4"] is None else torch.cat([D(o["x3"]), D(o["x4"])], 1)
        y = y + F.conv2d(xs, R.q16(D(o["w2"])))
    y = y.permute(0, 2, 3, 1)
    if o["rowvec"]:
        y = y + D(o["rv"][o["rv_step"]]).view(o["B"], 1, 1, -1)
    if o["res"]:
        y = y + D(o["resid"])
    return y


@pytest.mark.parametrize("name", [n for n in R.CONV_CASES if "phased" not in n])
def test_conv_reference_is_conv2d(name):
    o = R.conv_case(name, 2 ** 6)
    ref, bound = R.conv_case_ref(o)
    want = _torch_conv(o)
    assert ref.shape == want.shape == (o["B"], o["Ho"], o["Wo"], o["cout"])
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-9 * float(want.abs().max()))
    assert (bound > 0).all() and torch.isfinite(bound).all()


def test_phased_upsample_reference_is_the_direct_form_up_to_the_weight_rounding():
    o = R.conv_case("ups2x_96_64_phased", 1)
    ref, bound = R.conv_case_ref(o)
    direct = _torch_conv(dict(o, phased=False))
    # the phase weights are sums of up to four taps rounded to fp16 once more: 2^-11 of sum |x| |w| at the most
    x, w = _conv_operands(o)
    slack = 2.0 ** -11 * F.conv2d(F.interpolate(x.abs(), scale_factor=2, mode="nearest"), w.abs(), padding=1).permute(0, 2, 3, 1)
    assert ((ref - direct).abs() <= slack).all()
    assert float((ref - direct).abs().max()) > 0  # (it is the other operand set, not the same computation)


def test_norm_and_attention_references_are_torch_fp64():
    for name in R.GN_CASES:
        c = R.gn_case(name, 2 ** 10)
        for eps in (1e-5, 1e-6):
            ref, _ = R.groupnorm_ref(D(c["x"]), 32, D(c["gamma"]), D(c["beta"]), eps, False)
            want = F.group_norm(D(c["x"]).permute(0, 2, 1), 32, D(c["gamma"]), D(c["beta"]), eps).permute(0, 2, 1)
            assert torch.allclose(ref, want, rtol=1e-9, atol=1e-9)
            ref, _ = R.groupnorm_ref(D(c["x"]), 32, D(c["gamma"]), D(c["beta"]), eps, True)
            assert torch.allclose(ref, F.silu(want), rtol=1e-9, atol=1e-9)
    for rows, d in R.LN_ROWS:
        c = R.ln_case(rows, d, 2 ** 13)
        ref, _ = R.layernorm_ref(D(c["x"]), D(c["gamma"]), D(c["beta"]), 1e-5)
        assert torch.allclose(ref, F.layer_norm(D(c["x"]), (d,), D(c["gamma"]), D(c["beta"]), 1e-5), rtol=1e-9, atol=1e-9)
    for name in R.ATTN_CASES:
        o = R.attn_case(name, 2 ** 6)
        ref, _ = R.attn_case_ref(o)
        sp = lambda t, n: D(t).view(o["B"], n, o["heads"], o["d"]).transpose(1, 2)
        want = F.scaled_dot_product_attention(sp(o["q"], o["nq"]), sp(o["k"], o["nkv"]), sp(o["v"], o["nkv"]),
                                              is_causal=o["causal"], scale=o["scale"])
        assert torch.allclose(ref, want, rtol=1e-9, atol=1e-9)
    o = R.lngemm_case("ln96_224_256", 2 ** 10)
    ref, _ = R.lngemm_case_ref(o)
    # the fold is algebra: LayerNorm with gamma = 1, beta = 0, then the packed weight and the folded bias
    want = F.layer_norm(D(o["x"]), (o["d"],), None, None, o["eps"]) @ R.q16(D(o["wf"])).t() + D(o["bf"])
    # (u is the fp32 column sum: it differs from the fp64 one by its own rounding)
    assert torch.allclose(ref, want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# emulations: fp16 operands, fp32 arithmetic in the kernels' order, fp16 seams
def _silu32(v):
    return v * (1.0 / (1.0 + torch.exp(-v)))


def _silu_wrong_way_round(v):
    e = torch.exp(v)
    return v * e / (1.0 + e)


def emulate_linear(A, W, bias, rowvec=None, res=None, act=None, out="f16", splitk=1, acc16=False, drop_last_chunk=False,
                   silu=_silu32):
    A, W = A.float(), W.float()
    K = A.shape[-1]
    if drop_last_chunk:
        K -= 32
    if acc16:
        acc = torch.zeros(A.shape[:-1] + (W.shape[0],), dtype=torch.float16)
        for k0 in range(0, K, 32):
            acc = (acc.float() + A[..., k0:k0 + 32] @ W[:, k0:k0 + 32].t()).half()
        acc = acc.float()
    elif splitk > 1:
        chunks = K // 32
        per = -(-chunks // splitk)
        acc = torch.zeros(A.shape[:-1] + (W.shape[0],))
        for z in range(splitk):
            k0, k1 = z * per * 32, min(K, (z + 1) * per * 32)
            if k0 < k1:
                acc = acc + (A[..., k0:k1] @ W[:, k0:k1].t()).clamp(-65504, 65504).half().float()
    else:
        acc = A[..., :K] @ W[:, :K].t()
    v = acc + bias.float()
    if act == "geglu":
        n = W.shape[0] // 2
        g = v[..., n:]
        v = v[..., :n] * (0.5 * g * (1 + torch.erf(g * 0.7071067811865476)))
    if rowvec is not None:
        v = v + rowvec.float()
    if act == "silu":
        v = silu(v)
    elif act == "quickgelu":
        v = v * (1.0 / (1.0 + torch.exp(-1.702 * v)))
    if res is not None:
        v = v + res.float()
    return v.half() if out == "f16" else v


def _conv_A_W(o):
    x, w = _conv_operands(o)
    A = R.im2col(x, o["ks"], o["stride"], (0, 1, 0, 1) if o["asym"] else None, o["ups"])
    W = R.wmat(w)
    if o["seg"]:
        xs = D(o["x3"]) if o["x4"] is None else torch.cat([D(o["x3"]), D(o["x4"])], 1)
        A = torch.cat([A, xs.permute(0, 2, 3, 1)], -1)
        W = torch.cat([W, R.wmat(R.q16(D(o["w2"])))], -1)
    return A, W


def _emulate_conv(o, **kw):
    if o["phased"]:
        x, _ = _conv_operands(o)
        out = torch.zeros(o["B"], o["Ho"], o["Wo"], o["cout"], dtype=torch.float16)
        for (py, px), wp in R.phase_weights(o["w"]).items():
            A = R.im2col(x, 2, pad=(1 - py, py, 1 - px, px))
            out[:, py::2, px::2] = emulate_linear(A, R.wmat(R.q16(D(wp))), o["bias"], act=o["act"], **kw)
        return out
    A, W = _conv_A_W(o)
    rv = o["rv"][o["rv_step"]].view(o["B"], 1, 1, -1) if o["rowvec"] else None
    return emulate_linear(A, W, o["bias"], rowvec=rv, res=o["resid"] if o["res"] else None, act=o["act"],
                          out="f16" if o["out"] == "f16" else "f32", **kw)


@pytest.mark.parametrize("s", R.SCALES)
def test_faithful_linear_emulation_passes(s):
    for name in R.CONV_CASES:
        for act in (None, "silu", "quickgelu"):
            if act and name != "c3x3_64_224":
                continue
            o = R.conv_case(name, s, act=act)
            for sk in (1, 2, 3):
                ref, bound = R.conv_case_ref(o, splitk=sk)
                assert float(ref.abs().max()) < 6e4
                r = R.ratio(_emulate_conv(o, splitk=sk), ref, bound)
                assert r <= 1, (name, act, s, sk, r)
    for name in R.GEMM_CASES:
        o = R.gemm_case(name, s)
        ref, bound = R.gemm_case_ref(o)
        assert float(ref.abs().max()) < 6e4
        r = R.ratio(emulate_linear(o["a"], R.q16(D(o["w"])), o["bias"], res=o["resid"]), ref, bound)
        assert r <= 1, (name, s, r)
    o = R.gemm_case("geglu96_224", s, act="geglu", shape=(96, 224, 2 * 896), value_gain=R.GEGLU_VALUE_GAIN / s)
    ref, bound = R.gemm_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    r = R.ratio(emulate_linear(o["a"], R.q16(D(o["w"])), o["bias"], act="geglu"), ref, bound)
    assert r <= 1, ("geglu", s, r)
    assert float((D(o["a"]) @ R.q16(D(o["w"])).t())[:, 896:].abs().max()) > 3 * s  # the gate spans the full scale


def test_the_three_defects_exceed_the_bound():
    worst = {"acc16": 0.0, "drop": 0.0, "silu": 0.0}
    for s in R.SCALES:
        o = R.conv_case("c3x3_64_224", s)
        ref, bound = R.conv_case_ref(o)
        worst["acc16"] = max(worst["acc16"], R.ratio(_emulate_conv(o, acc16=True), ref, bound))
        worst["drop"] = max(worst["drop"], R.ratio(_emulate_conv(o, drop_last_chunk=True), ref, bound))
        o = R.conv_case("c3x3_64_224", s, act="silu")
        ref, bound = R.conv_case_ref(o)
        assert R.ratio(_emulate_conv(o), ref, bound) <= 1
        worst["silu"] = max(worst["silu"], R.ratio(_emulate_conv(o, silu=_silu_wrong_way_round), ref, bound))
    assert all(v > 1 for v in worst.values()), worst
    # a dropped chunk and fp16 accumulation are caught at EVERY scale, not only at one
    for s in R.SCALES:
        o = R.conv_case("c3x3_64_224", s)
        ref, bound = R.conv_case_ref(o)
        assert R.ratio(_emulate_conv(o, drop_last_chunk=True), ref, bound) > 1
        assert R.ratio(_emulate_conv(o, acc16=True), ref, bound) > 1


def _emulate_groupnorm(x, groups, gamma, beta, eps, silu):
    B, hw, C = x.shape
    cpg = C // groups
    xf = x.float().view(B, hw, groups, cpg)
    n = hw * cpg
    s1 = xf.sum((1, 3), dtype=torch.float32).double()
    s2 = (xf * xf).sum((1, 3), dtype=torch.float32).double()
    mean = s1 / n
    rstd = (1.0 / torch.sqrt((s2 / n - mean * mean).clamp(min=0) + eps)).float().view(B, 1, groups, 1)
    sc = rstd * gamma.float().view(1, 1, groups, cpg)
    y = xf * sc + (beta.float().view(1, 1, groups, cpg) - mean.float().view(B, 1, groups, 1) * sc)
    if silu:
        y = _silu32(y)
    return y.view(B, hw, C).half()


def _attn32(q, k, v, scale, causal=False, subtract_max=True):
    """fp32 attention on [B, h, n, d] with the weights rounded to fp16 in front of the second product."""
    cs = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    sc = q @ k.transpose(-1, -2)
    if causal:
        sc = sc.masked_fill(torch.ones(q.shape[-2], k.shape[-2], dtype=torch.bool).triu(1), float("-inf"))
    m = sc.max(-1, keepdim=True).values if subtract_max else torch.zeros_like(sc[..., :1])
    p = torch.exp2(sc * cs + (-m * cs)).half().float()
    return ((p @ v) * (1.0 / p.sum(-1, keepdim=True))).half()


def _emulate_attention(o, **kw):
    sp = lambda t, n: t.float().view(o["B"], n, o["heads"], o["d"]).transpose(1, 2)
    return _attn32(sp(o["q"], o["nq"]), sp(o["k"], o["nkv"]), sp(o["v"], o["nkv"]), o["scale"], o["causal"], **kw)


def _lnlin32(x, w, gamma, beta, eps, extra_bias=None, stat_cols=None):
    """The folded-LayerNorm Linear in fp32: one-pass statistics, (acc - mean u) rstd + b.  (stat_cols, a defect: the
    statistics are taken over the first stat_cols columns only.)"""
    wf = (w * gamma[None, :]).half().float()
    b = w @ beta if extra_bias is None else w @ beta + extra_bias
    xs = x if stat_cols is None else x[:, :stat_cols]
    mean = xs.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((xs * xs).mean(-1, keepdim=True) - mean * mean).clamp(min=0) + eps)
    return (x @ wf.t() - mean * wf.sum(1)) * rstd + b


def emulate_head(o, stat_cols=None):
    t0 = (o["x"].float() @ o["wi"].half().float().t() + o["bi"]).half()
    return t0, _lnlin32(t0.float(), o["wqkv"], o["gamma"], o["beta"], o["eps"], stat_cols=stat_cols).half()


def emulate_cross(o, stale_t1=False):
    B, hw, nkv = o["B"], o["hw"], o["nkv"]
    t1 = o["a1"].float() @ o["wo1"].half().float().t() + o["bo1"] + o["t0"].float()
    t1 = t1.half().float()
    q = _lnlin32(t1, o["wq"], o["gamma"], o["beta"], o["eps"]).half().float()
    sp = lambda t, n: t.float().reshape(B, n, o["heads"], o["dh"]).transpose(1, 2)
    a2 = _attn32(sp(q, hw), sp(o["k"], nkv), sp(o["v"], nkv), o["scale"]).float().transpose(1, 2).reshape(B * hw, -1)
    # (stale_t1, a defect: the final residual reads t0 where it should read t1)
    return (a2 @ o["wo2"].half().float().t() + o["bo2"] + (o["t0"].float() if stale_t1 else t1)).half()


def emulate_mlp(o, drop_last_chunk=False, gelu=F.gelu, stale_slice=False):
    inner = o["inner"]
    pre = _lnlin32(o["x"].float(), o["w1"], o["gamma"], o["beta"], o["eps"], extra_bias=o["b1"])
    h = pre[:, :inner] * gelu(pre[:, inner:])
    h = h.half().float()
    if stale_slice:  # (a defect: hidden columns 128..255 are a stale copy of 0..127, the streaming form's slice hazard)
        h[:, 128:256] = h[:, :128]
    kx = o["c"] - 32 if drop_last_chunk else o["c"]  # (a defect: the last 32-wide K chunk of the GEMM over [h | x] dropped)
    return (h @ o["w2h"].half().float().t() + o["x"].float()[:, :kx] @ o["w2x"].half().float()[:, :kx].t() + o["b2"]
            + o["res"].float()).half()


def emulate_qproj(o):
    B, nq, heads, dh = o["B"], o["nq"], o["heads"], o["dh"]
    q = _lnlin32(o["x"].float().reshape(B * nq, -1), o["w"], o["gamma"], o["beta"], o["eps"]).half().float()
    return _attn32(q.reshape(B, nq, heads, dh).transpose(1, 2), o["k"].float().transpose(1, 2), o["v"].float().transpose(1, 2),
                   o["scale"])


@pytest.mark.parametrize("s", R.SCALES)
def test_faithful_chain_emulations_pass(s):
    o = R.head_case(s)
    (t0, dt0), (qkv, dqkv) = R.head_case_ref(o)
    e_t0, e_qkv = emulate_head(o)
    assert float(t0.abs().max()) < 6e4
    assert R.ratio(e_t0, t0, dt0) <= 1 and R.ratio(e_qkv, qkv, dqkv) <= 1, s
    o = R.cross_case(s)
    ref, bound = R.cross_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    assert R.ratio(emulate_cross(o), ref, bound) <= 1, s
    for name in R.MLP_CASES:
        o = R.mlp_case(name, s)
        ref, bound = R.mlp_case_ref(o)
        assert float(ref.abs().max()) < 6e4
        assert R.ratio(emulate_mlp(o), ref, bound) <= 1, (name, s)
    o = R.qproj_case(s)
    ref, bound = R.qproj_case_ref(o)
    assert float(ref.abs().max()) < 6e4
    assert R.ratio(emulate_qproj(o), ref, bound) <= 1, s


def test_chain_defects_exceed_the_bound():
    """The chained bounds are worst-case sums and much wider than the single-stage ones; they still catch a dropped K
    chunk of the MLP tail's second GEMM, a cross block whose last residual reads t0 instead of t1, and a head block
    whose q | k | v are computed from an un-normalised t0, at every scale."""
    for s in R.SCALES:
        o = R.mlp_case("mlp128", s)
        ref, bound = R.mlp_case_ref(o)
        assert R.ratio(emulate_mlp(o, drop_last_chunk=True), ref, bound) > 1, s
        o = R.cross_case(s)
        ref, bound = R.cross_case_ref(o)
        assert R.ratio(emulate_cross(o, stale_t1=True), ref, bound) > 1, s
        o = R.head_case(s)
        _, (qkv, dqkv) = R.head_case_ref(o)
        t0, _ = emulate_head(o)
        wf = (o["wqkv"] * o["gamma"][None, :]).half().float()
        unnormalised = (t0.float() @ wf.t() + o["wqkv"] @ o["beta"]).half()
        assert R.ratio(unnormalised, qkv, dqkv) > 1, s


def test_attention_defects_exceed_the_bound():
    """exp without the running-maximum subtraction overflows to inf / inf once the logits pass ~88; a causal mask that is
    off by one key is wrong at every scale."""
    worst = 0.0
    for s in R.SCALES:
        o = R.attn_case("a64_48_87", s)
        ref, bound = R.attn_case_ref(o)
        worst = max(worst, R.ratio(_emulate_attention(o, subtract_max=False), ref, bound))
        c = R.attn_case("causal64_77", s)
        ref, bound = R.attn_case_ref(c)
        assert R.ratio(_emulate_attention(dict(c, causal=False)), ref, bound) > 1, s  # mask dropped
    assert worst > 1


@pytest.mark.parametrize("s", R.SCALES)
def test_faithful_norm_and_attention_emulations_pass(s):
    for name in R.GN_CASES:
        c = R.gn_case(name, s)
        for eps in (1e-5, 1e-6):
            for silu in (False, True):
                ref, bound = R.groupnorm_ref(D(c["x"]), 32, D(c["gamma"]), D(c["beta"]), eps, silu)
                r = R.ratio(_emulate_groupnorm(c["x"], 32, c["gamma"], c["beta"], eps, silu), ref, bound)
                assert r <= 1, (name, s, eps, silu, r)
    for rows, d in R.LN_ROWS:
        c = R.ln_case(rows, d, s)
        ref, bound = R.layernorm_ref(D(c["x"]), D(c["gamma"]), D(c["beta"]), 1e-5)
        got = F.layer_norm(c["x"].float(), (d,), c["gamma"], c["beta"], 1e-5).half()
        assert R.ratio(got, ref, bound) <= 1, (rows, d, s)
    for name in R.LNGEMM_CASES:
        o = R.lngemm_case(name, s)
        ref, bound = R.lngemm_case_ref(o)
        assert float(ref.abs().max()) < 6e4
        x = o["x"].float()
        W = o["wf"].half().float()
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0) + o["eps"])
        v = (x @ W.t() - mean * o["u"]) * rstd + o["bf"]
        if o["act"] == "geglu":
            n = o["N"] // 2
            v = v[:, :n] * F.gelu(v[:, n:])
        assert R.ratio(v.half(), ref, bound) <= 1, (name, s)
    for name in R.ATTN_CASES:
        o = R.attn_case(name, s)
        ref, bound = R.attn_case_ref(o)
        assert float(ref.abs().max()) < 6e4
        r = R.ratio(_emulate_attention(o), ref, bound)
        assert r <= 1, (name, s, r)


def test_generators_keep_the_input_conditions():
    """No fp16-subnormal (or zero, or non-finite) activation at any scale, and |mean| / std <= 4 per channel, group and row."""
    tiny = 2.0 ** -14
    for s in R.SCALES:
        xs = [R.conv_case(n, s)["x1"] for n in R.CONV_CASES] + [R.gemm_case(n, s)["a"] for n in R.GEMM_CASES]
        xs += [R.attn_case(n, s)[t] for n in R.ATTN_CASES for t in "qkv"]
        gn = [R.gn_case(n, s)["x"] for n in R.GN_CASES]
        ln = [R.ln_case(r, d, s)["x"] for r, d in R.LN_ROWS] + [R.lngemm_case(n, s)["x"] for n in R.LNGEMM_CASES]
        for x in xs + gn + ln:
            assert torch.isfinite(x).all() and float(x.abs().min()) >= max(tiny, 2.0 ** -10 * min(s, 64) / 64)
        assert max(float(x.abs().max()) for x in xs) > 2.5 * s  # the scale is really applied
        for x in gn:
            B, hw, C = x.shape
            xd = D(x)
            per_ch = xd.mean(1).abs() / xd.std(1)
            g = xd.view(B, hw, 32, C // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
            assert float(per_ch.max()) <= 4 and float((g.mean(-1).abs() / g.std(-1)).max()) <= 4
        for x in ln:
            xd = D(x)
            assert float((xd.mean(-1).abs() / xd.std(-1)).max()) <= 4
            if x.shape[0] >= 32:  # (a sample statistic over a handful of rows says nothing about the channel)
                assert float((xd.mean(0).abs() / xd.std(0)).max()) <= 4


def test_exclusion_caps_hold_on_the_reference():
    """Section A excludes elements whose base (scale 1) output is fp16-subnormal: at most 0.1 % of a case.  Section C
    needs a reference that is partly beyond 65504 and partly inside 6e4."""
    for name in R.CONV_CASES:
        ref, _ = R.conv_case_ref(R.conv_case(name, 1))
        assert float((ref.abs() < 2.0 ** -14).double().mean()) <= 1e-3, name
    for name in R.GEMM_CASES:
        ref, _ = R.gemm_case_ref(R.gemm_case(name, 1))
        assert float((ref.abs() < 2.0 ** -14).double().mean()) <= 1e-3, name
    o = R.conv_case("edge_conv", R.EDGE_SCALE, spec=R.EDGE_CONV)
    A, W = _conv_A_W(o)
    h = A.shape[-1] // 2
    sat = ((A[..., :h] @ W[:, :h].t()).abs() > 65504) | ((A[..., h:] @ W[:, h:].t()).abs() > 65504)
    assert (sat & (R.conv_case_ref(o)[0].abs() <= 6e4)).any()  # split-K 2 partials that saturate under an in-range sum
    for ref in edge_refs():
        over, inside = float((ref.abs() > 65520).double().mean()), float((ref.abs() <= 6e4).double().mean())
        assert over > 0.01 and inside > 0.5, (over, inside)


def edge_refs():
    o = R.conv_case("edge_conv", R.EDGE_SCALE, spec=R.EDGE_CONV)
    yield R.conv_case_ref(o)[0]
    o = R.gemm_case("edge_gemm", R.EDGE_SCALE, shape=R.EDGE_GEMM, wgain=4.0)
    yield R.gemm_case_ref(o, with_res=False)[0]


def test_model_probe_gain_and_seam_error():
    """The stress gains put the oracle's residual streams where the GPU probe wants them, and E_SEAM is what the fp64
    oracle loses when every layer output is stored as fp16 (measured: 5.05e-6 at max |h| 2.4e3, 4.70e-6 at 9.8e3)."""
    import upgpt_amd
    from upgpt_amd import synth
    sd = synth.fill_module_(upgpt_amd.build_model("tiny"))
    y, hmax = R.probe_oracle(sd, R.PROBE_GAIN)
    assert 1e3 <= hmax <= 4e3, hmax
    y16, _ = R.probe_oracle(sd, R.PROBE_GAIN, round_fn=lambda v: v.half().to(v.dtype))
    assert torch.isfinite(y16).all()
    e = R.rel_mse(y16, y)
    assert abs(e - R.E_SEAM) <= 0.02 * R.E_SEAM, e
    _, hmax2 = R.probe_oracle(sd, R.PROBE_GAIN_REPORT)
    assert 7e3 <= hmax2 <= 1.4e4, hmax2
