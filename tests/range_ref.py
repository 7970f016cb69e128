"""fp64 references with a derived, per-element error bound, for the dynamic-range tests.

Every reference takes the fp16-rounded operands the kernel gets, computes the operation in fp64 (on the CPU; the attention
references also on the device that holds the operands) and returns ``(ref, bound)``.  ``bound`` has the shape of ``ref`` and is the sum of the terms below; a kernel passes when
``|got - ref| <= bound`` at every element (``ratio()`` returns max |got - ref| / bound, NaN counted as infinite).
No term is fitted to a kernel: each follows from the number formats and the first-order error propagation.

Notation: u16(v) = one unit in the last place of fp16 at v (2^-24 below 2^-14, 2^(floor(log2 |v|) - 10) above),
e32 = 2^-24 (half an ulp of fp32, the rounding of one fp32 operation), E32 = 2^-23 (one ulp of fp32).

* Output rounding.  u16(ref): one ulp where the ideal is half of one (fp32 outputs: E32 |ref|).
* fp32 accumulation.  A dot product of K terms summed in fp32 in any order is off by at most K e32 sum|a||b|
  (Higham, Accuracy and Stability, eq. 3.5 to first order; fp16 x fp16 products are exact in fp32).  sum|a||b| is
  computed in fp64 from the absolute values of the same operands.
* Epilogue additions (bias, row vector, residual) in fp32: e32 of the partial result per addition, bounded by
  e32 (|acc| + |bias| + |rowvec| + |res|) each.
* fp16 seams.  A value v the kernel stores as fp16 and reads back is perturbed by u16(v); the perturbation is pushed
  through the absolute value of the linear map behind it (or |f'| for a nonlinear one).  The split-K slabs are such a
  seam: z partials p_1..p_z, sum |p_i| <= sum|a||b|, so the seam term is min(z u16(sum|a||b|), 2^-10 sum|a||b| + z 2^-24).
  The softmax weights of the attention kernels are another (they feed the second MFMA as fp16).
* Nonlinear stages.  f(v + dv) - f(v) ~ |f'(v)| dv, with dv the bound accumulated so far, plus the error of the
  instruction that evaluates f.  The guides give no accuracy for v_exp_f32, v_rcp_f32 and v_rsq_f32, so each is taken
  as one ulp of fp32 (E32, relative).  exp(x) evaluated as exp2(x log2 e) also carries the rounding of the product,
  |x| E32 relative.  The erf of the GELU is Abramowitz-Stegun 7.1.26, documented absolute error 1.5e-7.
    SiLU / QuickGELU  f = v sig(c v):  f' = sig + c v sig (1 - sig);
                      instruction error |v| sig (1 - sig) (|c v| E32 + 2 E32) + 3 E32 |f|
    GEGLU  f = a gelu(g):  |gelu(g)| da + |a| (|Phi(g) + g phi(g)| dg + |g| 0.75e-7 + 6 E32 |gelu(g)| ) + E32 |f|
                      (the kernel's folded form gelu = max(g, 0) - |g| q / 2 puts the erf error on q / 2)
    GroupNorm / LayerNorm  y = (x - mean) rstd gamma + beta: n-term fp32 sums perturb mean by n e32 mean|x| and the
                      variance by n e32 (2 mean(x^2)) (one-pass form E[x^2] - mean^2: both terms are of size mean(x^2));
                      d rstd = rstd dvar / (2 var) + E32 rstd; dy = |gamma| (rstd dmean + |x - mean| drstd) + 4 e32
                      (|x rstd gamma| + |mean rstd gamma| + |beta|) for the fp32 multiply-adds of the apply pass.
    softmax attention  out = sum_j p_j v_j / sum_j p_j,  p_j = exp(l_j - m):  logits are off by
                      dl = scale d e32 sum|q||k| + 4 E32 (|l_j| + |m|)  (accumulation; rounding of scale log2 e, of
                      m scale log2 e, and of the fused multiply-add; l_j and m both move, hence 2 dl), so
                      dp_j = p_j (exp(2 dl) - 1 + 2 E32) + max(2^-10 p_j, 2^-24)
                      (instruction error and the fp16 seam of p), and
                      dout = (sum_j dp_j |v_j| + |out| sum_j dp_j + n_kv e32 sum_j p_j |v_j|) / sum_j p_j + 3 E32 |out|.
  The folded-LayerNorm GEMM y = (acc - mean u) rstd + b applies the GroupNorm / LayerNorm statistics terms to the two
  accumulations acc = x W'^T and u = sum_k W'_k (W' = fp16(W gamma)).

The generators (``activations``) and the case tables are shared by the host and the GPU tests; ``attn_variant_rows`` is the
table of every compiled attention instantiation and ``attn_layout`` the two operand layouts they are run in; ``ROW_CHAIN``
is the table of every compiled row-chain instantiation and ``cross_probe`` / ``head_probe`` / ``mlp_probe`` the operands
that leave one stage of a chain inexact.
"""
import math

import torch

E32H = 2.0 ** -24  # rounding of one fp32 operation
E32 = 2.0 ** -23   # one ulp of fp32 (relative)
F16_MAX = 65504.0
SCALES = (1, 2 ** 6, 2 ** 10, 2 ** 13)
F64 = torch.float64


def u16(v):
    """One ulp of fp16 at v (fp64 tensor)."""
    a = v.abs().clamp(min=2.0 ** -14, max=F16_MAX)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def q16(v):
    """Round to fp16 and come back (fp64)."""
    return v.to(torch.float16).to(F64)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; NaN and inf count as infinite."""
    got = got.to(F64)
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())


def activations(shape, seed, s=1, mu=None, sigma=None, device="cpu"):
    """randn with |x| < 2^-10 replaced by +-2^-10, times s: fp16, no subnormal at any scale.  mu / sigma (broadcastable,
    |mu| / sigma <= 4 is the caller's business) shift and stretch before the scaling.  device: where the numbers are drawn
    (tensors of 10^8 elements take seconds on the CPU; a device generator draws other numbers from the same seed)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(*shape, generator=g, device=device)
    if sigma is not None:
        x = x * sigma.to(device)
    if mu is not None:
        x = x + mu.to(device)
    tiny = x.abs() < 2.0 ** -10
    x = torch.where(tiny, torch.where(x < 0, -(2.0 ** -10), 2.0 ** -10) * torch.ones_like(x), x)
    return (x.half() * float(s)).half()


def weights(shape, fan_in, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) / math.sqrt(fan_in)


def vector(n, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------
# conv / GEMM
def im2col(x, ks, stride=1, pad=None, ups=False):
    """x [B, C, H, W] -> A [B, Ho, Wo, ks*ks*C] (tap-major, then channel: the kernels' K order); pad = (top, bottom, left,
    right), default ks // 2 all round; ups: nearest 2x first."""
    if ups:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    pt, pb, pl, pr = pad if pad is not None else (ks // 2,) * 4
    B, C, H, W = x.shape
    xp = x.new_zeros(B, C, H + pt + pb, W + pl + pr)
    xp[:, :, pt:pt + H, pl:pl + W] = x
    Ho = (H + pt + pb - ks) // stride + 1
    Wo = (W + pl + pr - ks) // stride + 1
    cols = []
    for ky in range(ks):
        for kx in range(ks):
            cols.append(xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride])
    return torch.stack(cols, 1).reshape(B, ks * ks * C, Ho, Wo).permute(0, 2, 3, 1).contiguous()


def wmat(w):
    """[N, C, kh, kw] -> [N, kh*kw*C] in im2col's K order."""
    if w.dim() == 2:
        return w
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def phase_weights(w):
    """The four 2x2 phase weights of nearest-2x -> conv3x3 (fp32 sums of the taps, as the packing sees them)."""
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            wp = torch.zeros(w.shape[0], w.shape[1], 2, 2)
            for ky in range(3):
                for kx in range(3):
                    ty, tx = ((py + ky - 1) >> 1) - (py - 1), ((px + kx - 1) >> 1) - (px - 1)
                    wp[:, :, ty, tx] += w[:, :, ky, kx]
            out[(py, px)] = wp
    return out


def _sig(v):
    return torch.sigmoid(v)


def _act(v, dv, kind):
    """(f(v), bound) of SiLU / QuickGELU at v known to dv."""
    c = 1.0 if kind == "silu" else 1.702
    sg = _sig(c * v)
    f = v * sg
    d1 = (sg + c * v * sg * (1 - sg)).abs()
    inst = v.abs() * sg * (1 - sg) * ((c * v).abs() * E32 + 2 * E32) + 3 * E32 * f.abs()
    return f, d1 * dv + inst


def _gelu(g):
    return 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))


def _geglu(a, da, g, dg):
    ge = _gelu(g)
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    d1 = (0.5 * (1 + torch.erf(g / math.sqrt(2.0))) + g * phi).abs()
    f = a * ge
    return f, ge.abs() * da + a.abs() * (d1 * dg + g.abs() * 0.75e-7 + 6 * E32 * ge.abs()) + E32 * f.abs()


def linear_ref(A, W, *, bias=None, rowvec=None, res=None, act=None, out="f16", splitk=1, ln=None, dA=None, dres=None):
    """y = epilogue(A W^T): A [..., K], W [N, K] fp64 holding fp16 values; bias [N]; rowvec, res broadcastable to the
    output.  act: None, 'silu', 'quickgelu', 'geglu' (W = [value rows | gate rows]).  ln = (eps, u): the folded LayerNorm
    (rows of A are the raw stream, u = column sums of W).  dA / dres: A and res are themselves only known to these
    bounds (an fp16 seam in front of this stage): pushed through |W|, or through the first-order map of the
    normalisation, d xn = rstd (dA + mean dA) + |xn| rstd mean(|xn| dA)."""
    K = A.shape[-1]
    acc = A @ W.t()
    absacc = A.abs() @ W.abs().t()
    dv = K * E32H * absacc
    if splitk > 1:
        dv = dv + torch.minimum(splitk * u16(absacc), 2.0 ** -10 * absacc + splitk * 2.0 ** -24) + splitk * E32H * absacc
    v = acc
    if ln is not None:
        eps, u = ln
        mean = A.mean(-1, keepdim=True)
        msq = (A * A).mean(-1, keepdim=True)
        var = (msq - mean * mean).clamp(min=0)
        rstd = 1 / torch.sqrt(var + eps)
        dmean = K * E32H * A.abs().mean(-1, keepdim=True)
        dvar = K * E32H * 2 * msq + 2 * mean.abs() * dmean + 2 * E32H * msq
        drstd = rstd * dvar / (2 * (var + eps)) + E32 * rstd
        v = (acc - mean * u) * rstd
        dv = (dv + dmean * u.abs() + 2 * E32H * (acc.abs() + (mean * u).abs())) * rstd + (acc - mean * u).abs() * drstd \
            + E32H * v.abs()
        if dA is not None:
            xn = (A - mean) * rstd
            dxn = rstd * (dA + dA.mean(-1, keepdim=True)) + xn.abs() * rstd * (xn.abs() * dA).mean(-1, keepdim=True)
            dv = dv + dxn @ W.abs().t()
    elif dA is not None:
        dv = dv + dA @ W.abs().t()
    mag = v.abs()
    for t in (bias, rowvec):
        if t is not None and act != "geglu":
            v = v + t
            mag = mag + t.abs()
    if act == "geglu":
        n = W.shape[0] // 2
        if bias is not None:
            v = v + bias
            mag = mag + bias.abs()
        dv = dv + 2 * E32H * mag
        v, dv = _geglu(v[..., :n], dv[..., :n], v[..., n:], dv[..., n:])
        mag = v.abs()
        if rowvec is not None:
            v = v + rowvec
            mag = mag + rowvec.abs()
            dv = dv + E32H * mag
    else:
        dv = dv + 2 * E32H * mag
        if act is not None:
            v, dv = _act(v, dv, act)
            mag = v.abs()
    if res is not None:
        v = v + res
        dv = dv + E32H * (mag + res.abs()) + (dres if dres is not None else 0)
    dv = dv + (u16(v) if out == "f16" else E32 * v.abs())
    return v, dv


# ---------------------------------------------------------------------------------------------------------------------
# norms
def _norm_terms(x, mean, msq, n, eps):
    var = (msq - mean * mean).clamp(min=0)
    rstd = 1 / torch.sqrt(var + eps)
    dmean = n * E32H * x.abs().mean(-1, keepdim=True)
    dvar = n * E32H * 2 * msq + 2 * mean.abs() * dmean + 2 * E32H * msq
    drstd = rstd * dvar / (2 * (var + eps)) + E32 * rstd
    return rstd, dmean, drstd


def groupnorm_ref(x, groups, gamma, beta, eps, silu, dx=None):
    """x [B, hw, C] (fp64 of fp16 values), gamma / beta [C] -> ([B, hw, C], bound).  dx [B, hw, C]: x is itself only known
    to this bound (the kernel normalises ITS output, which is off from x by up to dx): pushed through the first-order map of
    the normalisation, d xn = rstd (dx + mean dx) + |xn| rstd mean(|xn| dx) with xn = (x - mean) rstd, as in linear_ref."""
    B, hw, C = x.shape
    cpg = C // groups
    grp = lambda t: t.reshape(B, hw, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, hw * cpg)
    xg = grp(x)
    mean = xg.mean(-1, keepdim=True)
    msq = (xg * xg).mean(-1, keepdim=True)
    rstd, dmean, drstd = _norm_terms(xg, mean, msq, hw * cpg, eps)
    gg = gamma.view(1, groups, 1, cpg).expand(B, groups, hw, cpg).reshape(B, groups, hw * cpg)
    bb = beta.view(1, groups, 1, cpg).expand(B, groups, hw, cpg).reshape(B, groups, hw * cpg)
    y = (xg - mean) * rstd * gg + bb
    dy = gg.abs() * (rstd * dmean + (xg - mean).abs() * drstd) \
        + 4 * E32H * ((xg * rstd * gg).abs() + (mean * rstd * gg).abs() + bb.abs())
    if dx is not None:
        dg, xn = grp(dx), ((xg - mean) * rstd).abs()
        dy = dy + gg.abs() * rstd * (dg + dg.mean(-1, keepdim=True) + xn * (xn * dg).mean(-1, keepdim=True))
    if silu:
        y, dy = _act(y, dy, "silu")
    dy = dy + u16(y)
    back = lambda t: t.view(B, groups, hw, cpg).permute(0, 2, 1, 3).reshape(B, hw, C)
    return back(y), back(dy)


def layernorm_ref(x, gamma, beta, eps):
    """x [rows, d] -> ([rows, d], bound)."""
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    msq = (x * x).mean(-1, keepdim=True)
    rstd, dmean, drstd = _norm_terms(x, mean, msq, d, eps)
    y = (x - mean) * rstd * gamma + beta
    dy = gamma.abs() * (rstd * dmean + (x - mean).abs() * drstd) \
        + 4 * E32H * ((x * rstd * gamma).abs() + (mean * rstd * gamma).abs() + beta.abs())
    return y, dy + u16(y)


# ---------------------------------------------------------------------------------------------------------------------
# attention
def attention_ref(q, k, v, scale, causal=False, dq=None):
    """q [B, h, nq, d], k, v [B, h, nkv, d] (fp64 of fp16 values) -> ([B, h, nq, d], bound).  dq: q is only known to
    this bound (the fp16 seam of a query projection in front), which moves the logits by scale dq |k|^T.  The weight
    error is p (exp(dl) - 1), the first-order p dl without its truncation."""
    d, nkv = q.shape[-1], k.shape[-2]
    logit = q @ k.transpose(-1, -2) * scale
    dl = scale * d * E32H * (q.abs() @ k.abs().transpose(-1, -2))
    if causal:
        mask = torch.ones(q.shape[-2], nkv, dtype=torch.bool, device=q.device).triu(1)
        logit = logit.masked_fill(mask, float("-inf"))
    m = logit.max(-1, keepdim=True).values
    p = torch.exp(logit - m)
    lfin = torch.where(torch.isfinite(logit), logit.abs(), torch.zeros_like(logit))
    dl = dl + 4 * E32 * (lfin + m.abs())
    if dq is not None:
        dl = dl + scale * (dq @ k.abs().transpose(-1, -2))
    dp = p * (torch.expm1(2 * dl) + 2 * E32) + torch.where(p > 0, torch.maximum(2.0 ** -10 * p, torch.full_like(p, 2.0 ** -24)),
                                          torch.zeros_like(p))
    den = p.sum(-1, keepdim=True)
    out = (p @ v) / den
    dout = (dp @ v.abs() + out.abs() * dp.sum(-1, keepdim=True) + nkv * E32H * (p @ v.abs())) / den + 3 * E32 * out.abs()
    return out, dout + u16(out)


# ---------------------------------------------------------------------------------------------------------------------
# cases shared by the host and the GPU tests
# name: (cin, cout, (H, W), ks, stride, ups, asym, c2, seg (c3, c4) or None, extras)
CONV_CASES = {
    "c3x3_64_224": dict(cin=64, cout=224, hw=(12, 10), ks=3),
    "c3x3_s2_64_96": dict(cin=64, cout=96, hw=(8, 8), ks=3, stride=2),
    "asym_nchw_f32": dict(cin=32, cout=4, hw=(8, 6), ks=3, stride=2, asym=True, out="nchw_f32"),
    "ups2x_96_64": dict(cin=96, cout=64, hw=(4, 3), ks=3, ups=True),
    "ups2x_96_64_phased": dict(cin=96, cout=64, hw=(4, 3), ks=3, ups=True, phased=True),
    "concat_64_32": dict(cin=64, c2=32, cout=96, hw=(6, 5), ks=3),
    "seg_3_64_96_32_224": dict(cin=64, cout=224, hw=(12, 10), ks=3, seg=(96, 32)),
    "res_rowvec": dict(cin=64, cout=96, hw=(6, 5), ks=3, res=True, rowvec=True),
    "bigtile_224_224": dict(cin=224, cout=224, hw=(32, 20), ks=3),
}
# edge of the range: the largest input scale and four times the weight gain, so the fp64 output has a standard deviation
# of 2^15: about 4 % of it lies beyond 65504, more than 90 % inside 6e4
EDGE_SCALE = 2 ** 13
EDGE_CONV = dict(cin=256, cout=64, hw=(8, 8), ks=1, wgain=4.0)
EDGE_GEMM = (64, 256, 96)
GEMM_CASES = {"g17_768_256": (17, 768, 256), "g96_896_224": (96, 896, 224)}


def conv_case(name, s, act=None, spec=None):
    """Operands (CPU; activations, bias, rowvec, residual scaled by s) of a conv case.  fp16 tensors are what the kernel
    reads; bias / rowvec are fp32 (scaled exactly)."""
    c = dict(stride=1, ups=False, asym=False, c2=0, seg=None, res=False, rowvec=False, out="f16", phased=False, wgain=1.0)
    c.update(spec if spec is not None else CONV_CASES[name])
    B, (H, W), ks = 2, c["hw"], c["ks"]
    seed = sum(ord(ch) for ch in name)
    cin = c["cin"] + c["c2"]
    o = dict(c, name=name, s=s, act=act, B=B)
    x = activations((B, cin, H, W), seed, s)
    o["x1"], o["x2"] = x[:, :c["cin"]], (x[:, c["cin"]:] if c["c2"] else None)
    o["w"] = weights((c["cout"], cin, ks, ks), ks * ks * cin, seed + 1) * c["wgain"]
    o["bias"] = vector(c["cout"], seed + 2) * s
    if c["seg"]:
        c3, c4 = c["seg"]
        o["x3"] = activations((B, c3, H, W), seed + 3, s)
        o["x4"] = activations((B, c4, H, W), seed + 4, s) if c4 else None
        o["w2"] = weights((c["cout"], c3 + c4, 1, 1), c3 + c4, seed + 5)
    Ho, Wo = (2 * H, 2 * W) if c["ups"] else ((H + (1 if c["asym"] else 2 * (ks // 2)) - ks) // c["stride"] + 1,
                                              (W + (1 if c["asym"] else 2 * (ks // 2)) - ks) // c["stride"] + 1)
    o["Ho"], o["Wo"] = Ho, Wo
    if c["res"]:
        o["resid"] = activations((B, Ho, Wo, c["cout"]), seed + 6, s)
    if c["rowvec"]:
        o["rv"] = vector(3 * B * c["cout"], seed + 7, 1.0).view(3, B, c["cout"]) * s
        o["rv_step"] = 2
    return o


def conv_case_ref(o, splitk=1):
    """(ref [B, Ho, Wo, N], bound) of conv_case's operands."""
    d = lambda t: t.to(F64)
    x = d(o["x1"]) if o["x2"] is None else torch.cat([d(o["x1"]), d(o["x2"])], 1)
    w16 = q16(d(o["w"]))
    bias = d(o["bias"])
    rv = d(o["rv"][o["rv_step"]]).view(o["B"], 1, 1, -1) if o["rowvec"] else None
    res = d(o["resid"]) if o["res"] else None
    out = "f16" if o["out"] == "f16" else "f32"
    if o["phased"]:
        B, _, H, W = x.shape
        ref = torch.zeros(B, 2 * H, 2 * W, o["cout"], dtype=F64)
        bnd = torch.zeros_like(ref)
        for (py, px), wp in phase_weights(o["w"]).items():
            A = im2col(x, 2, pad=(1 - py, py, 1 - px, px))
            r, b = linear_ref(A, wmat(q16(d(wp))), bias=bias, act=o["act"], out=out, splitk=splitk)
            ref[:, py::2, px::2], bnd[:, py::2, px::2] = r, b
        return ref, bnd
    A = im2col(x, o["ks"], o["stride"], (0, 1, 0, 1) if o["asym"] else None, o["ups"])
    W = wmat(w16)
    if o["seg"]:
        xs = d(o["x3"]) if o["x4"] is None else torch.cat([d(o["x3"]), d(o["x4"])], 1)
        A = torch.cat([A, xs.permute(0, 2, 3, 1)], -1)
        W = torch.cat([W, wmat(q16(d(o["w2"])))], -1)
    return linear_ref(A, W, bias=bias, rowvec=rv, res=res, act=o["act"], out=out, splitk=splitk)


def gemm_case(name, s, act=None, shape=None, value_gain=1.0, wgain=1.0):
    """a [M, K] fp16 (x s), w [N, K], bias [N] (x s), res [M, N] fp16 (x s).  act 'geglu': N = 2 * inner, rows
    [value | gate]; value_gain (a power of two) multiplies the value rows so that a x gelu(g) stays in range while the
    gate spans the full scale."""
    M, K, N = shape if shape is not None else GEMM_CASES[name]
    seed = sum(ord(ch) for ch in name)
    o = dict(name=name, s=s, act=act, M=M, K=K, N=N)
    o["a"] = activations((M, K), seed, s)
    w = weights((N, K), K, seed + 1) * wgain
    b = vector(N, seed + 2) * s
    if act == "geglu":
        w[: N // 2] *= value_gain
        b[: N // 2] *= value_gain
    o["w"], o["bias"] = w, b
    o["resid"] = activations((M, N), seed + 3, s) if act is None else None
    return o


def gemm_case_ref(o, splitk=1, out="f16", with_res=True):
    d = lambda t: t.to(F64)
    res = d(o["resid"]) if (with_res and o["resid"] is not None) else None
    return linear_ref(d(o["a"]), q16(d(o["w"])), bias=d(o["bias"]), res=res, act=o["act"], out=out, splitk=splitk)


def norm_input(shape, seed, s, chan_dim=-1, device="cpu"):
    """Activations with a per-channel mean and spread: sigma_c in [1/8, 1/2] (a factor 4 between channels), |mu_c| up to
    2.8 sigma_c (near the |mu| / sigma <= 4 the issue allows, with room for the sample statistic), so that the largest
    scale stays inside fp16 (7.3 sigma 2^13 < 65504); groups and rows that mix channels have a smaller ratio (the host
    test checks all three on the data)."""
    assert chan_dim == -1
    C = shape[chan_dim]
    g = torch.Generator().manual_seed(seed + 99)
    sigma = 0.125 + 0.375 * torch.rand(C, generator=g)
    mu = (2 * torch.rand(C, generator=g) - 1) * 2.8 * sigma
    return activations(shape, seed, s, mu=mu, sigma=sigma, device=device)


# (c1, c2), 32 groups, hw 48, B 2.  Groups of 3 channels: NOT the one-launch kernel although hw <= 64 (it has no form for an
# odd group width) but the statistics + apply pair with 2 pixels per chunk; tests/norm_ref.py has the tables per path
GN_CASES = {"gn96": (96, 0), "gn64_32": (64, 32)}
LN_ROWS = ((5, 1024), (33, 224))
LNGEMM_CASES = {"ln96_224_256": (96, 224, 256, None), "ln50_448_512": (50, 448, 512, None),
                "ln96_224_geglu": (96, 224, 512, "geglu")}
# (d, nq, nkv, causal), heads 2, B 2
ATTN_CASES = {"a32_48_87": (32, 48, 87, False), "a64_48_33": (64, 48, 33, False), "a64_48_87": (64, 48, 87, False),
              "a32_48_33": (32, 48, 33, False), "causal64_77": (64, 77, 77, True)}


def gn_case(name, s):
    c1, c2 = GN_CASES[name]
    seed = sum(ord(ch) for ch in name)
    C = c1 + c2
    return dict(x=norm_input((2, 48, C), seed, s), c1=c1, c2=c2, gamma=1 + vector(C, seed + 1), beta=vector(C, seed + 2))


def ln_case(rows, d, s):
    return dict(x=norm_input((rows, d), rows + d, s), gamma=1 + vector(d, d + 1), beta=vector(d, d + 2))


def lngemm_case(name, s):
    """LayerNorm folded into its consumer: weights W gamma (fp16 at packing), bias b + W beta, u = column sums of the
    packed weight.  GEGLU: the value rows carry a gain of 8 at most (the normalised rows are O(1) at every scale)."""
    M, d, N, act = LNGEMM_CASES[name]
    seed = sum(ord(ch) for ch in name)
    gamma, beta = 1 + vector(d, seed + 1, 0.2), vector(d, seed + 2)
    w, b = weights((N, d), d, seed + 3), vector(N, seed + 4)
    wf = (w * gamma[None, :]).contiguous()
    return dict(name=name, M=M, d=d, N=N, act=act, x=norm_input((M, d), seed, s), wf=wf, bf=b + w @ beta,
                u=wf.half().float().sum(1), eps=1e-5)


def lngemm_case_ref(o):
    d = lambda t: t.to(F64)
    W = q16(d(o["wf"]))
    return linear_ref(d(o["x"]), W, bias=d(o["bf"]), act=o["act"], ln=(o["eps"], d(o["u"])))


def attn_case(name, s, shape=None, B=2, heads=2, device="cpu"):
    """q, k scaled by sqrt(s) each (logits reach +-1e4 at 2^13), v by s; [B, n, heads * d] fp16.  shape = (d, nq, nkv,
    causal), B, heads: a shape of the caller's instead of ATTN_CASES[name] (the name then only seeds the generator)."""
    d, nq, nkv, causal = shape if shape is not None else ATTN_CASES[name]
    seed = sum(ord(ch) for ch in name)
    rs = math.sqrt(s)
    assert rs == int(rs) or s == 2 ** 13
    # sqrt(2^13) is not a power of two: 2^6 on q and 2^7 on k
    sq, sk = (2 ** 6, 2 ** 7) if s == 2 ** 13 else (int(rs), int(rs))
    return dict(d=d, nq=nq, nkv=nkv, causal=causal, B=B, heads=heads, scale=d ** -0.5,
                q=activations((B, nq, heads * d), seed, sq, device=device),
                k=activations((B, nkv, heads * d), seed + 1, sk, device=device),
                v=activations((B, nkv, heads * d), seed + 2, s, device=device))


def attn_case_ref(o):
    sp = lambda t, n: t.to(F64).view(o["B"], n, o["heads"], o["d"]).transpose(1, 2)
    return attention_ref(sp(o["q"], o["nq"]), sp(o["k"], o["nkv"]), sp(o["v"], o["nkv"]), o["scale"], o["causal"])


# GEGLU multiplies two pre-activations: with both at scale s the product leaves fp16 at s = 2^10.  The value rows of the
# weight (and their bias) carry this gain over s, a power of two, so the gate spans the full scale (both saturated tails
# of the erf) while value x gelu(gate) stays representable.
GEGLU_VALUE_GAIN = 2.0 ** -3


# ---------------------------------------------------------------------------------------------------------------------
# the fused row chains and the attention with its query projection inside: the references round the fp16 seams the
# kernels store (t0, t1, q, the attention output, the GEGLU product h) and carry each stage's whole bound into the next
HEADS, DH, DP = 8, 28, 32


def _fold(w, gamma, beta):
    """LayerNorm folded into the Linear behind it: (fp16 weight W gamma as fp64, fp32 column sums u, bias W beta)."""
    wf = (w * gamma[None, :]).half()
    return wf.to(F64), wf.float().sum(1), w @ beta


def head_case(s, B=2, hw=64, c=224, dh=DH, dp=DP):
    """proj_in -> t0 (fp16) -> norm1 -> q | k | v; x scaled by s.  c channels, HEADS heads of dh columns (dp: the padded
    head width the kernel stores them at)."""
    inner = HEADS * dh
    return dict(B=B, hw=hw, c=c, heads=HEADS, dh=dh, dp=dp, x=activations((B * hw, c), 11, s), wi=weights((c, c), c, 12),
                bi=vector(c, 13) * s, gamma=1 + vector(c, 14, 0.2), beta=vector(c, 15), wqkv=weights((3 * inner, c), c, 16),
                eps=1e-5)


def head_case_ref(o):
    d = lambda t: t.to(F64)
    t0, dt0 = linear_ref(d(o["x"]), q16(d(o["wi"])), bias=d(o["bi"]))
    t0r = q16(t0)
    wf, u, b = _fold(o["wqkv"], o["gamma"], o["beta"])
    qkv, dqkv = linear_ref(t0r, wf, bias=d(b), ln=(o["eps"], d(u)), dA=dt0)
    return (t0, dt0), (qkv, dqkv)


def cross_case(s, B=2, hw=64, nkv=87, c=224, dh=DH, dp=DP):
    """attn1.to_out (+ t0) -> t1 (fp16) -> norm2 -> to_q -> q (fp16) -> attention over the context -> a2 (fp16) ->
    to_out (+ t1); t0 scaled by s, a1 and the context at O(1).  c channels, HEADS heads of dh columns (dp: the padded
    head width)."""
    inner, M = HEADS * dh, B * hw
    return dict(B=B, hw=hw, c=c, nkv=nkv, heads=HEADS, dh=dh, dp=dp, a1=activations((M, inner), 21),
                t0=activations((M, c), 22, s),
                wo1=weights((c, inner), inner, 23), bo1=vector(c, 24), gamma=1 + vector(c, 25, 0.2), beta=vector(c, 26),
                wq=weights((inner, c), c, 27), wo2=weights((c, inner), inner, 28), bo2=vector(c, 29),
                k=activations((B, nkv, inner), 30), v=activations((B, nkv, inner), 31), eps=1e-5, scale=dh ** -0.5)


def _cross_stages(o):
    """(t1, dt1), (q, dq), (a2, da2) of cross_case's operands, the last two [B * hw, inner]; each bound carries the ones
    in front of it."""
    d = lambda t: t.to(F64)
    B, hw, nkv, heads, dh = o["B"], o["hw"], o["nkv"], o["heads"], o["dh"]
    t1, dt1 = linear_ref(d(o["a1"]), q16(d(o["wo1"])), bias=d(o["bo1"]), res=d(o["t0"]))
    t1r = q16(t1)
    wf, u, b = _fold(o["wq"], o["gamma"], o["beta"])
    q, dq = linear_ref(t1r, wf, bias=d(b), ln=(o["eps"], d(u)), dA=dt1)
    sp = lambda t, n: t.reshape(B, n, heads, dh).transpose(1, 2)
    a2, da2 = attention_ref(sp(q16(q), hw), sp(d(o["k"]), nkv), sp(d(o["v"]), nkv), o["scale"], dq=sp(dq, hw))
    back = lambda t: t.transpose(1, 2).reshape(B * hw, heads * dh)
    return (t1, dt1), (q, dq), (back(a2), back(da2))


def cross_case_ref(o):
    d = lambda t: t.to(F64)
    (t1, dt1), _, (a2, da2) = _cross_stages(o)
    return linear_ref(q16(a2), q16(d(o["wo2"])), bias=d(o["bo2"]), res=q16(t1), dA=da2, dres=dt1)


MLP_CASES = {"mlp96": (96, 32, 0), "mlp128": (128, 64, 64)}  # M, rows per workgroup, hw (0: no GroupNorm partials)


def mlp_case(name, s, B=None, hw=None, rows=None, c=224, M=None):
    """norm3 -> GEGLU -> h (fp16) -> ff.net.2 and proj_out in one GEMM over [h | x] (+ res); x and res scaled by s.
    B, hw, rows: a shape of the caller's (B samples of hw rows, `rows` per workgroup) instead of MLP_CASES[name]; M (with
    rows): M rows and no GroupNorm partials (hw = 0), e.g. a tail tile with rows past M."""
    M, rows, hw = (M, rows, 0) if M is not None else MLP_CASES[name] if B is None else (B * hw, rows, hw)
    inner = 4 * c
    return dict(M=M, rows=rows, hw=hw, c=c, inner=inner, x=norm_input((M, c), 41 + M, s), res=activations((M, c), 42, s),
                gamma=1 + vector(c, 43, 0.2), beta=vector(c, 44), w1=weights((2 * inner, c), c, 45), b1=vector(2 * inner, 46),
                w2h=weights((c, inner), inner, 47), w2x=weights((c, c), c, 48), b2=vector(c, 49) * s, eps=1e-5)


def mlp_case_ref(o):
    d = lambda t: t.to(F64)
    wf, u, b = _fold(o["w1"], o["gamma"], o["beta"])
    h, dh = linear_ref(d(o["x"]), wf, bias=d(o["b1"] + b), act="geglu", ln=(o["eps"], d(u)))
    A = torch.cat([q16(h), d(o["x"])], -1)
    W = torch.cat([q16(d(o["w2h"])), q16(d(o["w2x"]))], -1)
    return linear_ref(A, W, bias=d(o["b2"]), res=d(o["res"]), dA=torch.cat([dh, torch.zeros_like(d(o["x"]))], -1))


# ---------------------------------------------------------------------------------------------------------------------
# every compiled row-chain instantiation, and operands that make all stages but one exact, so that the output is held to
# that stage's own bound.  Shared by tests/test_row_chain_stages_{host,gpu}.py.
MLP_STREAM = 0x1000  # include/upk.h UPK_MLP_STREAM
XBLOCK_FAMILIES = {(224, 32): 28, (448, 64): 56}  # (c, padded head dim) -> real head dim; inner = 8 dh = c in both
ROW_CHAIN_DEFAULT_ROWS = {"xblock": 32, "hblock": 32, "mlp": 64}  # what rows_per_wg = 0 means
STAGE_SCALES = (1, 2 ** 10)   # the scale of the residual stream in the single-stage probes (the full chains: SCALES)
X2_NKV = (1, 16, 17, 80, 87, 96)  # both sides of a 16-key fragment edge, the production 87, the unmasked 96
X2_KEY_SCALES = (1, 4)        # diffuse and peaked softmax (ATTN_VARIANT_SCALES' logit gains)
GN_FOLD = dict(groups=32, eps=1e-6, ld_extra=32)


def _row_chain():
    rows = []
    for (c, d), dh in XBLOCK_FAMILIES.items():
        for r in ((16, 32, 64, 128) if c == 224 else (16, 32)):
            rows.append(dict(kind="xblock", c=c, d=d, dh=dh, rows=r, stream=False, gn=False))
    for r in (16, 32, 64, 128):
        for gn in (False, True):
            rows.append(dict(kind="hblock", c=224, d=32, dh=28, rows=r, stream=False, gn=gn))
    for r, st in ((32, False), (64, False), (128, True), (64, True)):
        rows.append(dict(kind="mlp", c=224, d=0, dh=0, rows=r, stream=st, gn=False))
    return rows


ROW_CHAIN = _row_chain()


def row_chain_key(row):
    return (row["kind"], row["c"], row["d"], row["rows"], row["stream"], row["gn"])


def row_chain_id(row):
    return "%s-c%d-rows%d%s%s" % (row["kind"], row["c"], row["rows"], "s" if row["stream"] and row["rows"] != 128 else "",
                                  "-gn" if row["gn"] else "")


def row_chain_shapes(row):
    """(B, hw, M) of a table row: one workgroup per sample (the sample boundary, the per-sample K / V^T bases), two tiles
    per sample (tok0 of the V^T store, the partial-block index), and for the MLP a tail tile with rows past M (hw = 0)."""
    r = row["rows"]
    shapes = [(2, r, 2 * r), (2, 2 * r, 4 * r)]
    if row["kind"] == "mlp":
        shapes.append((1, 0, r + 8))
    return shapes


def mlp_rows_per_wg(row):
    """The descriptor's rows_per_wg of an MLP table row."""
    return row["rows"] | (MLP_STREAM if row["stream"] and row["rows"] != 128 else 0)


def cross_probe(probe, s, B, hw, nkv, c=224, dh=DH, dp=DP, ks=1):
    """cross_case's operands with all stages but one made exact (ks multiplies the context keys):
      'X1'  w_q = 0, so q = 0 and every softmax is uniform over finite values; w_out2 = 0, b_out2 = 0, so the last GEMM
            adds exact zeros to the t1 the kernel keeps as fp16: y = fp16(t1), the first GEMM alone.
      'X2'  a1 = 0, b_out1 = 0: t1 = fp16(0 + 0 + t0) = t0 exactly.  w_out2 = I (inner = c), b_out2 = 0: every dot product
            of the last GEMM is one fp16 value times 1 plus exact zeros, so y = fp16(fp16(a2) + t0): LayerNorm, the query
            projection and the attention, then one fp32 addition and the output rounding.
      'X3'  as X2 with the general w_out2 / b_out2: the last GEMM behind the seam of a2.
      'X4'  the full chain."""
    o = cross_case(s, B=B, hw=hw, nkv=nkv, c=c, dh=dh, dp=dp)
    o["probe"], o["ks"] = probe, ks
    if ks != 1:
        o["k"] = (o["k"] * float(ks)).half()
    if probe == "X1":
        o["wq"], o["wo2"], o["bo2"] = torch.zeros_like(o["wq"]), torch.zeros_like(o["wo2"]), torch.zeros_like(o["bo2"])
    elif probe in ("X2", "X3"):
        o["a1"], o["bo1"] = torch.zeros_like(o["a1"]), torch.zeros_like(o["bo1"])
        if probe == "X2":
            assert HEADS * dh == c
            o["wo2"], o["bo2"] = torch.eye(c), torch.zeros_like(o["bo2"])
    else:
        assert probe == "X4"
    return o


def _attention_behind_ln(o, t):
    """(a2, da2) [B * hw, inner] of cross_case's attention over rows t that are exact (no seam in front)."""
    d = lambda v: v.to(F64)
    B, hw, nkv, heads, dh = o["B"], o["hw"], o["nkv"], o["heads"], o["dh"]
    wf, u, b = _fold(o["wq"], o["gamma"], o["beta"])
    q, dq = linear_ref(t, wf, bias=d(b), ln=(o["eps"], d(u)))
    sp = lambda v, n: v.reshape(B, n, heads, dh).transpose(1, 2)
    a2, da2 = attention_ref(sp(q16(q), hw), sp(d(o["k"]), nkv), sp(d(o["v"]), nkv), o["scale"], dq=sp(dq, hw))
    back = lambda v: v.transpose(1, 2).reshape(B * hw, heads * dh)
    return back(a2), back(da2)


def cross_probe_ref(o):
    """(ref, bound) of y for cross_probe's operands: the inexact stage's own bound, no term for the exact ones."""
    d = lambda t: t.to(F64)
    probe, t0 = o["probe"], d(o["t0"])
    if probe == "X1":
        return linear_ref(d(o["a1"]), q16(d(o["wo1"])), bias=d(o["bo1"]), res=t0)
    if probe == "X4":
        return cross_case_ref(o)
    a2, da2 = _attention_behind_ln(o, t0)
    if probe == "X3":
        return linear_ref(q16(a2), q16(d(o["wo2"])), bias=d(o["bo2"]), res=t0, dA=da2)
    y = a2 + t0  # X2: da2 holds the rounding of a2 to fp16; then one fp32 addition and the output rounding
    return y, da2 + E32H * (a2.abs() + t0.abs()) + u16(y)


def head_probe(probe, s, B, hw, c=224, dh=DH, dp=DP):
    """head_case's operands:
      'H1'  the full chain; t0 is a direct output and is checked at linear_ref's bound, q | k | v behind its seam.
      'H2'  w_in = I, b_in = 0: every dot product of the first GEMM is one fp16 value times 1 plus exact zeros, so
            t0 = x bit for bit and q | k | v are the folded-LayerNorm GEMM alone.
      'F1', 'F2'  the GroupNorm fold: x is the un-normalised input, whose per-(row block, channel) partial sums the test
            supplies (fp32 sums of hw / nblk rows each, nblk = max(1, hw / 16), leading dimension c + 32).  F2 has w_in = I,
            b_in = 0, so t0 = fp16(GroupNorm(x)) and q | k | v lie one seam behind it; F1 is the full chain behind it."""
    o = head_case(s, B=B, hw=hw, c=c, dh=dh, dp=dp)
    o["probe"] = probe
    if probe in ("H2", "F2"):
        o["wi"], o["bi"] = torch.eye(c), torch.zeros_like(o["bi"])
    if probe in ("F1", "F2"):
        o["x"] = norm_input((B * hw, c), 17, s)
        nblk = max(1, hw // 16)
        xf = o["x"].float().reshape(B, nblk, hw // nblk, c)
        part = torch.zeros(B, nblk, 2, c + GN_FOLD["ld_extra"])
        part[..., :c] = torch.stack([xf.sum(2), (xf * xf).sum(2)], 2)
        o.update(gn_part=part, gn_nblk=nblk, gn_gamma=1 + vector(c, 18, 0.3), gn_beta=vector(c, 19, 0.2),
                 gn_groups=GN_FOLD["groups"], gn_eps=GN_FOLD["eps"])
    else:
        assert probe in ("H1", "H2")
    return o


def head_probe_ref(o):
    """((t0, dt0), (qkv, dqkv)); H2: dt0 is None, t0 must equal x bit for bit.  The GroupNorm statistics of the fold come
    from exact fp32 partials of hw / nblk terms each, summed over nblk blocks in fp32 and over the group's channels in
    fp64: at most hw / nblk + nblk terms per channel, inside the hw c / groups terms groupnorm_ref allows for."""
    d = lambda t: t.to(F64)
    probe = o["probe"]
    if probe == "H1":
        return head_case_ref(o)
    wf, u, b = _fold(o["wqkv"], o["gamma"], o["beta"])
    ln = (o["eps"], d(u))
    if probe == "H2":
        return (d(o["x"]), None), linear_ref(d(o["x"]), wf, bias=d(b), ln=ln)
    B, hw, c = o["B"], o["hw"], o["c"]
    gn, dgn = groupnorm_ref(d(o["x"]).reshape(B, hw, c), o["gn_groups"], d(o["gn_gamma"]), d(o["gn_beta"]), o["gn_eps"], False)
    gn, dgn = gn.reshape(B * hw, c), dgn.reshape(B * hw, c)
    if probe == "F2":
        return (gn, dgn), linear_ref(q16(gn), wf, bias=d(b), ln=ln, dA=dgn)
    t0, dt0 = linear_ref(q16(gn), q16(d(o["wi"])), bias=d(o["bi"]), dA=dgn)
    return (t0, dt0), linear_ref(q16(t0), wf, bias=d(b), ln=ln, dA=dt0)


def mlp_probe(probe, s, B, hw, rows, c=224, M=None):
    """mlp_case's operands:
      'M1'  w2h = 0: the hidden tile is finite and meets exact zeros, y = res + x W2x^T + b2, the second GEMM alone.
      'M2j' (j = 0..3)  w2x = 0, b2 = 0, res = 0 and w2h selects the hidden columns [c j, c j + c): every dot product is
            one fp16 value times 1 plus exact zeros, so y = fp16(h) on those columns: LayerNorm and GEGLU alone.  The four
            probes cover every hidden column, hence both LDS slices of the streaming form at every position.
      'M3'  the full chain (and the GroupNorm partials it leaves)."""
    o = mlp_case("probe", s, B=B, hw=hw, rows=rows, c=c) if M is None else mlp_case("probe", s, rows=rows, c=c, M=M)
    o["probe"] = probe
    if probe == "M1":
        o["w2h"] = torch.zeros_like(o["w2h"])
    elif probe.startswith("M2"):
        j = int(probe[2:])
        sel = torch.zeros_like(o["w2h"])
        sel[torch.arange(c), c * j + torch.arange(c)] = 1.0
        o.update(w2h=sel, w2x=torch.zeros_like(o["w2x"]), b2=torch.zeros_like(o["b2"]), res=torch.zeros_like(o["res"]))
    else:
        assert probe == "M3"
    return o


def mlp_hidden_ref(o):
    """(h, dh) [M, inner]: the GEGLU hidden tile of mlp_case's operands at its single-stage bound."""
    d = lambda t: t.to(F64)
    wf, u, b = _fold(o["w1"], o["gamma"], o["beta"])
    return linear_ref(d(o["x"]), wf, bias=d(o["b1"] + b), act="geglu", ln=(o["eps"], d(u)))


def mlp_probe_ref(o, hidden=None):
    """(ref, bound) of y; hidden: mlp_hidden_ref(o) computed before (the four M2 probes share it)."""
    d = lambda t: t.to(F64)
    probe, c = o["probe"], o["c"]
    if probe == "M1":
        return linear_ref(d(o["x"]), q16(d(o["w2x"])), bias=d(o["b2"]), res=d(o["res"]))
    if probe == "M3":
        return mlp_case_ref(o)
    j = int(probe[2:])
    h, dh = hidden if hidden is not None else mlp_hidden_ref(o)
    return h[:, c * j:c * j + c], dh[:, c * j:c * j + c]


QPROJ = dict(C=224, heads=8, dh=28, nq=64, nkv=87)


def qproj_case(s, shape=None, B=2):
    """LayerNorm -> to_q -> q (fp16) -> cross-attention.  The normalisation makes q O(1) whatever the scale of x, so the
    scale goes to x (s), to k (sqrt(s), as in attn_case: logits of a few hundred, where one fp16 ulp of q still moves
    them by less than one) and to v (s).  shape: a dict with QPROJ's keys, instead of QPROJ."""
    shape = dict(shape if shape is not None else QPROJ)
    C, heads, dh, nq, nkv = (shape[k] for k in ("C", "heads", "dh", "nq", "nkv"))
    sk = 2 ** 7 if s == 2 ** 13 else int(math.sqrt(s))
    return dict(B=B, s=s, x=norm_input((B, nq, C), 51, s), w=weights((heads * dh, C), C, 52), gamma=1 + vector(C, 53, 0.2),
                beta=vector(C, 54), k=activations((B, nkv, heads, dh), 55, sk), v=activations((B, nkv, heads, dh), 56, s),
                eps=1e-5, scale=dh ** -0.5, **shape)


def qproj_case_ref(o):
    d = lambda t: t.to(F64)
    B, nq, heads, dh = o["B"], o["nq"], o["heads"], o["dh"]
    wf, u, b = _fold(o["w"], o["gamma"], o["beta"])
    q, dq = linear_ref(d(o["x"]).reshape(B * nq, -1), wf, bias=d(b), ln=(o["eps"], d(u)))
    sp = lambda t: t.reshape(B, nq, heads, dh).transpose(1, 2)
    return attention_ref(sp(q16(q)), d(o["k"]).transpose(1, 2), d(o["v"]).transpose(1, 2), o["scale"], dq=sp(dq))


# ---------------------------------------------------------------------------------------------------------------------
# every compiled attention instantiation (upk_attention_variant_name) at the smallest shapes that reach each of its code
# paths, and the two operand layouts they are run in.  Shared by tests/test_attention_variants_{host,gpu}.py.
ATTN_VARIANT_SCALES = (1, 4, 2 ** 10)  # diffuse, peaked, near one-hot (attn_case's convention: sqrt(s) on q and k, s on v)
ATTN_WPB = {"direct": (1, 2, 4), "qproj": (1, 2, 4), "lds": (4,), "wide": (4,)}  # waves per workgroup a family runs with
ATTN_FILL = 7.0  # what `out` holds before the launch
QPROJ_VARIANT_SHAPES = {32: (224, 28), 64: (448, 56)}  # padded head dim -> (input channels, real head dim)


def attn_variant_name(family, d, qt):
    return family + str(d) + ("q%d" % qt if (d <= 128) else "")


def launch_geometry(nq, qt, wpb):
    """(workgroups along the queries, valid rows of the last live wave, waves with no valid query) of nq queries in
    waves of 16 qt rows, wpb waves per workgroup."""
    rows = 16 * qt
    live = -(-nq // rows)
    wgs = -(-nq // (rows * wpb))
    return wgs, nq - (live - 1) * rows, wgs * wpb - live


def attn_variant_rows():
    """The table: one dict per (variant, shape).  `wpbs`: the waves per workgroup the row is launched with (all give the
    same bits); `w`: the one its n_q was sized for, and `claim` = (workgroups, valid rows of the last live wave, idle waves)
    at that w, written out here and recomputed from launch_geometry by the host test."""
    rows = []

    def add(family, d, qt, nq, nkv, w, claim, causal=False, B=2, heads=3, **kw):
        rows.append(dict(family=family, variant=attn_variant_name(family, d, qt), d=d, qt=qt, nq=nq, nkv=nkv, w=w, claim=claim,
                         causal=causal, B=B, heads=heads, wpbs=ATTN_WPB[family], **kw))

    # n_q = 16 qt w + 16 qt + 5: one workgroup more than the full ones; the last live wave holds 5 valid rows (with qt = 2
    # its second group is wholly invalid); w = 1 makes that three workgroups of one wave, w = 2 two workgroups with every
    # wave live, w = 4 two workgroups whose last two waves lie past the end
    ragged = {1: (3, 5, 0), 2: (2, 5, 0), 4: (2, 5, 2)}
    for d in (32, 64, 128):
        for qt in (1, 2):
            for w in (1, 2, 4):
                # 1: a single key; 33: a 32-key tile, then a tail tile with one valid key; 64: exactly one 64-key tile;
                # 95: a 64-key tile, then a masked tail; 160: two 64-key tiles, then a full 32-key tile
                for nkv in (1, 33, 64, 95, 160):
                    add("direct", d, qt, 16 * qt * w + 16 * qt + 5, nkv, w, ragged[w])
    for d in (256, 512):
        for w in (1, 2, 4):
            for nkv in (1, 50, 96):
                add("direct", d, 1, 16 * w + 21, nkv, w, ragged[w], heads=3 if d == 256 else 2)
    # one head of 512 with a ragged key count: the fall-through from the wide path to attn_kernel<512,0,1>
    add("direct", 512, 1, 16 * 4 + 21, 50, 4, ragged[4], heads=1)
    # causal (n_q == n_kv == n): 1 key; 17: two waves at qt = 1; 77: CLIP's length; 150: the 64-key loop with the q0-limited
    # end, then the 32-key form
    causal_claim = {(1, 1): (1, 1, 3), (1, 2): (1, 1, 3), (17, 1): (1, 1, 2), (17, 2): (1, 17, 3), (77, 1): (2, 13, 3),
                    (77, 2): (1, 13, 1), (150, 1): (3, 6, 2), (150, 2): (2, 22, 3)}
    for d in (32, 64):
        for qt in (1, 2):
            for n in (1, 17, 77, 150):
                add("direct", d, qt, n, n, 4, causal_claim[(n, qt)], causal=True)
    for qt in (1, 2):
        add("direct", 128, qt, 77, 77, 4, causal_claim[(77, qt)], causal=True)
    # LDS-staged: four and five 64-key tiles (the last one in either buffer); 7 queries (one live wave of four), and
    # 64 qt + 21: two workgroups, the second with 21 rows (qt = 1: 16 + 5 in two waves; qt = 2: one wave, 16 + 5 in its
    # two groups) and waves with no valid query that still have to reach every barrier
    lds_claim = {(7, 1): (1, 7, 3), (7, 2): (1, 7, 3), (85, 1): (2, 5, 2), (149, 2): (2, 21, 3)}
    for d in (32, 64):
        for qt in (1, 2):
            for nkv in (256, 320):
                for nq in (7, 64 * qt + 21):
                    add("lds", d, qt, nq, nkv, 4, lds_claim[(nq, qt)])
    # wide: one tile (nothing is prefetched), three and five tiles; 1, 70 (two workgroups, 6 rows in the second) and 128
    # queries (two full workgroups); ldk = 512 is the dense layout, ldk = 1024 the production one
    wide_claim = {1: (1, 1, 3), 70: (2, 6, 3), 128: (2, 16, 0)}
    for nkv in (32, 96, 160):
        for nq in (1, 70, 128):
            add("wide", 512, 1, nq, nkv, 4, wide_claim[nq], B=3, heads=1)
    # query projection inside: (input channels, padded head dim, real head dim) = (224, 32, 28) with two query groups per
    # wave and (448, 64, 56) with one
    for d, qt in ((32, 2), (64, 1)):
        for w in (1, 2, 4):
            for nkv in (1, 64, 87):
                add("qproj", d, qt, 16 * qt * w + 16 * qt + 5, nkv, w, ragged[w])
    return rows


def attn_variant_case(row, s, device="cpu"):
    """The operands of a table row at scale s: attn_case's dict, or qproj_case's for the qproj family."""
    if row["family"] == "qproj":
        C, dh = QPROJ_VARIANT_SHAPES[row["d"]]
        return qproj_case(s, dict(C=C, heads=row["heads"], dh=dh, nq=row["nq"], nkv=row["nkv"]), B=row["B"])
    name = "%s_%d_%d" % (row["variant"], row["nq"], row["nkv"])
    return attn_case(name, s, (row["d"], row["nq"], row["nkv"], row["causal"]), B=row["B"], heads=row["heads"], device=device)


def attn_layout(q, k, v, heads, d, nq, layout):
    """Device (or host) buffers and leading dimensions for one launch.  q [B, nq, heads * d] or None (the qproj entry point
    has no q), k, v [B, nkv, heads * d], fp16.
      'dense':       q, k, out contiguous, vt_ld = round_up(nkv, 32).
      'production':  q and k are the column halves of one [B * n, 2 heads d] buffer when nq == nkv (the self-attention of
                     the engines), else column slices of two such buffers whose other half holds NaN; vt_ld =
                     round_up(nkv, 32) + 32 with NaN in the columns at and beyond round_up(nkv, 32), which no kernel may
                     read; out starts a [B, nq + 2, heads d + 8] buffer.
    Both: vt holds zeros in [nkv, round_up(nkv, 32)); out holds ATTN_FILL.  -> dict with the tensors q, k, vt, out (their
    data_ptr() is what the launch gets), the buffer out lives in, and ldq, qbs, ldk, kbs, vt_ld, ldo, obs."""
    B, nkv, hd = k.shape
    assert hd == heads * d and layout in ("dense", "production")
    new = lambda shape, val: torch.full(shape, val, dtype=torch.float16, device=k.device)
    nan, rup = float("nan"), (nkv + 31) // 32 * 32
    L = dict(layout=layout, q=None, nq=nq, nkv=nkv, hd=hd)
    if layout == "dense":
        L.update(q=q.contiguous() if q is not None else None, k=k.contiguous(), ldq=hd, qbs=nq * hd, ldk=hd, kbs=nkv * hd,
                 vt_ld=rup, ldo=hd, obs=nq * hd)
        vt, L["out_buf"] = new((B, heads, d, rup), 0.0), new((B, nq, hd), ATTN_FILL)
    else:
        if q is not None and nq == nkv:
            qb = kb = new((B * nq, 2 * hd), nan)
        else:
            qb, kb = (new((B * nq, 2 * hd), nan) if q is not None else None), new((B * nkv, 2 * hd), nan)
        if q is not None:
            qb[:, :hd] = q.reshape(B * nq, hd)
            L["q"] = qb[:, :hd]
        kb[:, hd:] = k.reshape(B * nkv, hd)
        L.update(k=kb[:, hd:], ldq=2 * hd, qbs=nq * 2 * hd, ldk=2 * hd, kbs=nkv * 2 * hd, vt_ld=rup + 32, ldo=hd + 8,
                 obs=(nq + 2) * (hd + 8))
        vt, L["out_buf"] = new((B, heads, d, rup + 32), nan), new((B, nq + 2, hd + 8), ATTN_FILL)
        vt[..., :rup] = 0
    vt[..., :nkv] = v.reshape(B, nkv, heads, d).permute(0, 2, 3, 1)
    L.update(vt=vt, out=L["out_buf"])
    return L


def attn_layout_decode(L, B, heads, d):
    """(q or None, k, v) [B, n, heads * d] read back from a layout's buffers through its leading dimensions alone."""
    hd, nq, nkv = heads * d, L["nq"], L["nkv"]
    q = torch.as_strided(L["q"], (B, nq, hd), (L["qbs"], L["ldq"], 1)) if L["q"] is not None else None
    k = torch.as_strided(L["k"], (B, nkv, hd), (L["kbs"], L["ldk"], 1))
    v = torch.as_strided(L["vt"], (B, heads, d, nkv), (heads * d * L["vt_ld"], d * L["vt_ld"], L["vt_ld"], 1))
    return q, k, v.permute(0, 3, 1, 2).reshape(B, nkv, hd)


def attn_owned(L):
    """The part of a layout's out buffer the launch owns: [B, nq, heads * d]."""
    return L["out_buf"][:, :L["nq"], :L["hd"]]


def attn_outside_untouched(L):
    """True when every element of the out buffer outside [0, nq) x [0, heads d) still holds ATTN_FILL bit for bit."""
    t = L["out_buf"].clone()
    t[:, :L["nq"], :L["hd"]] = ATTN_FILL
    return bool((t.view(torch.int16) == torch.tensor(ATTN_FILL, dtype=torch.float16).view(torch.int16).item()).all())


# ---------------------------------------------------------------------------------------------------------------------
# model-level probe: the tiny UNet with its residual streams pushed to 1e3 .. 1e4
PROBE_GAIN = 128.0        # max |h| over the oracle's taps 2.4e3 (inside [1e3, 4e3]); a power of two
PROBE_GAIN_REPORT = 512.0  # max |h| 9.8e3: reported only
# relative MSE of the fp64 oracle with every layer output rounded to fp16 against the plain fp64 oracle, at PROBE_GAIN
# (computed on the CPU; the host test recomputes it): the error fp16 STORAGE alone costs
E_SEAM = 5.05e-6


def probe_inputs():
    from upgpt_amd import synth
    inp = synth.synth_inputs(2, (32, 24), 4, 87, 768, seed=3)
    return inp, torch.tensor([981, 401])


def stress_state(sd, g):
    """Recipe weights with the residual-producing convs (ResBlock out_layers.3) and the transformers' proj_out, weight and
    bias, multiplied by g: every residual branch adds g times as much to the stream."""
    return {k: (v * g if (".out_layers.3." in k or ".proj_out." in k) else v)
            for k, v in sd.items() if k.startswith("model.diffusion_model.")}


def probe_oracle(sd, g, round_fn=None):
    """(eps, max |h| over the taps) of the fp64 oracle on the stress state."""
    from oracle import unet as o_unet
    from upgpt_amd import synth
    inp, t = probe_inputs()
    sd64 = {k: v.to(F64) for k, v in stress_state(sd, g).items()}
    taps = {}
    x = torch.cat([inp["x_T"], inp["c_concat"]], 1)
    y = o_unet.unet_forward(sd64, synth.TINY_UNET, x, t, inp["c_crossattn"].to(F64), taps=taps, dtype=F64, round_fn=round_fn)
    return y, max(float(v.abs().max()) for v in taps.values())


def rel_mse(a, b):
    return float(((a.to(F64) - b) ** 2).mean() / (b ** 2).mean())
