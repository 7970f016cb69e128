"""Case tables and fp64 references for the path tests of upgpt_amd/csrc/norm.hip (tests/test_norm_paths_host.py and
tests/test_norm_paths_gpu.py).  No tolerance of its own:

* y is judged by range_ref.groupnorm_ref / layernorm_ref as they are.
* Sums the kernels leave in a workspace follow launch_ref.sum_refs' rule: an fp32 sum of n values, in any order, is off
  by at most n e32 sum|x|; a sum of n squares by (n + 1) e32 sum x^2 (one more rounding for the square).  For
  gn_stats_kernel n is the number of values the chunk contributes to the group: (pixels of the chunk) x (channels per
  group) (``stats_chunk_refs``).
* Mode-2 partials are per-(row block, channel) fp32 sums of the rows of the block: n = rows (``partial_refs``).  Their
  fold, upk_groupnorm_finalize_f32, adds them in fp64 and rounds ONCE to fp32: the sum of the partials' own bounds plus
  e32 sum|partial| (``fold_refs``).

The tables state, next to each shape, the path / chunking / apply geometry the case is there for.  The GPU tests
assert each against upk_groupnorm_plan before the launch, so a table that drifts away from the dispatch fails there and
does not silently run another kernel.  Data: range_ref.norm_input (|mu| / sigma <= 2.8 per channel).

The large cases (``REFILL``, ``FINALIZE``) are treated one sample at a time (launch_ref's convention): no fp64 tensor
of a whole batch is built; the GPU tests draw and reference them on the device.

``emu_*``: the same operations in fp32 in the kernels' summation order (host test: the reference algorithm is inside its
own bounds, so the bounds are reachable), and ``mut_*`` / the ``keep`` / ``roll`` hooks: near misses of the algorithm the
bounds must tell from it.
"""
import torch

import launch_ref as LR
import range_ref as R

F64 = torch.float64
E32H = R.E32H
SCALES = R.STAGE_SCALES
EPS = (1e-5, 1e-6)
PATHS = ("onepass_v8n2", "onepass_v8n4", "onepass_v4n4", "onepass_v4n8", "onepass_v2n8", "twopass")

# Group A, upk_groupnorm_stats_nhwc_f16: name -> (c1, c2, hw, B, groups, nchunks, pix_per_chunk)
STATS_CASES = {
    "s32_65": (32, 0, 65, 2, 32, 22, 3),            # rpi 64: first size past the one-pass limit, most row slots empty
    "s224_768": (224, 0, 768, 2, 32, 32, 24),       # vpr 28, rpi 9, 4 idle threads; tail loop only
    "s224_2400": (224, 0, 2400, 2, 32, 32, 75),     # ppc 75 >= 8 * 9: unrolled loop, then the tail
    "s128_4100": (128, 0, 4100, 2, 32, 32, 129),    # rpi 16: one unrolled pass + a tail for row slot 0; last chunk 101
    "s96_64_700": (96, 64, 700, 3, 32, 32, 22),     # cpg 5: groups straddle the 16-byte vectors and the seam
    "s896_448_192": (896, 448, 192, 2, 32, 32, 6),  # cpg 42, vpr 168, rpi 1, 88 idle threads
    "s2048_33": (2048, 0, 33, 1, 32, 17, 2),        # vpr 256
    "s128g16_300": (128, 0, 300, 2, 16, 30, 10),    # 16 groups
}
# Group B, upk_groupnorm_nhwc_f16 at <= 64 pixels (and the first size past): name -> (c1, c2, hw, B, groups, path)
ONEPASS_CASES = {
    "o256_64": (256, 0, 64, 2, 32, "onepass_v8n2"),
    "o1024_1024_64": (1024, 1024, 64, 2, 32, "onepass_v8n2"),
    "o2048g16_64": (2048, 0, 64, 2, 16, "onepass_v8n4"),      # v8n4 needs fewer than 32 groups
    "o896_64": (896, 0, 64, 2, 32, "onepass_v4n4"),
    "o1984g16_64": (1984, 0, 64, 2, 16, "onepass_v4n8"),      # cpg 124
    "o896_448_64": (896, 448, 64, 2, 32, "onepass_v2n8"),     # the seam inside a group
    "o896_448_16": (896, 448, 16, 2, 32, "onepass_v2n8"),
    "o1984_64": (1984, 0, 64, 2, 32, "onepass_v2n8"),         # cpg 62, nv 8: every slot used
    "o32_1": (32, 0, 1, 2, 32, "twopass"),                    # cpg 1: no vector width divides an odd group
    "o96_48": (96, 0, 48, 2, 32, "twopass"),                  # cpg 3 (range_ref.GN_CASES' shape)
    "o256_65": (256, 0, 65, 2, 32, "twopass"),                # the other side of hw = 64 | 65 for o256_64
}
# Group C, mode-2 apply: name -> (c1, c2, hw, B, groups, nblk1, nblk2, stats_ld1, stats_ld2)
MODE2_CASES = {
    "m224_b1": (224, 0, 224, 2, 32, 1, 0, 224 + 24, 0),
    "m224_b7": (224, 0, 224, 2, 32, 7, 0, 224 + 24, 0),
    "m224_b32": (224, 0, 224, 2, 32, 32, 0, 224 + 24, 0),
    "m896_448_b3_32": (896, 448, 96, 2, 32, 3, 32, 896 + 8, 448 + 40),  # cpg 42, the producers block differently
}
# Group C, upk_groupnorm_finalize_f32: name -> (c, hw, B, groups, nblk, ld, mode-1 apply afterwards)
FINALIZE_CASES = {
    "f128_16384": (128, 16384, 2, 32, 256, 128 + 24, True),    # 1024 (block, channel) pairs per group: one stride
    "f128_65536": (128, 65536, 2, 32, 1024, 128 + 24, False),  # 4096 pairs: four strides
}
# Group D, the refill loop of gn_apply_kernel: the smallest element count with rows_per_block * C / 8 > 1024
REFILL = dict(c=128, hw=65600, B=4, groups=32, nchunks=32, ppc=2050, rows=65, blocks=1010, eps=1e-6, silu=True)
# Group E, upk_layernorm_f16: nv = 1, 28, 64 | 65, 128 | 129, 256 (VPL 1 | 2 | 4 on both sides of both thresholds)
LN_D = (8, 224, 512, 520, 1024, 1032, 2048)
LN_ROWS = (1, 5, 33)


def seed_of(name):
    return sum(ord(ch) for ch in name)


def gn_data(name, c, hw, B, s, device="cpu"):
    """x [B, hw, c] fp16, gamma, beta [c] fp32 of the case `name`."""
    seed = seed_of(name)
    return R.norm_input((B, hw, c), seed, s, device=device), 1 + R.vector(c, seed + 1), R.vector(c, seed + 2)


def ln_data(rows, d, s):
    return R.norm_input((rows, d), 7 * rows + d, s), 1 + R.vector(d, d + 1), R.vector(d, d + 2)


def stats_geometry(C):
    """(vpr, rpi) of gn_stats_kernel: 16-byte vectors per pixel, pixels in flight (row slots)."""
    vpr = C // 8
    return vpr, 256 // vpr


def straddling_group(c1, c2, groups):
    """The group whose channels lie on both sides of the concat seam, or None."""
    if not c2:
        return None
    cpg = (c1 + c2) // groups
    return c1 // cpg if c1 % cpg else None


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references
def _group_sums(v, groups):
    """v [B, npix, C] -> (sum, sum|.|, sum of squares) per group [B, groups]."""
    B, npix, C = v.shape
    g = v.reshape(B, npix, groups, C // groups)
    return g.sum((1, 3)), g.abs().sum((1, 3)), (g * g).sum((1, 3))


def pixel_sums(x, idx, groups):
    """[B, groups, 2]: (sum, sum of squares) of the pixels `idx` of x [B, hw, C] (fp64)."""
    s, _, q = _group_sums(x[:, idx], groups)
    return torch.stack([s, q], -1)


def stats_chunk_refs(x, groups, nchunks, pix_per_chunk):
    """x [B, hw, C] fp64 -> (ref, bound) [B, nchunks, groups, 2] of the workspace upk_groupnorm_stats_nhwc_f16 leaves:
    chunk k holds the sum and the sum of squares of the pixels [k ppc, min(hw, (k + 1) ppc)) of each group; bounds by
    launch_ref.sum_refs' rule with n = the number of values the chunk contributes."""
    B, hw, C = x.shape
    cpg = C // groups
    assert (nchunks - 1) * pix_per_chunk < hw <= nchunks * pix_per_chunk
    pad = nchunks * pix_per_chunk - hw
    xp = torch.cat([x, x.new_zeros(B, pad, C)], 1) if pad else x  # (zeros add nothing to a sum or to its bound)
    v = xp.reshape(B, nchunks, pix_per_chunk, groups, cpg).permute(0, 1, 3, 2, 4).reshape(B, nchunks, groups, -1)
    npix = torch.full((nchunks, 1), pix_per_chunk, dtype=F64, device=x.device)
    npix[-1] = pix_per_chunk - pad
    (s, ds), (q, dq) = LR.sum_refs(v, npix * cpg, -1)
    return torch.stack([s, q], -1), torch.stack([ds, dq], -1)


def partial_refs(x, nblk):
    """x [B, hw, c] fp64 -> (ref, bound) [B, nblk, 2, c]: per-(row block, channel) sums as a producer's epilogue leaves
    them (hw / nblk rows each), sum_refs' rule with n = rows."""
    B, hw, c = x.shape
    rows = hw // nblk
    assert rows * nblk == hw
    (s, ds), (q, dq) = LR.sum_refs(x.reshape(B, nblk, rows, c), rows, 2)
    return torch.stack([s, q], 2), torch.stack([ds, dq], 2)


def make_partials(x16, nblk, ld, pad=float("nan")):
    """fp32 [B, nblk, 2, ld] partials of fp16 x [B, hw, c], on x's device: fp32 sums of the fp16 values (squares of fp16
    values are exact in fp32); columns >= c hold `pad`."""
    B, hw, c = x16.shape
    xf = x16.float().view(B, nblk, hw // nblk, c)
    out = torch.full((B, nblk, 2, ld), pad, dtype=torch.float32, device=x16.device)
    out[..., 0, :c] = xf.sum(2)
    out[..., 1, :c] = (xf * xf).sum(2)
    return out


def fold_refs(x, nblk, groups):
    """x [B, hw, c] fp64 -> (ref, bound) [B, groups, 2] of chunk 0 of upk_groupnorm_finalize_f32's workspace when the
    partials are within partial_refs' bounds: their errors add up, the fp64 fold rounds once to fp32."""
    B, hw, c = x.shape
    ref, bnd = partial_refs(x, nblk)
    grp = lambda t: t.reshape(B, nblk, 2, groups, c // groups).sum((1, 4)).transpose(1, 2)
    return grp(ref), grp(bnd) + E32H * grp(ref.abs())


def totals(part, groups, keep=None, swap=False):
    """fp64 per-group totals [B, groups, 2] of mode-2 partials [B, nblk, 2, >= c] (the first c = groups * cpg columns of
    `part` are used; pass part[..., :c]).  keep: the row blocks that are summed; swap: the two planes exchanged."""
    B, nblk, _, c = part.shape
    p = part.to(F64)
    if keep is not None:
        p = p[:, keep]
    if swap:
        p = p.flip(2)
    return p.reshape(B, -1, 2, groups, c // groups).sum((1, 4)).transpose(1, 2)


def apply_from_totals(x, tot, groups, gamma, beta, eps, silu, stat_roll=0, param_roll=0):
    """y [B, hw, C] (fp64) from per-group totals [B, groups, 2]: the normalisation both GroupNorm forms finish with.
    stat_roll: group g takes the statistics of group g + stat_roll; param_roll: channel c takes gamma / beta of c + roll."""
    B, hw, C = x.shape
    cpg = C // groups
    n = float(hw * cpg)
    mean = tot[..., 0] / n
    var = (tot[..., 1] / n - mean * mean).clamp(min=0)
    rstd = 1 / torch.sqrt(var + eps)
    if stat_roll:
        mean, rstd = mean.roll(-stat_roll, 1), rstd.roll(-stat_roll, 1)
    gamma, beta = gamma.roll(-param_roll), beta.roll(-param_roll)
    ex = lambda t: t.repeat_interleave(cpg, 1).unsqueeze(1)
    y = (x - ex(mean)) * ex(rstd) * gamma + beta
    return y * torch.sigmoid(y) if silu else y


def group_totals(x, groups, c_only=None):
    """[B, groups, 2] totals of x [B, hw, C] (fp64).  c_only = (g, c1): group g is summed over its channels < c1 only
    (a seam-straddling group that is given the channels of the first source)."""
    if c_only is not None:
        g, c1 = c_only
        cpg = x.shape[-1] // groups
        x = x.clone()
        x[..., c1:(g + 1) * cpg] = 0
    return pixel_sums(x, slice(None), groups)


def layernorm_mutant(x, gamma, beta, eps, drop_last_vector=False, padded_count=False):
    """fp64 LayerNorm with a near miss: the last 8 values left out of the mean, or 1 / d taken over the padded lane slots."""
    rows, d = x.shape
    nv = d // 8
    vpl = 1 if nv <= 64 else 2 if nv <= 128 else 4
    dd = 8.0 * 64 * vpl if padded_count else float(d)
    xs = x[:, :d - 8] if drop_last_vector else x
    mean = xs.sum(-1, keepdim=True) / dd
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / dd
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


# ---------------------------------------------------------------------------------------------------------------------
# fp32 in the kernels' order (the compiler contracts a * b + c: the fused form is taken in fp64 and rounded once, which
# is exact for the squares of fp16 values added to an fp32 sum)
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _seq_sum(v):
    """fp32 sum over the LAST dim, left to right."""
    acc = torch.zeros_like(v[..., 0])
    for i in range(v.shape[-1]):
        acc = acc + v[..., i]
    return acc


def emu_stats(x16, groups, nchunks, ppc):
    """gn_stats_kernel: fp32 [B, nchunks, groups, 2].  Thread (r, v) adds the pixels p0 + r, + rpi, ... of its 8
    channels; 4 threads per (group, quantity) add the (row slot, channel) pairs e = sub, sub + 4, ...; then (0 + 1) + (2 + 3)."""
    B, hw, C = x16.shape
    _, rpi = stats_geometry(C)
    cpg = C // groups
    T = -(-ppc // rpi)
    off = torch.arange(T)[None, :, None] * rpi + torch.arange(rpi)[None, None, :]
    p = torch.arange(nchunks)[:, None, None] * ppc + off
    ok = (off < ppc) & (p < hw)
    xs = x16.float()[:, p.clamp(max=hw - 1)] * ok[None, ..., None]  # [B, nchunks, T, rpi, C]
    s = torch.zeros(B, nchunks, rpi, C)
    ss = torch.zeros(B, nchunks, rpi, C)
    for t in range(T):
        f = xs[:, :, t]
        s = s + f
        ss = _fma32(f, f, ss)
    sc = torch.stack([s, ss], -1).reshape(B, nchunks, rpi, groups, cpg, 2).permute(0, 1, 3, 5, 2, 4)
    sc = sc.reshape(B, nchunks, groups, 2, rpi * cpg)
    n4 = -(-rpi * cpg // 4)
    sc = torch.cat([sc, sc.new_zeros(*sc.shape[:-1], n4 * 4 - rpi * cpg)], -1).reshape(B, nchunks, groups, 2, n4, 4)
    t = _seq_sum(sc.transpose(-1, -2))  # [.., 4]
    return (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])


def emu_partial_totals(parts, cs, groups):
    """gn_apply_kernel, mode 2: per channel an fp32 sum over the row blocks in order, then fp64 over a group's channels.
    parts / cs: one [B, nblk, 2, ld] fp32 tensor and channel count per source."""
    chs = torch.cat([_seq_sum(p[..., :c].permute(0, 2, 3, 1)) for p, c in zip(parts, cs)], -1)  # [B, 2, C]
    B, _, C = chs.shape
    return chs.double().reshape(B, 2, groups, C // groups).sum(-1).transpose(1, 2)


def emu_apply(x16, tot, groups, gamma, beta, eps, silu):
    """The tail of gn_apply_kernel / gn_onepass_kernel from fp64 per-group totals [B, groups, 2]: mean / variance in fp64,
    scale = rstd gamma and shift = beta - mean scale in fp32, y = x scale + shift, SiLU, fp16."""
    B, hw, C = x16.shape
    cpg = C // groups
    n = float(hw * cpg)
    mean = tot[..., 0] / n
    var = (tot[..., 1] / n - mean * mean).clamp(min=0)
    fmean, frstd = mean.float(), (1 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    ex = lambda t: t.repeat_interleave(cpg, 1).unsqueeze(1)
    sc = ex(frstd) * gamma.float()
    f = _fma32(x16.float(), sc, _fma32(-ex(fmean), sc, beta.float()))
    if silu:
        f = f * (1 / (1 + torch.exp(-f)))
    return f.half()


def emu_onepass_totals(x16, groups, V):
    """gn_onepass_kernel<V, NV>: thread tid owns the vectors tid + 256 k of its (sample, group), adds their values in
    fp32 in the order (k, j); the 256 threads are then added in fp64."""
    B, hw, C = x16.shape
    cpg = C // groups
    xg = x16.float().reshape(B, hw, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, hw * cpg)
    nv = -(-(hw * cpg // V) // 256)
    xg = torch.cat([xg, xg.new_zeros(B, groups, nv * 256 * V - hw * cpg)], -1)
    th = xg.reshape(B, groups, nv, 256, V).permute(0, 1, 3, 2, 4).reshape(B, groups, 256, nv * V)
    s = torch.zeros(B, groups, 256)
    ss = torch.zeros(B, groups, 256)
    for i in range(nv * V):
        f = th[..., i]
        s = s + f
        ss = _fma32(f, f, ss)
    return torch.stack([s.double().sum(-1), ss.double().sum(-1)], -1)


def _butterfly(v):
    """__shfl_xor sums over 64 lanes (last dim), offsets 32 .. 1, fp32."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., :1]


def emu_layernorm(x16, gamma, beta, eps):
    """layernorm_kernel<VPL>: lane l owns the vectors l + 64 i; fp32 throughout."""
    rows, d = x16.shape
    nv = d // 8
    vpl = 1 if nv <= 64 else 2 if nv <= 128 else 4
    x = x16.float()
    xp = torch.cat([x, x.new_zeros(rows, vpl * 512 - d)], -1).reshape(rows, vpl, 64, 8).permute(0, 2, 1, 3)
    on = (torch.arange(vpl * 512) < d).reshape(vpl, 64, 8).permute(1, 0, 2).reshape(64, vpl * 8)
    xl = xp.reshape(rows, 64, vpl * 8)
    mean = _butterfly(_seq_sum(xl)) / torch.tensor(float(d))
    q = torch.zeros(rows, 64)
    for i in range(vpl * 8):
        f = (xl[..., i] - mean) * on[:, i]
        q = _fma32(f, f, q)
    rstd = torch.rsqrt(_butterfly(q) / torch.tensor(float(d)) + torch.tensor(eps))
    return _fma32((x - mean) * rstd, gamma.float(), beta.float()).half()
