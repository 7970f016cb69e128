"""A descriptor-driven fp64 reference of one upk_conv2d_nhwc_f16 launch: the fields of a upk_conv_desc (include/upk.h) and
the operands, which the caller owns, in; ``(ref, bound)`` for everything the launch writes out.

It is built on tests/range_ref.py (``im2col``, ``linear_ref``, ``phase_weights``, ``groupnorm_ref``) and adds no tolerance
of its own: every bound is range_ref's, derived there, with the following few additions (each follows from the same
rules; n e32 sum|v| for an fp32 sum of n values is range_ref's "fp32 accumulation" rule):

* Row statistics the launch reads (``ln_rows_in``).  The caller fills them from the fp16 rows: each slot holds the exactly
  rounded fp32 sum of its share of the row, at most 8 slots are added in fp32.  That is 8 + 1 roundings of at most
  e32 sum|x| each, inside the K e32 mean|x| (K >= 32) linear_ref's folded LayerNorm already allows for statistics taken
  in the kernel, so the same reference serves both forms.
* Sums of stored values (``ln_rows_out``, the GroupNorm partials of modes 1 and 2, upk_groupnorm_finalize_f32).  They are
  checked against the fp16 output the SAME launch stored: a sum of n stored values is off by at most n e32 sum|y|, a
  sum of n squares by (n + 1) e32 sum y^2 (one more rounding for the square; tests/test_dynamic_range_gpu.py uses the
  same rule for the feed-forward tail's partials).
* The normalising reduce pass (mode 3) with ``gno_skip_y``.  y is never stored, so ``gno_y`` is compared with the GroupNorm
  of the REFERENCE output; the kernel normalises its own fp16 values, which are off from the reference by up to the
  output's bound, pushed through the normalisation by groupnorm_ref(dx=...).
* A cost-model launch (tune_cfg == 0) does not tell its split-K factor.  The library only ever picks one of
  {1, 2, 3, 4, 6, 8, 9, 12, 16, 18} (upgpt_amd/csrc/igemm.hip sk_cands), and the seam term of linear_ref grows with the
  factor, so ``SPLITK_MAX`` = 18 bounds every split launch whose factor is not pinned.

The operands are torch tensors on any one device (the reference runs where they live, in fp64, one sample at a time, so
that no im2col matrix of a whole batch exists):

    x1, x2      fp16 [batch, in_h, in_w, ld]    the first c1 / c2 channels are read
    x3, x4      fp16 [batch, Ho, Wo, ld]        the appended 1x1 segment's sources
    w           fp32 [N, c1 + c2, ksize, ksize] NATURAL row order: GEGLU N = 2 n_out as [value rows | gate rows] (the
                                                 packing interleaves them), with a V^T tail N = n_pad, else N = n_out
    w_app       fp32 [N, c3 + c4, 1, 1]
    bias, ln_colsum  fp32 [N], natural order
    rowvec      fp32, flat, indexed step * rv_step_stride + b * rv_batch_stride + n;  step: int
    residual    fp16 [M, ld_res]
    gno_gamma, gno_beta  fp32 [n_out]
"""
import ctypes

import torch

import range_ref as R
from upgpt_amd import _lib as L

F64 = torch.float64
SPLITK_MAX = 18
KNOWN_FLAGS = L.F_SILU | L.F_GEGLU | L.F_OUT_F32 | L.F_OUT_NCHW_F32 | L.F_UPSAMPLE2X | L.F_PAD_ASYM | L.F_QUICKGELU
POINTERS = tuple(n for n, t in L.ConvDesc._fields_ if t is ctypes.c_void_p)
# the fields the reference and the replica builder of tests/test_production_launches_gpu.py treat.  A field that
# upk_conv_desc gains later is reported by unhandled() until it is added here AND to both of them.
HANDLED = frozenset("""x1 x2 c1 c2 ld1 ld2 batch in_h in_w ksize stride w_packed n_out n_pad bias residual ld_res rowvec
    rv_batch_stride rv_step_stride step y ldy vt vt_from vt_heads vt_dhead vt_ld vt_tokens flags tune_cfg tune_splitk
    ln_colsum ln_eps ln_dim gn_stats_ws gn_groups x3 x4 c3 c4 ld3 ld4 gno_gamma gno_beta gno_y gno_eps gno_silu gno_ld
    gno_skip_y ln_rows_out ln_rows_in ln_rows_slots w_phase gn_stats_cap pf_next pf_bytes""".split())


def fields(d=None, **over):
    """Every field of a upk_conv_desc as a dict: sizes, strides, flags and choices as they are, pointers as booleans
    (set or not).  `over`: values to put on top (host tests describe a launch without a device pointer to give)."""
    d = d if d is not None else L.ConvDesc()
    f = {n: (bool(getattr(d, n)) if n in POINTERS else getattr(d, n)) for n, _ in L.ConvDesc._fields_}
    for k, v in over.items():
        if k not in f:
            raise KeyError("upk_conv_desc has no field %r" % k)
        f[k] = v
    return f


def out_dims(f):
    """(Ho, Wo) of the launch, as include/upk.h defines them."""
    H, W = (2 * f["in_h"], 2 * f["in_w"]) if f["flags"] & L.F_UPSAMPLE2X else (f["in_h"], f["in_w"])
    if f["flags"] & L.F_PAD_ASYM:
        return (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    pad = 1 if f["ksize"] == 3 else 0
    return (H + 2 * pad - f["ksize"]) // f["stride"] + 1, (W + 2 * pad - f["ksize"]) // f["stride"] + 1


def phase_form(f):
    """Whether the launch computes nearest-2x -> conv3x3 as four 2x2 convs (include/upk.h w_phase: plain epilogue only,
    bias -> fp16 NHWC / fp32; otherwise w_packed is used)."""
    return bool(f["w_phase"] and f["flags"] & L.F_UPSAMPLE2X and f["ksize"] == 3 and f["stride"] == 1
                and not f["flags"] & (L.F_PAD_ASYM | L.F_GEGLU | L.F_OUT_NCHW_F32 | L.F_SILU | L.F_QUICKGELU)
                and not (f["x3"] or f["ln_colsum"] or f["vt"] or f["residual"] or f["rowvec"]))


def unhandled(f):
    """Names of the fields (or combinations) of a descriptor that launch_ref does not implement; empty = all covered."""
    fl, bad = f["flags"], []
    if set(f) - HANDLED:
        bad += sorted(set(f) - HANDLED)
    if fl & ~KNOWN_FLAGS:
        bad.append("flags (unknown bits %#x)" % (fl & ~KNOWN_FLAGS))
    if f["ksize"] not in (1, 3) or f["stride"] not in (1, 2):
        bad.append("ksize / stride")
    if fl & L.F_PAD_ASYM and (f["stride"] != 2 or f["ksize"] != 3 or fl & L.F_UPSAMPLE2X):
        bad.append("flags (UPK_F_PAD_ASYM outside a 3x3 stride-2 conv)")
    if bool(fl & L.F_SILU) + bool(fl & L.F_QUICKGELU) + bool(fl & L.F_GEGLU) > 1:
        bad.append("flags (two activations)")
    if fl & L.F_OUT_F32 and fl & L.F_OUT_NCHW_F32:
        bad.append("flags (two output formats)")
    if fl & L.F_GEGLU and (f["rowvec"] or f["residual"] or f["vt"] or f["n_pad"] != 2 * f["n_out"]):
        bad.append("flags (UPK_F_GEGLU with rowvec / residual / vt, or n_pad != 2 n_out)")
    if fl & L.F_OUT_NCHW_F32 and f["ldy"] != 0:
        bad.append("ldy (UPK_F_OUT_NCHW_F32 with ldy != 0)")
    if f["vt"] and (f["residual"] or fl & (L.F_OUT_F32 | L.F_OUT_NCHW_F32) or f["n_out"] > f["vt_from"]
                    or f["vt_from"] + f["vt_heads"] * f["vt_dhead"] != f["n_pad"]):
        bad.append("vt (with residual / fp32 output, or a tail that is not [vt_from, n_pad))")
    if f["ln_colsum"] and (f["ln_dim"] != f["c1"] or f["c2"] or f["ksize"] != 1 or f["stride"] != 1 or fl & L.F_UPSAMPLE2X):
        bad.append("ln_dim (folded LayerNorm over fewer channels than c1, or not a single-source 1x1)")
    if f["ln_rows_in"] and not f["ln_colsum"]:
        bad.append("ln_rows_in (without ln_colsum)")
    if f["x3"] and (f["stride"] != 1 or fl & (L.F_UPSAMPLE2X | L.F_PAD_ASYM) or f["ln_colsum"]):
        bad.append("x3 (appended segment on a strided / upsampled / LayerNorm-folded launch)")
    if (f["x4"] and not f["x3"]) or (f["c4"] and not f["x4"]) or (f["c2"] and not f["x2"]):
        bad.append("x2 / x4 (channels without a source)")
    if f["w_phase"] and fl & L.F_UPSAMPLE2X and fl & (L.F_SILU | L.F_QUICKGELU):
        bad.append("w_phase (with an activation)")
    if (f["gn_stats_ws"] or f["gno_y"]) and (f["gn_groups"] <= 0 or f["n_out"] % f["gn_groups"]):
        bad.append("gn_groups")
    if f["gno_y"] and not (f["gno_gamma"] and f["gno_beta"]):
        bad.append("gno_gamma / gno_beta")
    return bad


def _nchw(x, c):
    return x[..., :c].permute(0, 3, 1, 2).to(F64)


def launch_ref(f, ops, splitk=1):
    """{'y': (ref, bound)[, 'vt': (ref, bound)]} of the launch `f` (fields()) on `ops` (module docstring).
    y: [M, n_out] in packed row order (row m = (b, oy, ox)), or [batch, n_out, Ho, Wo] with UPK_F_OUT_NCHW_F32; columns
    at or past n_out are not part of it (the launch leaves them alone).  vt: [M / vt_tokens, vt_heads, vt_dhead,
    vt_tokens].  splitk: the split-K factor of the launch (an upper bound where it is not known)."""
    bad = unhandled(f)
    if bad:
        raise NotImplementedError("launch_ref does not handle: " + "; ".join(bad))
    fl = f["flags"]
    B, ks, n_out = f["batch"], f["ksize"], f["n_out"]
    Ho, Wo = out_dims(f)
    hw = Ho * Wo
    dev = ops["x1"].device
    d = lambda t: t.to(dev, F64)
    w = ops["w"]
    N = w.shape[0]
    geglu = bool(fl & L.F_GEGLU)
    assert N == (2 * n_out if geglu else (f["n_pad"] if f["vt"] else n_out)), (N, n_out, f["n_pad"])
    act = "geglu" if geglu else "silu" if fl & L.F_SILU else "quickgelu" if fl & L.F_QUICKGELU else None
    out = "f32" if fl & (L.F_OUT_F32 | L.F_OUT_NCHW_F32) else "f16"
    phased = phase_form(f)
    if phased:
        Wp = {k: R.wmat(R.q16(d(v))) for k, v in R.phase_weights(w.float().cpu()).items()}
    else:
        Wm = R.wmat(R.q16(d(w)))
        if f["x3"]:
            Wm = torch.cat([Wm, R.wmat(R.q16(d(ops["w_app"])))], -1)
    bias = d(ops["bias"]) if f["bias"] else None
    ln = (f["ln_eps"], d(ops["ln_colsum"])) if f["ln_colsum"] else None
    step = int(ops.get("step") or 0) if f["step"] else 0
    refs, bnds = [], []
    for b in range(B):
        x = _nchw(ops["x1"][b:b + 1], f["c1"])
        if f["x2"]:
            x = torch.cat([x, _nchw(ops["x2"][b:b + 1], f["c2"])], 1)
        rv = None
        if f["rowvec"]:
            o = step * f["rv_step_stride"] + b * f["rv_batch_stride"]
            rv = d(ops["rowvec"].reshape(-1)[o:o + N])
        res = d(ops["residual"][b * hw:(b + 1) * hw, :n_out]) if f["residual"] else None
        if phased:
            r = torch.zeros(Ho, Wo, N, dtype=F64, device=dev)
            bd = torch.zeros_like(r)
            for (py, px), wp in Wp.items():
                A = R.im2col(x, 2, pad=(1 - py, py, 1 - px, px))[0]
                r[py::2, px::2], bd[py::2, px::2] = R.linear_ref(A, wp, bias=bias, out=out, splitk=splitk)
            r, bd = r.reshape(hw, N), bd.reshape(hw, N)
        else:
            A = R.im2col(x, ks, f["stride"], (0, 1, 0, 1) if fl & L.F_PAD_ASYM else None, bool(fl & L.F_UPSAMPLE2X))
            A = A.reshape(hw, -1)
            if f["x3"]:
                segs = [d(ops["x3"][b, ..., :f["c3"]]).reshape(hw, -1)]
                if f["x4"]:
                    segs.append(d(ops["x4"][b, ..., :f["c4"]]).reshape(hw, -1))
                A = torch.cat([A] + segs, -1)
            r, bd = R.linear_ref(A, Wm, bias=bias, rowvec=rv, res=res, act=act, out=out, splitk=splitk, ln=ln)
        refs.append(r)
        bnds.append(bd)
        del A
    ref, bnd = torch.cat(refs), torch.cat(bnds)
    outs = {}
    if fl & L.F_OUT_NCHW_F32:
        nchw = lambda t: t[:, :n_out].reshape(B, Ho, Wo, n_out).permute(0, 3, 1, 2)
        outs["y"] = (nchw(ref), nchw(bnd))
    else:
        outs["y"] = (ref[:, :n_out], bnd[:, :n_out])
    if f["vt"]:
        tok, hd = f["vt_tokens"], f["vt_heads"] * f["vt_dhead"]
        tr = lambda t: t[:, f["vt_from"]:f["vt_from"] + hd].reshape(-1, tok, f["vt_heads"], f["vt_dhead"]).permute(0, 2, 3, 1)
        outs["vt"] = (tr(ref), tr(bnd))
    return outs


def sum_refs(v, n_terms, dim):
    """(sum, bound), (sum of squares, bound) of fp64 `v` over `dim`, for fp32 sums of n_terms stored values."""
    s, a, q = v.sum(dim), v.abs().sum(dim), (v * v).sum(dim)
    return (s, n_terms * R.E32H * a), (q, (n_terms + 1) * R.E32H * q)


def byproduct_refs(f, ops, stored, y, *, gn_mode=0, gn_nblk=0, ln_slots=0, finalize=False):
    """References of what the launch leaves besides y, from `stored` = the fp16 y [M, >= n_out] the same launch wrote
    (with gno_skip_y, where it writes none, from y = launch_ref's (ref, bound)):

      'ln_rows'   [M, 2]                      ln_rows_out, slots summed (ln_slots > 0)
      'gn_part'   [batch, nblk, 2, n_out]     gn_stats_ws mode 2 (per row block and channel)
      'gn_group'  [batch, groups, 2]          gn_stats_ws mode 1, chunks summed; with finalize=True the same sums are what
                                              upk_groupnorm_finalize_f32 leaves in chunk 0 of its workspace
      'gno_y'     [M, n_out]                  mode 3
    """
    B, n_out = f["batch"], f["n_out"]
    Ho, Wo = out_dims(f)
    hw = Ho * Wo
    outs = {}
    if f["gno_y"] and gn_mode == 3 and f["gno_skip_y"]:
        yv, dy = (t.reshape(B, hw, n_out) for t in y)
    else:
        yv, dy = stored[:, :n_out].to(F64).reshape(B, hw, n_out), None
    dev = yv.device
    if ln_slots > 0:
        (s, ds), (q, dq) = sum_refs(yv.reshape(B * hw, n_out), n_out, -1)
        outs["ln_rows"] = (torch.stack([s, q], -1), torch.stack([ds, dq], -1))
    if gn_mode == 2:
        rows = hw // gn_nblk
        (s, ds), (q, dq) = sum_refs(yv.reshape(B, gn_nblk, rows, n_out), rows, 2)
        outs["gn_part"] = (torch.stack([s, q], 2), torch.stack([ds, dq], 2))
    if gn_mode == 1 or (gn_mode == 2 and finalize):
        g = f["gn_groups"]
        cpg = n_out // g
        grp = yv.reshape(B, hw, g, cpg).permute(0, 2, 1, 3).reshape(B, g, hw * cpg)
        (s, ds), (q, dq) = sum_refs(grp, hw * cpg, -1)
        outs["gn_group"] = (torch.stack([s, q], -1), torch.stack([ds, dq], -1))
    if gn_mode == 3:
        r, bd = R.groupnorm_ref(yv, f["gn_groups"], ops["gno_gamma"].to(dev, F64), ops["gno_beta"].to(dev, F64), f["gno_eps"],
                                bool(f["gno_silu"]), dx=dy)
        outs["gno_y"] = (r.reshape(B * hw, n_out), bd.reshape(B * hw, n_out))
    return outs
