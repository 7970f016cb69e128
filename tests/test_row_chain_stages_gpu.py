"""Every compiled instantiation of the three row-chain kernels (range_ref.ROW_CHAIN: upk_cross_block_f16,
upk_head_block_f16, upk_geglu_mlp_f16), one stage at a time.  Their intermediates never leave the CU, so each stage is made
the only inexact one by operands that make the others exact (range_ref.cross_probe / head_probe / mlp_probe), and the output
is held to that stage's own fp64 bound: ``range_ref.ratio(got, ref, bound) <= 1`` over every element, printed per case.
Then properties that need no bound (sample swap, key padding, padded head columns, guard regions, determinism), the
closure of the table over the upk_*_supported functions, and the census of the UNet plans.

Every launch writes into buffers with leading dimension width + 8 (V^T: hw + 32) that hold a sentinel bit pattern, one
guard row in front and one behind, and is checked to have left everything it does not own alone.
tests/test_row_chain_stages_host.py shows that the criterion passes a faithful emulation and fails on seeded defects."""
import ctypes as C
import functools
import re

import pytest
import torch

import range_ref as R
from test_dynamic_range_gpu import report
from test_ops_gpu import geglu_row_map
from test_production_launches_gpu import model, unet_plan  # noqa: F401  (model: the fixture)
from test_xblock_gpu import head_cols
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = 0x5BD5  # fp16 bit pattern (251.6): what every output buffer holds before a launch
KEYS = 96          # context keys the cross block covers; vt_ld of its context
IDS = [R.row_chain_id(r) for r in R.ROW_CHAIN]
TABLE = {R.row_chain_key(r) for r in R.ROW_CHAIN}
LAUNCHED = set()   # table keys the stage tests launched (the closure test at the end checks it)


# ---------------------------------------------------------------------------------------------------------------------
# guarded outputs
def guarded(rows, width, extra=8):
    """A [rows + 2, width + extra] sentinel buffer and the [rows, width] part in its middle a launch owns."""
    buf = torch.full((rows + 2, width + extra), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
    return buf, buf[1:rows + 1, :width]


def assert_guards(what, *pairs):
    """Every element outside the owned part still holds the sentinel, bit for bit."""
    for buf, own in pairs:
        t = buf.clone().view(torch.int16)
        t[1:own.shape[0] + 1, :own.shape[1]] = SENTINEL
        assert bool((t == SENTINEL).all()), "%s: wrote outside the rows / columns it owns" % what


def to_dev(o, *names):
    return [o[n].to(DEV) for n in names]


def vec256(*parts):
    v = torch.cat(parts)
    return torch.cat([v, v.new_zeros(-v.numel() % 256)]).contiguous()


def finite_fill(shape, seed):
    """Finite fp16 values up to +-6e4."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 3e4).clamp(-6e4, 6e4).half().to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# launches
def launch_cross(ctx, o, rows, pad_fill=False):
    """One upk_cross_block_f16 launch on cross_case's operands; y [M, c] on the CPU.  pad_fill: rows >= n_kv of the last
    sample's k_ctx and columns [n_kv, 96) of vt_ctx hold finite values up to +-6e4 instead of zeros."""
    B, hw, c, nkv, heads, dh, dp = (o[k] for k in ("B", "hw", "c", "nkv", "heads", "dh", "dp"))
    M, hd = B * hw, heads * dp
    t0, wo1, bo1, gamma, beta, wq, wo2, bo2 = to_dev(o, "t0", "wo1", "bo1", "gamma", "beta", "wq", "wo2", "bo2")
    cols = head_cols(heads, dh, dp).to(DEV)
    real = cols >= 0

    def padded(x):
        out = torch.zeros(*x.shape[:-1], hd, device=DEV, dtype=torch.float16)
        out[..., real] = x.to(DEV)
        return out

    a1 = padded(o["a1"])
    kc = torch.zeros(B * nkv + KEYS, hd, device=DEV, dtype=torch.float16)
    vt = torch.zeros(B, heads, dp, KEYS, device=DEV, dtype=torch.float16)
    if pad_fill:
        kc[B * nkv:] = finite_fill((KEYS, hd), 71)
        vt[..., nkv:] = finite_fill((B, heads, dp, KEYS - nkv), 72)
    kc[:B * nkv] = padded(o["k"]).reshape(B * nkv, hd)
    vt[:, :, :dh, :nkv] = o["v"].to(DEV).reshape(B, nkv, heads, dh).permute(0, 2, 3, 1)
    wqf = (wq * gamma[None, :]).half().float()
    w1p, n1 = ctx.pack_weight(wo1.contiguous(), col_map=cols)
    w3p, n3 = ctx.pack_weight(wo2.contiguous(), col_map=cols)
    wqp, nq = ctx.pack_weight((wq * gamma[None, :]).contiguous(), row_map=cols)
    assert n1 == c and n3 == c and nq == hd
    uq = torch.zeros(hd, device=DEV); uq[real] = wqf.sum(dim=1)
    bq = torch.zeros(hd, device=DEV); bq[real] = wq @ beta
    vec = vec256(bo1, uq, bq, bo2)
    ybuf, y = guarded(M, c)
    d = L.XblockDesc()
    d.a1, d.lda, d.m, d.c, d.heads, d.d = a1.data_ptr(), hd, M, c, heads, dp
    d.t0, d.ld_t0 = t0.data_ptr(), c
    d.w_out1, d.w_q, d.w_out2, d.vec = w1p.data_ptr(), wqp.data_ptr(), w3p.data_ptr(), vec.data_ptr()
    d.ln_eps, d.ln_dim = o["eps"], c
    d.k_ctx, d.ldk, d.n_kv = kc.data_ptr(), hd, nkv
    d.vt_ctx, d.vt_ld, d.scale = vt.data_ptr(), KEYS, o["scale"]
    d.y, d.ldy, d.hw, d.rows_per_wg = y.data_ptr(), ybuf.shape[1], hw, rows
    assert ctx.lib.upk_cross_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_cross_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    assert_guards("cross block rows %d" % rows, (ybuf, y))
    return y.cpu()


def launch_head(ctx, o, rows):
    """One upk_head_block_f16 launch on head_case's operands (with o["gn_part"]: the GroupNorm fold); (t0 [M, c],
    q | k [M, 2 inner], v [M, inner]) on the CPU, the padded head columns checked to be zero and taken out."""
    B, hw, c, heads, dh, dp = (o[k] for k in ("B", "hw", "c", "heads", "dh", "dp"))
    M, hd, inner = B * hw, heads * dp, heads * dh
    x, wi, bi, gamma, beta, wqkv = to_dev(o, "x", "wi", "bi", "gamma", "beta", "wqkv")
    cols = head_cols(heads, dh, dp).to(DEV)
    rows3 = torch.cat([torch.where(cols >= 0, cols + i * inner, cols) for i in range(3)]).to(torch.int32)
    real3 = rows3 >= 0
    wf = (wqkv * gamma[None, :]).half().float()
    w1p, n1 = ctx.pack_weight(wi.contiguous())
    w2p, n2 = ctx.pack_weight((wqkv * gamma[None, :]).contiguous(), row_map=rows3)
    assert n1 == c and n2 == 3 * hd
    u2 = torch.zeros(3 * hd, device=DEV); u2[real3] = wf.sum(dim=1)
    b2 = torch.zeros(3 * hd, device=DEV); b2[real3] = wqkv @ beta
    vec = vec256(bi, u2, b2)
    t0buf, t0 = guarded(M, c)
    qkbuf, qk = guarded(M, 2 * hd)
    vtbuf, vt = guarded(B * heads * dp, hw, extra=32)
    d = L.HblockDesc()
    d.x, d.ldx, d.m, d.c, d.heads, d.d = x.data_ptr(), c, M, c, heads, dp
    d.w_in, d.w_qkv, d.vec, d.ln_eps, d.ln_dim = w1p.data_ptr(), w2p.data_ptr(), vec.data_ptr(), o["eps"], c
    d.t0, d.ld_t0, d.qk, d.ld_qk = t0.data_ptr(), t0buf.shape[1], qk.data_ptr(), qkbuf.shape[1]
    d.vt, d.vt_ld, d.hw, d.rows_per_wg = vt.data_ptr(), vtbuf.shape[1], hw, rows
    keep = None
    if "gn_part" in o:
        keep = part, gg, gb = to_dev(o, "gn_part", "gn_gamma", "gn_beta")
        assert part.is_contiguous()
        d.gn_part, d.gn_gamma, d.gn_beta = part.data_ptr(), gg.data_ptr(), gb.data_ptr()
        d.gn_nblk, d.gn_ld, d.gn_groups, d.gn_eps = o["gn_nblk"], part.shape[-1], o["gn_groups"], o["gn_eps"]
    assert ctx.lib.upk_head_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_head_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    del keep
    what = "head block rows %d" % rows
    assert_guards(what, (t0buf, t0), (qkbuf, qk), (vtbuf, vt))
    real = (cols >= 0).cpu()
    qk_c, vt_c = qk.cpu().view(M, 2, hd), vt.cpu().view(B, heads, dp, hw)
    # columns dh..dp-1 of each head in q | k, and those rows of V^T, are exactly 0: the self-attention reads them
    assert not qk_c[:, :, ~real].any() and not vt_c[:, :, dh:].any(), what + ": the padded head columns are not zero"
    got_v = vt_c.permute(0, 3, 1, 2).reshape(M, hd)[:, real]
    return t0.cpu(), qk_c[:, :, real].reshape(M, 2 * inner), got_v


def launch_mlp(ctx, o, rows_per_wg):
    """One upk_geglu_mlp_f16 launch on mlp_case's operands; (y [M, c], partials [B, nblk, 2, n_pad] or None) on the CPU."""
    M, hw, c, inner = o["M"], o["hw"], o["c"], o["inner"]
    rows = rows_per_wg & ~L.MLP_STREAM
    x, res, gamma, beta, w1, b1, w2h, w2x, b2 = to_dev(o, "x", "res", "gamma", "beta", "w1", "b1", "w2h", "w2x", "b2")
    rm = geglu_row_map(inner).to(DEV)
    w1p, _ = ctx.pack_weight((w1 * gamma[None, :]).contiguous(), row_map=rm)
    b1p = (b1 + w1 @ beta)[rm.long()].contiguous()
    u1p = (w1 * gamma[None, :]).half().float().sum(dim=1)[rm.long()].contiguous()
    w2a, n_pad = ctx.pack_weight(w2h.contiguous())
    w2b, _ = ctx.pack_weight(w2x.contiguous())
    w2p = torch.cat([w2a.reshape(-1), w2b.reshape(-1)]).contiguous()
    b2p = torch.zeros(n_pad, device=DEV); b2p[:c] = b2
    ybuf, y = guarded(M, c)
    d = L.MlpDesc()
    d.x, d.ldx, d.m, d.c, d.inner = x.data_ptr(), c, M, c, inner
    d.w1, d.b1, d.u1, d.ln_eps, d.ln_dim = w1p.data_ptr(), b1p.data_ptr(), u1p.data_ptr(), o["eps"], c
    d.w2, d.b2, d.n_out, d.n_pad = w2p.data_ptr(), b2p.data_ptr(), c, n_pad
    d.residual, d.ld_res, d.y, d.ldy = res.data_ptr(), c, y.data_ptr(), ybuf.shape[1]
    d.rows_per_wg, d.hw = rows_per_wg, hw
    sws = None
    if hw:
        B, nblk = M // hw, hw // rows
        sws = torch.full((ctx.gn_stats_floats(B, n_pad),), float("nan"), device=DEV)
        d.gn_stats_ws = sws.data_ptr()
    assert ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_geglu_mlp_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    what = "mlp rows_per_wg %#x" % rows_per_wg
    assert_guards(what, (ybuf, y))
    if not hw:
        return y.cpu(), None
    used = B * nblk * 2 * n_pad
    assert bool(torch.isnan(sws[used:]).all()), what + ": wrote past its GroupNorm partials"
    return y.cpu(), sws[:used].reshape(B, nblk, 2, n_pad).cpu()


# ---------------------------------------------------------------------------------------------------------------------
# references, computed once per (probe, shape, scale) and shared by the instantiations (treat as read-only)
@functools.lru_cache(maxsize=None)
def cross_ref(probe, s, B, hw, nkv, c, dh, dp, ks=1):
    o = R.cross_probe(probe, s, B, hw, nkv, c, dh, dp, ks)
    ref, bound = R.cross_probe_ref(o)
    assert float(ref.abs().max()) < 6e4
    return o, ref, bound


@functools.lru_cache(maxsize=None)
def head_ref(probe, s, B, hw):
    o = R.head_probe(probe, s, B, hw)
    (t0, dt0), (qkv, dqkv) = R.head_probe_ref(o)
    assert float(t0.abs().max()) < 6e4 and float(qkv.abs().max()) < 6e4
    return o, (t0, dt0), (qkv, dqkv)


@functools.lru_cache(maxsize=None)
def mlp_hidden(s, B, hw, M):
    return R.mlp_hidden_ref(R.mlp_probe("M3", s, B, hw, 32, M=M if not hw else None))


@functools.lru_cache(maxsize=None)
def mlp_ref(probe, s, B, hw, M):
    o = R.mlp_probe(probe, s, B, hw, 32, M=M if not hw else None)
    ref, bound = R.mlp_probe_ref(o, mlp_hidden(s, B, hw, M) if probe.startswith("M2") else None)
    assert float(ref.abs().max()) < 6e4
    return o, ref, bound


class Peaks(dict):
    def add(self, probe, r):
        self[probe] = max(self.get(probe, 0.0), r)
        return r

    def line(self):
        return "  ".join("%s %.3f" % kv for kv in sorted(self.items()))


# ---------------------------------------------------------------------------------------------------------------------
# the stages
def cross_stages(ctx, row):
    c, dp, dh, rows = row["c"], row["d"], row["dh"], row["rows"]
    top = Peaks()
    for B, hw, _ in R.row_chain_shapes(row):
        def run(probe, s, nkv, ks=1):
            o, ref, bound = cross_ref(probe, s, B, hw, nkv, c, dh, dp, ks)
            y = launch_cross(ctx, o, rows)
            r = top.add(probe, R.ratio(y, ref, bound))
            assert report("%s %s B%d hw%d nkv%d ks%d" % (R.row_chain_id(row), probe, B, hw, nkv, ks), s, r) <= 1
            if probe == "X2" and nkv == 1:  # a single key: the sample's value row + t0, under the same bound
                v = o["v"].to(F64).reshape(B, 1, c).expand(B, hw, c).reshape(B * hw, c)
                assert R.ratio(y, v + o["t0"].to(F64), bound) <= 1

        for s in R.STAGE_SCALES:
            run("X1", s, 87)
            run("X3", s, 87)
            for nkv in R.X2_NKV:
                for ks in R.X2_KEY_SCALES:
                    run("X2", s, nkv, ks)  # (n_kv = 1: the reference is V's row + t0, as the host test asserts)
        for s in R.SCALES:
            run("X4", s, 87)
    return top


def head_stages(ctx, row):
    rows, inner = row["rows"], R.HEADS * row["dh"]
    top = Peaks()
    probes = (("F1", R.SCALES), ("F2", R.STAGE_SCALES)) if row["gn"] else (("H1", R.SCALES), ("H2", R.STAGE_SCALES))
    for B, hw, _ in R.row_chain_shapes(row):
        for probe, scales in probes:
            for s in scales:
                o, (t0, dt0), (qkv, dqkv) = head_ref(probe, s, B, hw)
                got_t0, got_qk, got_v = launch_head(ctx, o, rows)
                tag = "%s %s B%d hw%d" % (R.row_chain_id(row), probe, B, hw)
                if dt0 is None:
                    assert torch.equal(got_t0, o["x"]), tag + ": t0 is not x bit for bit"
                else:
                    assert report(tag + " t0", s, top.add(probe + " t0", R.ratio(got_t0, t0, dt0))) <= 1
                r = R.ratio(got_qk, qkv[:, :2 * inner], dqkv[:, :2 * inner])
                assert report(tag + " q | k", s, top.add(probe + " q|k", r)) <= 1
                r = R.ratio(got_v, qkv[:, 2 * inner:], dqkv[:, 2 * inner:])
                assert report(tag + " v", s, top.add(probe + " v", r)) <= 1
    return top


def check_partials(y, part, rows, hw, c):
    """check_mlp_tail's rule: per (row block, channel) fp32 sums of the kernel's OWN fp16 output, rows terms each."""
    B, nblk = y.shape[0] // hw, hw // rows
    part, yb = part.to(F64), y.to(F64).reshape(B, nblk, rows, c)
    r1 = R.ratio(part[:, :, 0, :c], yb.sum(2), rows * R.E32H * yb.abs().sum(2))
    r2 = R.ratio(part[:, :, 1, :c], (yb * yb).sum(2), (rows + 1) * R.E32H * (yb * yb).sum(2))
    return max(r1, r2)


def mlp_stages(ctx, row):
    rows, rpw, c = row["rows"], R.mlp_rows_per_wg(row), row["c"]
    top = Peaks()
    for B, hw, M in R.row_chain_shapes(row):
        for probe, scales in [("M1", R.STAGE_SCALES), ("M3", R.SCALES)] + [("M2%d" % j, R.STAGE_SCALES) for j in range(4)]:
            for s in scales:
                o, ref, bound = mlp_ref(probe, s, B, hw, M)
                y, part = launch_mlp(ctx, o, rpw)
                tag = "%s %s M%d hw%d" % (R.row_chain_id(row), probe, M, hw)
                assert report(tag, s, top.add(probe, R.ratio(y, ref, bound))) <= 1
                if hw:
                    r = top.add("partials", check_partials(y, part, rows, hw, c))
                    assert report(tag + " GroupNorm partials", s, r) <= 1
    return top


STAGES = {"xblock": cross_stages, "hblock": head_stages, "mlp": mlp_stages}


@pytest.mark.parametrize("row", R.ROW_CHAIN, ids=IDS)
def test_each_stage_against_its_own_fp64_bound(ctx, row):
    top = STAGES[row["kind"]](ctx, row)
    LAUNCHED.add(R.row_chain_key(row))
    print("stages %-22s max err/bound: %s" % (R.row_chain_id(row), top.line()))


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
def swap_samples(o, rows_of, per_sample):
    """The two samples exchanged: the row halves of the [2 hw, .] operands and the leading index of the per-sample ones."""
    n = dict(o)
    for k in rows_of:
        n[k] = torch.cat([o[k][o[k].shape[0] // 2:], o[k][:o[k].shape[0] // 2]])
    for k in per_sample:
        n[k] = o[k].flip(0)
    return n


def halves_swapped(t):
    return torch.cat([t[t.shape[0] // 2:], t[:t.shape[0] // 2]])


@pytest.mark.parametrize("row", R.ROW_CHAIN, ids=IDS)
def test_exact_properties(ctx, row):
    """Bit for bit, at both two-sample shapes: two runs agree; exchanging the samples' rows (and contexts, partials)
    exchanges the outputs (hw is a multiple of the tile height, so every row keeps its place in its tile); the cross block
    ignores k_ctx rows >= n_kv and multiplies the V^T columns [n_kv, 96) by weights that are exactly 0.  The guard regions
    and the padded head columns are checked inside every launch of this file."""
    kind, rows = row["kind"], row["rows"]
    for B, hw, M in R.row_chain_shapes(row):
        if B != 2:  # the MLP's tail tile: one sample, nothing to exchange
            o, _, _ = mlp_ref("M3", 1, B, hw, M)
            assert torch.equal(launch_mlp(ctx, o, R.mlp_rows_per_wg(row))[0], launch_mlp(ctx, o, R.mlp_rows_per_wg(row))[0])
            continue
        if kind == "xblock":
            for nkv in (80, 87):
                o, _, _ = cross_ref("X4", 1, B, hw, nkv, row["c"], row["dh"], row["d"])
                y = launch_cross(ctx, o, rows)
                assert torch.equal(y, launch_cross(ctx, o, rows)), "two runs differ"
                ys = launch_cross(ctx, swap_samples(o, ("a1", "t0"), ("k", "v")), rows)
                assert torch.equal(ys, halves_swapped(y)), "sample swap"
                assert torch.equal(launch_cross(ctx, o, rows, pad_fill=True), y), "key padding (n_kv %d)" % nkv
        elif kind == "hblock":
            o, _, _ = head_ref("F1" if row["gn"] else "H1", 1, B, hw)
            out = launch_head(ctx, o, rows)
            again = launch_head(ctx, o, rows)
            swapped = launch_head(ctx, swap_samples(o, ("x",), ("gn_part",) if row["gn"] else ()), rows)
            for u, v, w in zip(out, again, swapped):
                assert torch.equal(u, v), "two runs differ"
                assert torch.equal(w, halves_swapped(u)), "sample swap"
        else:
            o, _, _ = mlp_ref("M3", 1, B, hw, M)
            rpw = R.mlp_rows_per_wg(row)
            y, part = launch_mlp(ctx, o, rpw)
            y2, part2 = launch_mlp(ctx, o, rpw)
            assert torch.equal(y, y2) and torch.equal(part, part2), "two runs differ"
            ys, parts = launch_mlp(ctx, swap_samples(o, ("x", "res"), ()), rpw)
            assert torch.equal(ys, halves_swapped(y)) and torch.equal(parts, part.flip(0)), "sample swap"


# ---------------------------------------------------------------------------------------------------------------------
# closure and census
def supported_sweep(ctx):
    """What the three upk_*_supported functions accept (nothing is enqueued), as table keys; rows 0 = the default."""
    got = set()
    hw, m = 256, 512
    for c in (224, 448, 672, 896):
        for dp in (32, 64, 128):
            for rows in (0, 16, 32, 64, 128, 256):
                x = L.XblockDesc()
                x.m, x.c, x.heads, x.d, x.hw, x.rows_per_wg, x.n_kv, x.vt_ld = m, c, R.HEADS, dp, hw, rows, 87, KEYS
                x.lda, x.ld_t0, x.ldy, x.ldk = R.HEADS * dp, c, c, R.HEADS * dp
                if ctx.lib.upk_cross_block_supported(ctx.h, C.byref(x)):
                    got.add(("xblock", c, dp, rows or R.ROW_CHAIN_DEFAULT_ROWS["xblock"], False, False))
                h = L.HblockDesc()
                h.m, h.c, h.heads, h.d, h.hw, h.rows_per_wg = m, c, R.HEADS, dp, hw, rows
                h.ldx, h.ld_t0, h.ld_qk, h.vt_ld = c, c, 2 * R.HEADS * dp, hw
                if ctx.lib.upk_head_block_supported(ctx.h, C.byref(h)):
                    for gn in (False, True):  # (the fold is chosen by gn_part alone: every accepted shape has both forms)
                        got.add(("hblock", c, dp, rows or R.ROW_CHAIN_DEFAULT_ROWS["hblock"], False, gn))
        for rows in (0, 16, 32, 64, 128, 256):
            for flag in (0, L.MLP_STREAM):
                d = L.MlpDesc()
                d.m, d.c, d.inner, d.n_out, d.n_pad, d.hw, d.rows_per_wg = m, c, 4 * c, c, c, hw, rows | flag
                d.ldx, d.ld_res, d.ldy, d.ln_dim = c, c, c, c
                if ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(d)):
                    r = rows or R.ROW_CHAIN_DEFAULT_ROWS["mlp"]
                    got.add(("mlp", c, 0, r, bool(flag) or r == 128, False))
    return got


def test_the_table_is_what_the_kernels_accept(ctx):
    """A new instantiation fails here until range_ref.ROW_CHAIN lists it (and the stage tests run it)."""
    assert L.MLP_STREAM == R.MLP_STREAM
    got = supported_sweep(ctx)
    assert got == TABLE, (sorted(got - TABLE), sorted(TABLE - got))


LABEL = re.compile(r"^(hblock|xblock|mlp) M(\d+) C(\d+)(?: d(\d+))? rows(\d+)(s?)( gn)?$")


@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_census_of_the_unet_plans(ctx, model, H, W, lanes):  # noqa: F811
    """Every row-chain launch of the plans the benchmark replays is a row of the table."""
    plan = unet_plan(model, H, W, lanes)
    seen = {}
    for lab in plan.body.labels:
        if lab.split(" ")[0] not in ("hblock", "xblock", "mlp"):
            continue
        m = LABEL.match(lab)
        assert m, "unparsed row-chain label %r" % lab
        kind, _, c, dp, rows, st, gn = m.groups()
        # (a head labelled "gn" takes the fold when its producer left channel partials, else the plain form)
        for g in ((False, True) if gn else (False,)):
            key = (kind, int(c), int(dp or 0), int(rows), bool(st), g)
            seen[key] = seen.get(key, 0) + 1
    # (the 32x24 latent on its own leaves the head unfused: M / 32 workgroups would not cover the chip)
    assert {"xblock", "mlp"} <= {k[0] for k in seen}, sorted(seen)
    assert (H, W) != (32, 32) or "hblock" in {k[0] for k in seen}, sorted(seen)
    print("\nUNet %dx%d %s: %s" % (H, W, "shared_chip(4)" if lanes > 1 else "single forward",
                                  ", ".join("%s x%d" % (k, n) for k, n in sorted(seen.items()))))
    assert set(seen) <= TABLE, sorted(set(seen) - TABLE)


def test_every_table_row_was_launched():
    """Runs last: the stage tests above launched every row of the table (a row added to it must be run by them)."""
    assert LAUNCHED == TABLE, sorted(TABLE - LAUNCHED)
