"""The 64- and 128-row forms of the row-chain kernels (upgpt_amd/csrc/xblock.hip hblock_kernel / xblock_kernel, include/upk.h
rows_per_wg): the fat workgroups that launches sharing the chip with other batches use.  Same references and bounds as
tests/test_xblock_gpu.py, at the smallest shapes at which a tall tile can still go wrong: one workgroup, two samples (the
sample boundary between workgroups, the per-sample K / V^T bases), and a 32x24 latent (hw = 768: 6 / 12 workgroups)."""
import ctypes as C
import functools
import math

import pytest
import torch

from upgpt_amd import _lib as L
from test_ops_gpu import DEV, check, rnd
from test_xblock_gpu import head_cols

pytestmark = pytest.mark.gpu

HEADS, C_, DH, DP, NKV = 8, 224, 28, 32, 87
HD, INNER = HEADS * DP, HEADS * DH
CASES = [(1, 128, 128), (2, 128, 64), (2, 128, 128), (1, 768, 64), (1, 768, 128)]  # B, hw, rows


def rel_err(got, ref):
    """The measure of test_ops_gpu.check: max |got - ref| over max |ref|."""
    return (got.float() - ref.float()).abs().max().item() / (ref.float().abs().max().item() + 1e-6)


# ---------------------------------------------------------------------------------------------------------- hblock
@functools.lru_cache(maxsize=None)
def hblock_case(ctx, B, hw):
    """Operands and the fp32 reference of test_head_block_vs_torch, computed once per shape."""
    M = B * hw
    x = (rnd(M, C_, seed=1) * 1.3).half()
    wi, bi = rnd(C_, C_, scale=1 / math.sqrt(C_), seed=2), rnd(C_, scale=0.1, seed=3)
    gamma, beta = 1 + 0.2 * rnd(C_, seed=4), 0.1 * rnd(C_, seed=5)
    wqkv = rnd(3 * INNER, C_, scale=1 / math.sqrt(C_), seed=6)
    cols = head_cols(HEADS, DH, DP).to(DEV)
    rows3 = torch.cat([torch.where(cols >= 0, cols + i * INNER, cols) for i in range(3)]).to(torch.int32)
    real3 = rows3 >= 0
    t0 = (x.float() @ wi.half().float().t() + bi).half().float()
    wf = (wqkv * gamma[None, :]).half().float()
    xn = (t0 - t0.mean(1, keepdim=True)) * torch.rsqrt(t0.var(1, unbiased=False, keepdim=True) + 1e-5)
    qkv = xn @ wf.t() + wqkv @ beta
    w1p, n1 = ctx.pack_weight(wi.contiguous())
    w2p, n2 = ctx.pack_weight((wqkv * gamma[None, :]).contiguous(), row_map=rows3)
    assert n1 == C_ and n2 == 3 * HD
    u2 = torch.zeros(3 * HD, device=DEV); u2[real3] = wf.sum(dim=1)
    b2 = torch.zeros(3 * HD, device=DEV); b2[real3] = wqkv @ beta
    vec = torch.cat([bi, u2, b2])
    vec = torch.cat([vec, vec.new_zeros(-vec.numel() % 256)]).contiguous()
    ref_qk = torch.zeros(M, 2 * HD, device=DEV)
    ref_qk[:, real3[: 2 * HD]] = qkv[:, : 2 * INNER]
    ref_v = torch.zeros(M, HD, device=DEV)
    ref_v[:, cols >= 0] = qkv[:, 2 * INNER:]
    ref_vt = ref_v.reshape(B, hw, HEADS, DP).permute(0, 2, 3, 1)
    return dict(B=B, hw=hw, M=M, x=x, w1p=w1p, w2p=w2p, vec=vec, t0=t0, qk=ref_qk, vt=ref_vt)


def hblock_desc(k, rows):
    d = L.HblockDesc()
    d.x, d.ldx, d.m, d.c, d.heads, d.d = k["x"].data_ptr(), C_, k["M"], C_, HEADS, DP
    d.w_in, d.w_qkv, d.vec, d.ln_eps, d.ln_dim = k["w1p"].data_ptr(), k["w2p"].data_ptr(), k["vec"].data_ptr(), 1e-5, C_
    d.ld_t0, d.ld_qk, d.vt_ld = C_, 2 * HD, k["hw"]
    d.hw, d.rows_per_wg = k["hw"], rows
    return d


def run_hblock(ctx, k, rows, d=None):
    d = d or hblock_desc(k, rows)
    t0 = torch.zeros(k["M"], C_, device=DEV, dtype=torch.float16)
    qk = torch.zeros(k["M"], 2 * HD, device=DEV, dtype=torch.float16)
    vt = torch.zeros(k["B"], HEADS, DP, k["hw"], device=DEV, dtype=torch.float16)
    d.t0, d.qk, d.vt = t0.data_ptr(), qk.data_ptr(), vt.data_ptr()
    assert ctx.lib.upk_head_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_head_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    return t0, qk, vt


@pytest.mark.parametrize("B,hw,rows", CASES)
def test_head_block_tall_tiles_vs_torch(ctx, B, hw, rows):
    """t0, q | k and V^T against fp32 PyTorch with test_head_block_vs_torch's bounds, and two runs bit for bit."""
    k = hblock_case(ctx, B, hw)
    t0, qk, vt = run_hblock(ctx, k, rows)
    print("hblock B%d hw%d rows%d: t0 %.2e  qk %.2e  vt %.2e" % (B, hw, rows, rel_err(t0, k["t0"]), rel_err(qk, k["qk"]),
                                                                 rel_err(vt, k["vt"])))
    check(t0, k["t0"], tol=4e-3)
    check(qk, k["qk"], tol=8e-3)
    check(vt, k["vt"], tol=8e-3)
    for u, v in zip((t0, qk, vt), run_hblock(ctx, k, rows)):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B,hw,rows,nblk", [(2, 128, 64, 4), (2, 128, 128, 4), (1, 768, 128, 24)])
def test_head_block_tall_tiles_groupnorm_fold_is_bit_identical_to_the_launch(ctx, B, hw, rows, nblk):
    """gn_part at 64 / 128 rows: the GroupNorm applied on the tile inside the kernel == upk_groupnorm_apply + plain call."""
    M = B * hw
    x = (rnd(M, C_, seed=1) * 1.7 + 0.4).half()
    gamma, beta = 1 + 0.3 * rnd(C_, seed=2), 0.2 * rnd(C_, seed=3)
    w1p, _ = ctx.pack_weight(rnd(C_, C_, scale=1 / math.sqrt(C_), seed=4).contiguous())
    w2p, _ = ctx.pack_weight(rnd(3 * HD, C_, scale=1 / math.sqrt(C_), seed=5).contiguous())
    vec = torch.cat([rnd(C_, scale=0.1, seed=6), rnd(3 * HD, scale=0.3, seed=7), rnd(3 * HD, scale=0.1, seed=8)])
    vec = torch.cat([vec, vec.new_zeros(-vec.numel() % 256)]).contiguous()
    xf = x.float().reshape(B, nblk, hw // nblk, C_)
    part = torch.stack([xf.sum(2), (xf * xf).sum(2)], dim=2).contiguous()  # [B][nblk][2][ld]
    k = dict(B=B, hw=hw, M=M, x=x, w1p=w1p, w2p=w2p, vec=vec)
    xn = torch.zeros_like(x)
    ctx._chk(ctx.lib.upk_groupnorm_apply_nhwc_f16(ctx.h, x.data_ptr(), C_, C_, None, 0, 0, B, hw, 32, gamma.data_ptr(),
                                                  beta.data_ptr(), 1e-6, 0, xn.data_ptr(), C_, part.data_ptr(), 2, nblk, C_,
                                                  None, 0, 0, ctx._s()))
    plain = hblock_desc(k, rows)
    plain.x = xn.data_ptr()
    fold = hblock_desc(k, rows)
    fold.gn_part, fold.gn_gamma, fold.gn_beta = part.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    fold.gn_nblk, fold.gn_ld, fold.gn_groups, fold.gn_eps = nblk, C_, 32, 1e-6
    a, b = run_hblock(ctx, k, rows, plain), run_hblock(ctx, k, rows, fold)
    assert float(a[0].float().abs().max()) > 1.0  # (sanity of the test data)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------- xblock
@functools.lru_cache(maxsize=None)
def xblock_case(ctx, B, hw):
    """Operands and the fp32 reference of test_cross_block_vs_torch, computed once per shape."""
    M = B * hw
    a1r = rnd(M, INNER, seed=1)
    t0 = (rnd(M, C_, seed=2) * 1.5 + 0.3).half()
    wo1, bo1 = rnd(C_, INNER, scale=1 / math.sqrt(INNER), seed=3), rnd(C_, scale=0.1, seed=4)
    gamma, beta = 1 + 0.2 * rnd(C_, seed=5), 0.1 * rnd(C_, seed=6)
    wq = rnd(INNER, C_, scale=1 / math.sqrt(C_), seed=7)
    wo2, bo2 = rnd(C_, INNER, scale=1 / math.sqrt(INNER), seed=8), rnd(C_, scale=0.1, seed=9)
    kr, vr = rnd(B, NKV, INNER, seed=10), rnd(B, NKV, INNER, seed=11)
    scale = DH ** -0.5
    cols = head_cols(HEADS, DH, DP).to(DEV)
    real = cols >= 0

    def padded(x):
        out = torch.zeros(*x.shape[:-1], HD, device=DEV, dtype=torch.float16)
        out[..., real] = x.half()
        return out

    a1 = padded(a1r)
    kc = padded(kr).reshape(B * NKV, HD).contiguous()
    vt = torch.zeros(B, HEADS, DP, 96, device=DEV, dtype=torch.float16)
    vt[:, :, :DH, :NKV] = vr.half().reshape(B, NKV, HEADS, DH).permute(0, 2, 3, 1)
    t1 = (a1r.half().float() @ wo1.half().float().t() + bo1 + t0.float()).half().float()
    wqf = (wq * gamma[None, :]).half().float()
    xn = (t1 - t1.mean(1, keepdim=True)) * torch.rsqrt(t1.var(1, unbiased=False, keepdim=True) + 1e-5)
    q = (xn @ wqf.t() + wq @ beta).half().float().reshape(B, hw, HEADS, DH).permute(0, 2, 1, 3)
    kk = kr.half().float().reshape(B, NKV, HEADS, DH).permute(0, 2, 1, 3)
    v = vr.half().float().reshape(B, NKV, HEADS, DH).permute(0, 2, 1, 3)
    p = torch.softmax(q @ kk.transpose(-1, -2) * scale, dim=-1)
    a2 = (p @ v).permute(0, 2, 1, 3).reshape(M, INNER).half().float()
    ref = a2 @ wo2.half().float().t() + bo2 + t1
    w1p, n1 = ctx.pack_weight(wo1.contiguous(), col_map=cols)
    w3p, n3 = ctx.pack_weight(wo2.contiguous(), col_map=cols)
    wqp, nq = ctx.pack_weight((wq * gamma[None, :]).contiguous(), row_map=cols)
    assert n1 == C_ and n3 == C_ and nq == HD
    uq = torch.zeros(HD, device=DEV); uq[real] = wqf.sum(dim=1)
    bq = torch.zeros(HD, device=DEV); bq[real] = wq @ beta
    vec = torch.cat([bo1, uq, bq, bo2])
    vec = torch.cat([vec, vec.new_zeros(-vec.numel() % 256)]).contiguous()
    return dict(B=B, hw=hw, M=M, a1=a1, t0=t0, w1p=w1p, wqp=wqp, w3p=w3p, vec=vec, kc=kc, vt=vt, scale=scale, ref=ref)


def run_xblock(ctx, k, rows):
    y = torch.zeros(k["M"], C_, device=DEV, dtype=torch.float16)
    d = L.XblockDesc()
    d.a1, d.lda, d.m, d.c, d.heads, d.d = k["a1"].data_ptr(), HD, k["M"], C_, HEADS, DP
    d.t0, d.ld_t0 = k["t0"].data_ptr(), C_
    d.w_out1, d.w_q, d.w_out2, d.vec = k["w1p"].data_ptr(), k["wqp"].data_ptr(), k["w3p"].data_ptr(), k["vec"].data_ptr()
    d.ln_eps, d.ln_dim = 1e-5, C_
    d.k_ctx, d.ldk, d.n_kv = k["kc"].data_ptr(), HD, NKV
    d.vt_ctx, d.vt_ld, d.scale = k["vt"].data_ptr(), 96, k["scale"]
    d.y, d.ldy, d.hw, d.rows_per_wg = y.data_ptr(), C_, k["hw"], rows
    assert ctx.lib.upk_cross_block_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_cross_block_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("B,hw,rows", CASES)
def test_cross_block_tall_tiles_vs_torch(ctx, B, hw, rows):
    """Against test_cross_block_vs_torch's reference with its 8e-3, and two runs bit for bit."""
    k = xblock_case(ctx, B, hw)
    y = run_xblock(ctx, k, rows)
    print("xblock B%d hw%d rows%d: %.2e" % (B, hw, rows, rel_err(y, k["ref"])))
    check(y, k["ref"], tol=8e-3)
    assert torch.equal(y, run_xblock(ctx, k, rows))


# ---------------------------------------------------------------------------------- one tile height against another
@pytest.mark.parametrize("B,hw", [(2, 128), (1, 768)])
def test_row_chain_kernels_agree_across_tile_heights(ctx, B, hw):
    """Rows 32, 64 and 128 on the same inputs.  A row's GEMM K order does not depend on the tile height; only the lane
    split of the LayerNorm statistics does (512 / rows lanes per row), so the outputs may differ by fp32 summation order
    in the statistics, far inside the 8e-3 of the reference checks, which is the bound asserted.
    Observed on an MI355X (max |a - b| / max |a| over every pair of heights and both shapes): hblock t0 0 (bit for bit,
    asserted), q | k 3.86e-4, V^T 2.02e-4, xblock 4.88e-4 — an fp16 ulp or two of the largest output."""
    hk, xk = hblock_case(ctx, B, hw), xblock_case(ctx, B, hw)
    h = {r: run_hblock(ctx, hk, r) for r in (32, 64, 128)}
    x = {r: run_xblock(ctx, xk, r) for r in (32, 64, 128)}
    for a, b in ((32, 64), (32, 128), (64, 128)):
        errs = [rel_err(u, v) for u, v in zip(h[b], h[a])] + [rel_err(x[b], x[a])]
        print("B%d hw%d rows %d vs %d: t0 %.2e  qk %.2e  vt %.2e  xblock %.2e" % (B, hw, b, a, *errs))
        assert torch.equal(h[a][0], h[b][0])  # (t0 is in front of the LayerNorm: the same arithmetic at every height)
        assert max(errs) < 8e-3, errs


# ------------------------------------------------------------------------------------------------------- refusals
def test_tall_tiles_refuse_shapes_outside_their_domain(ctx):
    h = L.HblockDesc()
    h.m, h.c, h.heads, h.d, h.hw, h.rows_per_wg = 128, C_, HEADS, DP, 64, 128
    h.ldx, h.ld_t0, h.ld_qk, h.vt_ld = C_, C_, 2 * HD, 64
    assert not ctx.lib.upk_head_block_supported(ctx.h, C.byref(h))  # a workgroup would straddle two samples
    h.rows_per_wg = 64
    assert ctx.lib.upk_head_block_supported(ctx.h, C.byref(h))
    h.rows_per_wg = 256
    assert not ctx.lib.upk_head_block_supported(ctx.h, C.byref(h))
    x = L.XblockDesc()
    x.m, x.c, x.heads, x.d, x.hw, x.rows_per_wg, x.n_kv, x.vt_ld = 128, C_, HEADS, DP, 64, 128, NKV, 96
    x.lda, x.ld_t0, x.ldy, x.ldk = HD, C_, C_, HD
    assert not ctx.lib.upk_cross_block_supported(ctx.h, C.byref(x))
    x.rows_per_wg = 64
    assert ctx.lib.upk_cross_block_supported(ctx.h, C.byref(x))
    x.m, x.c, x.d, x.hw, x.rows_per_wg = 2048, 448, 64, 256, 128  # (the 16x16 level: its tile does not fit at 128 rows)
    x.lda, x.ld_t0, x.ldy, x.ldk = 512, 448, 448, 512
    assert not ctx.lib.upk_cross_block_supported(ctx.h, C.byref(x))
    x.rows_per_wg = 32
    assert ctx.lib.upk_cross_block_supported(ctx.h, C.byref(x))


# ---------------------------------------------------------------------------------------------------- model level
def test_unet_forward_with_tall_row_chain_tiles():
    """One forward of the bbox UNet at B = 1, 32x32 with both row-chain kernels forced to 128 rows against the same
    forward at 32 rows (measure and threshold of test_unet_forward_with_and_without_the_fused_head)."""
    import upgpt_amd
    from upgpt_amd import knobs, synth

    def run(rows):
        old = knobs.HBLOCK, knobs.XBLOCK, knobs.XB_ROWS
        knobs.HBLOCK, knobs.XBLOCK, knobs.XB_ROWS = "1", "1", rows
        try:
            m = upgpt_amd.build_model("bbox")
            synth.fill_module_(m)
            m = m.cuda()
            inp = synth.synth_inputs(1, (32, 32), 4, 87, 768, seed=3, text_only=True)
            cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
            t = torch.full((1,), 601, dtype=torch.long, device=DEV)
            eps = m.apply_model(inp["x_T"].cuda(), t, cond)
            pl = next(iter(m.model.diffusion_model._plans.values()))
            tag = "rows%d" % rows
            return eps.float().cpu(), [sum(1 for lab in pl.body.labels if lab.startswith(p) and lab.split(" gn")[0].endswith(tag))
                                       for p in ("hblock ", "xblock ")]
        finally:
            knobs.HBLOCK, knobs.XBLOCK, knobs.XB_ROWS = old

    e128, n128 = run(128)
    e32, n32 = run(32)
    assert n128 == [5, 5] and n32[0] == 5 and n32[1] >= 5, (n128, n32)
    assert float(((e128 - e32) ** 2).mean()) < 1e-5 * max(1.0, float((e32 ** 2).mean()))
