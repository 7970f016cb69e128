"""The streaming form of the fused feed-forward tail (upgpt_amd/csrc/mlp.hip mlp_stream_kernel; include/upk.h rows_per_wg
= 128 or 64 | UPK_MLP_STREAM): the hidden activation in two 128-column LDS slices instead of a whole tile.  Reference,
operands and bounds of tests/test_mlp_gpu.py::test_geglu_mlp_vs_torch, at the smallest shapes at which this kernel can still
go wrong: two workgroups with one tile per sample, two tiles per sample (the partial layout), a tail tile with rows past M,
a single partial tile — and against the resident kernels on the same operands."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from upgpt_amd import _lib as L
from test_ops_gpu import DEV, check, geglu_row_map, rnd

pytestmark = pytest.mark.gpu

C_ = 224
STREAM = L.MLP_STREAM


@functools.lru_cache(maxsize=None)
def mlp_case(ctx, M, c=C_):
    """Operands and the fp32 reference of test_geglu_mlp_vs_torch, computed once per shape."""
    inner = 4 * c
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.randn(M, c, generator=g) * (0.5 + 2 * torch.rand(M, 1, generator=g)) + 2 * torch.randn(M, 1, generator=g)).to(DEV).half()
    res = rnd(M, c, seed=7).half()
    gamma, beta = 1 + 0.2 * rnd(c, seed=2), 0.1 * rnd(c, seed=3)
    w1 = rnd(2 * inner, c, scale=1 / math.sqrt(c), seed=4)
    b1 = rnd(2 * inner, scale=0.1, seed=5)
    w2h = rnd(c, inner, scale=1 / math.sqrt(inner), seed=6)   # (P F2)
    w2x = rnd(c, c, scale=1 / math.sqrt(c), seed=8)           # P
    b2 = rnd(c, scale=0.1, seed=9)
    w1f = (w1 * gamma[None, :]).half().float()
    xn = (x.float() - x.float().mean(1, keepdim=True)) * torch.rsqrt(x.float().var(1, unbiased=False, keepdim=True) + 1e-5)
    hpre = xn @ w1f.t() + (b1 + w1 @ beta)
    h = (hpre[:, :inner] * F.gelu(hpre[:, inner:])).half().float()
    ref = res.float() + h @ w2h.half().float().t() + x.float() @ w2x.half().float().t() + b2
    rm = geglu_row_map(inner).to(DEV)
    w1p, n1 = ctx.pack_weight((w1 * gamma[None, :]).contiguous(), row_map=rm)
    b1p = (b1 + w1 @ beta)[rm.long()].contiguous()
    u1p = (w1 * gamma[None, :]).half().float().sum(dim=1)[rm.long()].contiguous()
    w2a, n_pad = ctx.pack_weight(w2h.contiguous())
    w2b, _ = ctx.pack_weight(w2x.contiguous())
    w2p = torch.cat([w2a.reshape(-1), w2b.reshape(-1)]).contiguous()
    b2p = torch.zeros(n_pad, device=DEV); b2p[:c] = b2
    return dict(M=M, c=c, inner=inner, x=x, res=res, ref=ref, w1p=w1p, b1p=b1p, u1p=u1p, w2p=w2p, b2p=b2p, n_pad=n_pad)


def mlp_desc(k, rows_per_wg, hw, y=None, sws=None):
    d = L.MlpDesc()
    c = k["c"]
    d.x, d.ldx, d.m, d.c, d.inner = k["x"].data_ptr(), c, k["M"], c, k["inner"]
    d.w1, d.b1, d.u1, d.ln_eps, d.ln_dim = k["w1p"].data_ptr(), k["b1p"].data_ptr(), k["u1p"].data_ptr(), 1e-5, c
    d.w2, d.b2, d.n_out, d.n_pad = k["w2p"].data_ptr(), k["b2p"].data_ptr(), c, k["n_pad"]
    d.residual, d.ld_res = k["res"].data_ptr(), c
    if y is not None:
        d.y, d.ldy = y.data_ptr(), c
    d.rows_per_wg, d.hw = rows_per_wg, hw
    if sws is not None:
        d.gn_stats_ws = sws.data_ptr()
    return d


def run_mlp(ctx, k, rows_per_wg, hw):
    """One launch: (y, partials [B, nblk, 2, n_pad] or None)."""
    rows = rows_per_wg & ~STREAM
    y = torch.zeros(k["M"], k["c"], device=DEV, dtype=torch.float16)
    sws = torch.zeros(ctx.gn_stats_floats(k["M"] // hw, k["n_pad"]), device=DEV) if hw else None
    d = mlp_desc(k, rows_per_wg, hw, y, sws)
    assert ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(d))
    ctx._chk(ctx.lib.upk_geglu_mlp_f16(ctx.h, C.byref(d), ctx._s()))
    torch.cuda.synchronize()
    if not hw:
        return y, None
    B, nblk = k["M"] // hw, hw // rows
    return y, sws[: B * nblk * 2 * k["n_pad"]].reshape(B, nblk, 2, k["n_pad"]).clone()


@pytest.mark.parametrize("rows_per_wg", [128, 64 | STREAM], ids=["rows128", "rows64s"])
@pytest.mark.parametrize("M,hw", [(256, 128), (512, 256), (200, 0), (96, 0)])
def test_streaming_mlp_vs_torch(ctx, M, hw, rows_per_wg):
    k = mlp_case(ctx, M)
    y, part = run_mlp(ctx, k, rows_per_wg, hw)
    check(y, k["ref"], tol=8e-3)
    if hw:
        yf = y.float().reshape(M // hw, hw, C_)
        check(part[:, :, 0, :C_].sum(1), yf.sum(1), tol=2e-3)
        check(part[:, :, 1, :C_].sum(1), (yf * yf).sum(1), tol=2e-3)
    y2, part2 = run_mlp(ctx, k, rows_per_wg, hw)  # bitwise reproducible
    assert torch.equal(y, y2)
    assert part is None or torch.equal(part, part2)


def test_streaming_mlp_against_the_resident_kernels(ctx):
    """Same operands, (M, hw) = (512, 256).  At 64 rows the two forms share the LayerNorm lane split and the K order of a
    row (hidden chunks ascending, then t2), so they are bit-identical, partials included.  The 128-row form differs from
    the 32-row kernel by the lane split of the LayerNorm statistics alone (4 against 16 lanes per row): the bound is the
    8e-3 of the largest output that test_row_chain_kernels_agree_across_tile_heights uses, 2e-3 on the per-sample sums."""
    k = mlp_case(ctx, 512)
    y64, p64 = run_mlp(ctx, k, 64, 256)
    y64s, p64s = run_mlp(ctx, k, 64 | STREAM, 256)
    assert torch.equal(y64s, y64)
    assert torch.equal(p64s, p64)
    y32, p32 = run_mlp(ctx, k, 32, 256)
    y128, p128 = run_mlp(ctx, k, 128, 256)
    err = (y128.float() - y32.float()).abs().max().item() / (y32.float().abs().max().item() + 1e-6)
    print("rows 128 (streaming) vs 32 (resident): max |a - b| / max |a| = %.2e" % err)
    assert err < 8e-3, err
    check(p128.sum(1), p32.sum(1), tol=2e-3)


def test_streaming_mlp_refusals(ctx):
    """Everything outside the domain is refused by upk_geglu_mlp_supported and as UpkError by the launch."""
    k = mlp_case(ctx, 512)
    y = torch.zeros(512, C_, device=DEV, dtype=torch.float16)
    sws = torch.zeros(ctx.gn_stats_floats(4, k["n_pad"]), device=DEV)

    def refused(d):
        assert not ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(d))
        with pytest.raises(L.UpkError):
            ctx._chk(ctx.lib.upk_geglu_mlp_f16(ctx.h, C.byref(d), ctx._s()))

    assert ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(mlp_desc(k, 128, 256, y, sws)))
    refused(mlp_desc(k, 96, 0, y))                 # no such tile height
    refused(mlp_desc(k, 96 | STREAM, 0, y))
    refused(mlp_desc(k, 32 | STREAM, 0, y))        # (the streaming form exists at 64 and 128 rows)
    refused(mlp_desc(k, 128, 192, y, sws))         # hw % rows != 0 with a statistics buffer
    refused(mlp_desc(k, 64 | STREAM, 160, y, sws))
    assert ctx.lib.upk_geglu_mlp_supported(ctx.h, C.byref(mlp_desc(k, 128, 192, y)))  # (without one, hw is not used)
    d = mlp_desc(k, 128, 256, y)                   # c = 448 at 128 rows: 114 KB of t2 + 64 KB of slices
    d.c, d.inner, d.ldx, d.ln_dim, d.n_out, d.n_pad, d.ld_res, d.ldy = 448, 1792, 448, 448, 448, 448, 448, 448
    refused(d)
    d.n_out, d.n_pad = 224, 224                    # (and not for its output width alone)
    refused(d)
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0             # no refused launch wrote


def test_unet_forward_with_the_streaming_mlp():
    """One forward of the bbox UNet at B = 1, 32x32 with the 128-row streaming form forced into its five 32x32-level
    transformer blocks against the default lowering of that shape (the two-launch path), by the criterion of
    test_unet_forward_with_and_without_the_fused_mlp."""
    import upgpt_amd
    from upgpt_amd import knobs, synth

    def run(fuse, rows):
        old = knobs.MLP_FUSE, knobs.MLP_ROWS
        knobs.MLP_FUSE, knobs.MLP_ROWS = fuse, rows
        try:
            m = upgpt_amd.build_model("bbox")
            synth.fill_module_(m)
            m = m.cuda()
            inp = synth.synth_inputs(1, (32, 32), 4, 87, 768, seed=3, text_only=True)
            cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
            t = torch.full((1,), 601, dtype=torch.long, device=DEV)
            eps = m.apply_model(inp["x_T"].cuda(), t, cond)
            pl = next(iter(m.model.diffusion_model._plans.values()))
            return eps.float().cpu(), [lab for lab in pl.body.labels if lab.startswith("mlp ")]
        finally:
            knobs.MLP_FUSE, knobs.MLP_ROWS = old

    e1, n1 = run("1", 128)
    e0, n0 = run("auto", 0)
    assert n0 == [] and len(n1) == 5 and all(lab.endswith("rows128s") for lab in n1), (n0, n1)
    assert float(((e1 - e0) ** 2).mean()) < 1e-5 * max(1.0, float((e0 ** 2).mean()))
