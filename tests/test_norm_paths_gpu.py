"""Every kernel path of upgpt_amd/csrc/norm.hip against the fp64 bounds of tests/range_ref.py, at the shapes of
tests/norm_ref.py's tables (tests/test_norm_paths_host.py shows what those bounds can and cannot tell apart).

Before a GroupNorm launch the test asks upk_groupnorm_plan which path the call takes and asserts it is the one the case
is in the table for.  Inputs are allocated with leading dimensions larger than the channel count and NaN in the unused
columns (a read of padding poisons the statistics); outputs and workspaces are prefilled with NaN, which both fails the
comparison of anything a kernel owns and leaves unwritten, and must still be there, bit for bit, in everything the ABI does
not define as written: y's padding columns, the statistics workspace past [B][nchunks][groups][2], all of it on the
one-launch paths.

Not covered: the cap rows <= 4096 of the apply pass needs 16.7 M pixels per launch (a 4 GB tensor at 128 channels)."""
import pytest
import torch

import norm_ref as N
import range_ref as R
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
NAN = float("nan")
KIND = {torch.float16: torch.int16, torch.float32: torch.int32}
d64 = lambda t: t.to(DEV, F64)


def report(path, what, s, r):
    print("norm %-14s %-40s scale %-5g max err/bound %.3f" % (path, what, s, r))
    return r


def untouched(t):
    """Whether every element of t still holds the NaN it was prefilled with, bit for bit."""
    fill = torch.full((1,), NAN, dtype=t.dtype, device=t.device).view(KIND[t.dtype])
    return bool((t.contiguous().view(KIND[t.dtype]) == fill).all())


def padded(x16, ld):
    """[B, hw, c] -> device [B, hw, ld], NaN in the columns >= c."""
    out = torch.full(x16.shape[:-1] + (ld,), NAN, dtype=torch.float16, device=DEV)
    out[..., :x16.shape[-1]] = x16
    return out


def sources(x16, c1, c2):
    """The one or two sources of a concat input, with ld1 = c1 + 8 and ld2 = c2 + 24."""
    xa = padded(x16[..., :c1], c1 + 8)
    xb = padded(x16[..., c1:], c2 + 24) if c2 else None
    return xa, c1 + 8, xb, (c2 + 24 if c2 else 0)


def workspace(ctx, B, hw):
    """The statistics workspace (NaN) with 256 floats of slack behind what upk_groupnorm_ws_bytes asks for."""
    return torch.full((ctx.groupnorm_ws_bytes(B, hw) // 4 + 256,), NAN, device=DEV)


def plan_is(ctx, c1, c2, B, hw, groups, stats, apply, **want):
    p = ctx.groupnorm_plan(c1, c2, B, hw, groups, stats, apply)
    for k, v in want.items():
        assert p[k] == v, "plan %s = %r, the case expects %r (%r)" % (k, p[k], v, p)
    return p


def stats_launch(ctx, xa, c1, lda, xb, c2, ldb, B, hw, groups, ws):
    ctx._chk(ctx.lib.upk_groupnorm_stats_nhwc_f16(ctx.h, xa.data_ptr(), c1, lda, xb.data_ptr() if c2 else None, c2, ldb, B,
                                                  hw, groups, ws.data_ptr(), ctx._s()))


def apply_launch(ctx, xa, c1, lda, xb, c2, ldb, B, hw, groups, gamma, beta, eps, silu, y, ldy, ws, mode=1, nblk=0, sld=0,
                 ws2=None, nblk2=0, sld2=0):
    ctx._chk(ctx.lib.upk_groupnorm_apply_nhwc_f16(
        ctx.h, xa.data_ptr(), c1, lda, xb.data_ptr() if c2 else None, c2, ldb, B, hw, groups, gamma.data_ptr(),
        beta.data_ptr(), eps, int(silu), y.data_ptr(), ldy, ws.data_ptr(), mode, nblk, sld,
        ws2.data_ptr() if ws2 is not None else None, nblk2, sld2, ctx._s()))


def check_y(path, what, s, y, C, ref, bound):
    """y [B, hw, ldy]: the first C columns inside the bound, the others untouched."""
    r = report(path, what, s, R.ratio(y[..., :C], ref, bound))
    assert r <= 1, what
    assert untouched(y[..., C:]), what + ": y's padding columns were written"


def check_ws(path, what, s, ws, x64, B, groups, nch, ppc):
    """The workspace of a statistics pass, chunk by chunk and sample by sample; everything behind it untouched."""
    n = B * nch * groups * 2
    got = ws[:n].view(B, nch, groups, 2)
    r = 0.0
    for b in range(B):
        ref, bnd = N.stats_chunk_refs(x64(b), groups, nch, ppc)
        r = max(r, R.ratio(got[b:b + 1], ref, bnd))
    report(path, what, s, r)
    assert r <= 1, what
    assert untouched(ws[n:]), what + ": the workspace was written past [B][nchunks][groups][2]"


def test_every_path_is_claimed_by_a_case_whose_plan_matches(ctx):
    names = ctx.groupnorm_paths()
    assert tuple(names) == N.PATHS and ctx.lib.upk_groupnorm_path_name(len(names)) == b"?"
    claimed = set()
    for name, (c1, c2, hw, B, groups, path) in N.ONEPASS_CASES.items():
        plan_is(ctx, c1, c2, B, hw, groups, True, True, path=path)
        # the halves of the call never take the one-launch kernel
        plan_is(ctx, c1, c2, B, hw, groups, True, False, path="twopass", apply_rows=0, apply_blocks=0)
        plan_is(ctx, c1, c2, B, hw, groups, False, True, path="twopass")
        claimed.add(path)
    for name, (c1, c2, hw, B, groups, nch, ppc) in N.STATS_CASES.items():
        plan_is(ctx, c1, c2, B, hw, groups, True, False, path="twopass", nchunks=nch, pix_per_chunk=ppc)
        assert ctx.lib.upk_groupnorm_chunks(hw) == nch
        claimed.add("twopass")
    assert claimed == set(names)


def test_plan_refuses_what_the_launch_refuses(ctx):
    """Sizes the library rejects before any launch: the query and the call give the same code."""
    buf = torch.zeros(2 * 64 * 2064, dtype=torch.float16, device=DEV)
    par = torch.zeros(4096, device=DEV)
    ws = workspace(ctx, 2, 64)
    cases = [((12, 0, 2, 64, 4), -1), ((32, -8, 2, 64, 4), -1), ((32, 0, 2, 64, 33), -2), ((40, 0, 2, 64, 32), -2),
             ((2056, 0, 2, 64, 8), -2), ((32, 0, 2, 0, 32), -1), ((32, 0, 0, 64, 32), -1)]
    for (c1, c2, B, hw, groups), code in cases:
        with pytest.raises(L.UpkError) as e1:
            ctx.groupnorm_plan(c1, c2, B, hw, groups)
        with pytest.raises(L.UpkError) as e2:
            ctx.groupnorm(buf, c1, 2064, buf, c2, 2064, B, hw, groups, par, par, 1e-5, False, buf, 2064, ws)
        assert e1.value.code == e2.value.code == code, (c1, c2, B, hw, groups)
    with pytest.raises(L.UpkError):
        ctx.groupnorm_plan(32, 0, 2, 64, 32, False, False)
    torch.cuda.synchronize()
    assert untouched(ws)


# ---------------------------------------------------------------------------------------------------------------------
# A. the statistics pass, then mode-1 apply (two sources: the whole call) on the same shape
@pytest.mark.parametrize("name", list(N.STATS_CASES))
def test_statistics_pass_per_chunk_and_apply(ctx, name):
    c1, c2, hw, B, groups, nch, ppc = N.STATS_CASES[name]
    C = c1 + c2
    for s in N.SCALES:
        x16, gamma, beta = N.gn_data(name, C, hw, B, s)
        xa, lda, xb, ldb = sources(x16, c1, c2)
        x, g64, b64 = d64(x16), d64(gamma), d64(beta)
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        ws = workspace(ctx, B, hw)
        plan_is(ctx, c1, c2, B, hw, groups, True, False, path="twopass", nchunks=nch, pix_per_chunk=ppc)
        stats_launch(ctx, xa, c1, lda, xb, c2, ldb, B, hw, groups, ws)
        torch.cuda.synchronize()
        check_ws("twopass.stats", name, s, ws, lambda b: x[b:b + 1], B, groups, nch, ppc)
        for eps in N.EPS:
            for silu in (False, True):
                ref, bound = R.groupnorm_ref(x, groups, g64, b64, eps, silu)
                y = torch.full((B, hw, C + 16), NAN, dtype=torch.float16, device=DEV)
                tag = "%s eps=%g silu=%d" % (name, eps, silu)
                if c2:  # (mode 1 describes a single-source tensor)
                    plan_is(ctx, c1, c2, B, hw, groups, True, True, path="twopass", nchunks=nch, pix_per_chunk=ppc)
                    ws.fill_(NAN)
                    ctx.groupnorm(xa, c1, lda, xb, c2, ldb, B, hw, groups, gamma, beta, eps, silu, y, C + 16, ws)
                    torch.cuda.synchronize()
                    check_y("twopass", tag + " one call", s, y, C, ref, bound)
                    check_ws("twopass.stats", tag + " one call", s, ws, lambda b: x[b:b + 1], B, groups, nch, ppc)
                else:
                    plan_is(ctx, c1, 0, B, hw, groups, False, True, path="twopass", nchunks=nch, pix_per_chunk=ppc)
                    keep = ws.clone()
                    apply_launch(ctx, xa, c1, lda, None, 0, 0, B, hw, groups, gamma, beta, eps, silu, y, C + 16, ws)
                    torch.cuda.synchronize()
                    check_y("twopass.apply1", tag, s, y, C, ref, bound)
                    assert torch.equal(ws.view(torch.int32), keep.view(torch.int32)), "the apply pass wrote its statistics"


# ---------------------------------------------------------------------------------------------------------------------
# B. the one-launch kernel, every instantiation the dispatch can pick, and the shapes at <= 64 pixels it cannot take
@pytest.mark.parametrize("name", list(N.ONEPASS_CASES))
def test_small_feature_maps_one_call(ctx, name):
    c1, c2, hw, B, groups, path = N.ONEPASS_CASES[name]
    C = c1 + c2
    for s in N.SCALES:
        x16, gamma, beta = N.gn_data(name, C, hw, B, s)
        xa, lda, xb, ldb = sources(x16, c1, c2)
        x, g64, b64 = d64(x16), d64(gamma), d64(beta)
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        p = plan_is(ctx, c1, c2, B, hw, groups, True, True, path=path)
        for eps in N.EPS:
            for silu in (False, True):
                ref, bound = R.groupnorm_ref(x, groups, g64, b64, eps, silu)
                tag = "%s eps=%g silu=%d" % (name, eps, silu)
                ys = []
                for _ in range(2):
                    ws = workspace(ctx, B, hw)
                    y = torch.full((B, hw, C + 16), NAN, dtype=torch.float16, device=DEV)
                    ctx.groupnorm(xa, c1, lda, xb, c2, ldb, B, hw, groups, gamma, beta, eps, silu, y, C + 16, ws)
                    torch.cuda.synchronize()
                    ys.append(y)
                check_y(path, tag, s, ys[0], C, ref, bound)
                assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), tag + ": a rerun differs"
                if path == "twopass":
                    check_ws("twopass.stats", tag, s, ws, lambda b: x[b:b + 1], B, groups, p["nchunks"], p["pix_per_chunk"])
                else:
                    assert untouched(ws), tag + ": the one-launch kernel wrote the workspace"


# ---------------------------------------------------------------------------------------------------------------------
# C. mode-2 apply and the fold on partials built here from the fp16 data
@pytest.mark.parametrize("name", list(N.MODE2_CASES))
def test_apply_on_channel_partials(ctx, name):
    c1, c2, hw, B, groups, nb1, nb2, sld1, sld2 = N.MODE2_CASES[name]
    C = c1 + c2
    for s in N.SCALES:
        x16, gamma, beta = N.gn_data(name, C, hw, B, s)
        xa, lda, xb, ldb = sources(x16, c1, c2)
        x, g64, b64 = d64(x16), d64(gamma), d64(beta)
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        pa = N.make_partials(x16[..., :c1].contiguous().to(DEV), nb1, sld1)
        pb = N.make_partials(x16[..., c1:].contiguous().to(DEV), nb2, sld2) if c2 else None
        plan_is(ctx, c1, c2, B, hw, groups, False, True, path="twopass")
        for eps in N.EPS:
            for silu in (False, True):
                ref, bound = R.groupnorm_ref(x, groups, g64, b64, eps, silu)
                y = torch.full((B, hw, C + 16), NAN, dtype=torch.float16, device=DEV)
                apply_launch(ctx, xa, c1, lda, xb, c2, ldb, B, hw, groups, gamma, beta, eps, silu, y, C + 16, pa, 2, nb1, sld1,
                             pb, nb2, sld2)
                torch.cuda.synchronize()
                check_y("twopass.apply2", "%s eps=%g silu=%d" % (name, eps, silu), s, y, C, ref, bound)


@pytest.mark.parametrize("name", list(N.FINALIZE_CASES))
def test_fold_of_many_block_partials(ctx, name):
    c, hw, B, groups, nblk, ld, then_apply = N.FINALIZE_CASES[name]
    nch = ctx.lib.upk_groupnorm_chunks(hw)
    for s in N.SCALES:
        x16, gamma, beta = N.gn_data(name, c, hw, B, s, device=DEV)
        part = N.make_partials(x16, nblk, ld)
        ws = workspace(ctx, B, hw)
        ctx._chk(ctx.lib.upk_groupnorm_finalize_f32(ctx.h, part.data_ptr(), nblk, ld, B, hw, c, groups, ws.data_ptr(),
                                                    ctx._s()))
        torch.cuda.synchronize()
        n = B * nch * groups * 2
        got = ws[:n].view(B, nch, groups, 2)
        r = 0.0
        for b in range(B):
            ref, bnd = N.fold_refs(x16[b:b + 1].to(F64), nblk, groups)
            r = max(r, R.ratio(got[b:b + 1, 0], ref, bnd))
        assert report("finalize", "%s (%d pairs per group)" % (name, nblk * c // groups), s, r) <= 1
        assert bool((got[:, 1:].contiguous().view(torch.int32) == 0).all()), "chunks >= 1 must be +0"
        assert untouched(ws[n:]), "the fold wrote past [B][nchunks][groups][2]"
        if not then_apply:
            continue
        xa = padded(x16, c + 8)
        g64, b64 = d64(gamma), d64(beta)
        gamma, beta = gamma.to(DEV), beta.to(DEV)
        plan_is(ctx, c, 0, B, hw, groups, False, True, path="twopass", nchunks=nch)
        for eps in N.EPS:
            for silu in (False, True):
                y = torch.full((B, hw, c + 16), NAN, dtype=torch.float16, device=DEV)
                apply_launch(ctx, xa, c, c + 8, None, 0, 0, B, hw, groups, gamma, beta, eps, silu, y, c + 16, ws)
                torch.cuda.synchronize()
                r = 0.0
                for b in range(B):
                    ref, bound = R.groupnorm_ref(x16[b:b + 1].to(F64), groups, g64, b64, eps, silu)
                    r = max(r, R.ratio(y[b:b + 1, :, :c], ref, bound))
                assert report("twopass.apply1", "%s eps=%g silu=%d after the fold" % (name, eps, silu), s, r) <= 1
                assert untouched(y[..., c:])


# ---------------------------------------------------------------------------------------------------------------------
# D. the refill loop of the apply pass: a block that owns more than 4 x 256 vectors
def test_apply_refill_loop(ctx):
    D = N.REFILL
    c, hw, B, groups, eps, silu = D["c"], D["hw"], D["B"], D["groups"], D["eps"], D["silu"]
    x16, gamma, beta = N.gn_data("refill", c, hw, B, 1, device=DEV)
    g64, b64 = d64(gamma), d64(beta)
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    xa = padded(x16, c + 8)
    ws = workspace(ctx, B, hw)
    y = torch.full((B, hw, c + 16), NAN, dtype=torch.float16, device=DEV)
    plan_is(ctx, c, 0, B, hw, groups, True, False, path="twopass", nchunks=D["nchunks"], pix_per_chunk=D["ppc"])
    p = plan_is(ctx, c, 0, B, hw, groups, False, True, path="twopass", apply_rows=D["rows"], apply_blocks=D["blocks"])
    assert p["apply_rows"] * c // 8 > 1024  # more vectors than the 4 x 256 a block prefetches: the loop runs
    stats_launch(ctx, xa, c, c + 8, None, 0, 0, B, hw, groups, ws)
    apply_launch(ctx, xa, c, c + 8, None, 0, 0, B, hw, groups, gamma, beta, eps, silu, y, c + 16, ws)
    torch.cuda.synchronize()
    check_ws("twopass.stats", "refill", 1, ws, lambda b: x16[b:b + 1].to(F64), B, groups, D["nchunks"], D["ppc"])
    r = 0.0
    for b in range(B):
        ref, bound = R.groupnorm_ref(x16[b:b + 1].to(F64), groups, g64, b64, eps, silu)
        r = max(r, R.ratio(y[b:b + 1, :, :c], ref, bound))
        del ref, bound
    assert report("twopass.apply1", "refill (%d rows per block)" % p["apply_rows"], 1, r) <= 1
    assert untouched(y[..., c:])


# ---------------------------------------------------------------------------------------------------------------------
# E. LayerNorm: 1, 2 and 4 vectors per lane on both sides of both thresholds
@pytest.mark.parametrize("d", N.LN_D)
def test_layernorm_rows(ctx, d):
    nv = d // 8
    path = "layernorm<%d>" % (1 if nv <= 64 else 2 if nv <= 128 else 4)
    for rows in N.LN_ROWS:
        for s in N.SCALES:
            x16, gamma, beta = N.ln_data(rows, d, s)
            xa = padded(x16, d + 8)
            for eps in N.EPS:
                ref, bound = R.layernorm_ref(d64(x16), d64(gamma), d64(beta), eps)
                y = torch.full((rows, d + 16), NAN, dtype=torch.float16, device=DEV)
                ctx.layernorm(xa, d + 8, rows, d, gamma.to(DEV), beta.to(DEV), eps, y, d + 16)
                torch.cuda.synchronize()
                check_y(path, "%dx%d eps=%g" % (rows, d, eps), s, y, d, ref, bound)
