"""Every compiled attention instantiation (upk_attention_variant_name), pinned with upk_attention_override at 1, 2 and 4
waves per workgroup, against range_ref.attention_ref's fp64 reference and derived bound, at the shapes of
range_ref.attn_variant_rows() (the smallest that reach each code path), at three softmax regimes and in two operand
layouts: dense, and the production one (q | k as column halves of one buffer, a wider vt_ld whose unused columns hold NaN,
out inside a sentinel-filled buffer).  Then the census: every attention launch of the plans the benchmark replays and of
the guided UNet, upscale UNet, VAE encoder and image tower plans, with the variant it takes at the production batch, and a
replica of it at batch 2 under that variant.

tests/test_attention_variants_host.py shows that the criterion passes a faithful tiled emulation and fails on seeded
defects.  The fp64 references are computed on the device that holds the operands."""
import time

import pytest
import torch

import range_ref as R
from test_production_launches_gpu import B as PROD_B
import test_production_launches_gpu as P
from test_production_launches_gpu import model, towers, unet_plan, upscale_models  # noqa: F401  (the fixtures)
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ROWS = R.attn_variant_rows()
GROUPS = sorted({(r["family"], r["d"]) for r in ROWS})
LAYOUTS = ("dense", "production")

LAUNCHED = set()  # (variant name, waves per workgroup, causal) of every checked launch of this process
DONE = set()      # (family, d) groups of the table that ran
PEAK = {}         # variant name -> largest ratio
QT_SAME = {}      # (family, d) -> [(causal, n_q, one / two query groups per wave bit-identical?), ...]
CLOSURE = {(r["variant"], w) for r in ROWS for w in r["wpbs"]}  # what the table launches (the closure test checks it did)


def names(ctx):
    return ctx.attention_variants()


def pinned(ctx, variant, wpb, plan, launch):
    """Asks what would run, pins (variant, wpb), asks again, launches once; the heuristic is back afterwards."""
    idx = names(ctx).index(variant)
    free = plan()
    assert 0 <= free[0] < len(names(ctx)) and free[1] in (1, 2, 4)
    try:
        ctx.attention_override(idx, wpb)
        assert plan() == (idx, wpb), (variant, wpb, plan())
        launch()
    finally:
        ctx.attention_override(-1, 0)
    assert plan() == free
    torch.cuda.synchronize()
    return free


def attn_args(Lt, o):
    return (Lt["q"], Lt["ldq"], Lt["qbs"], Lt["k"], Lt["ldk"], Lt["kbs"], Lt["vt"], Lt["vt_ld"], Lt["out"], Lt["ldo"], Lt["obs"],
            o["B"], o["heads"])


def run_attn(ctx, Lt, o, variant, wpb):
    """One pinned launch of upk_attention_f16 / upk_attention_causal_f16 into the layout's out buffer."""
    a = attn_args(Lt, o)
    plan = lambda: ctx.attention_plan(*a, o["nq"], o["nkv"], o["d"], o["scale"], o["causal"])
    if o["causal"]:
        launch = lambda: ctx.attention_causal(*a, o["nq"], o["d"], o["scale"])
    else:
        launch = lambda: ctx.attention(*a, o["nq"], o["nkv"], o["d"], o["scale"])
    return pinned(ctx, variant, wpb, plan, launch)


def qproj_operands(o, dp):
    """x, the packed projection and k, v padded to the head width dp, on the device."""
    from upgpt_amd.packing import qproj_pack
    Bn, heads, dh, nkv, Cc = o["B"], o["heads"], o["dh"], o["nkv"], o["C"]
    k = torch.zeros(Bn, nkv, heads, dp, device=DEV, dtype=torch.float16)
    v = torch.zeros_like(k)
    k[..., :dh], v[..., :dh] = o["k"].to(DEV), o["v"].to(DEV)
    pack = qproj_pack(o["w"].to(DEV), o["gamma"].to(DEV), o["beta"].to(DEV), heads, dh, dp, Cc, DEV)
    return o["x"].to(DEV).contiguous(), pack, k.view(Bn, nkv, heads * dp), v.view(Bn, nkv, heads * dp)


def run_qproj(ctx, Lt, o, x, pack, dp, variant, wpb):
    Bn, heads, nq, nkv, Cc = o["B"], o["heads"], o["nq"], o["nkv"], o["C"]
    wq, wu, wb = pack
    plan = lambda: ctx.attention_qproj_plan(Cc, Cc, Cc, Lt["ldk"], Lt["vt_ld"], Lt["ldo"], Bn, heads, nq, nkv, dp)
    launch = lambda: ctx._chk(ctx.lib.upk_attention_qproj_f16(
        ctx.h, x.data_ptr(), Cc, nq * Cc, Cc, Cc, o["eps"], wq.data_ptr(), wu.data_ptr(), wb.data_ptr(), Lt["k"].data_ptr(),
        Lt["ldk"], Lt["kbs"], Lt["vt"].data_ptr(), Lt["vt_ld"], Lt["out"].data_ptr(), Lt["ldo"], Lt["obs"], Bn, heads, nq, nkv,
        dp, o["scale"], ctx._s()))
    return pinned(ctx, variant, wpb, plan, launch)


def to_dev(o):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()}


def check(what, s, got, ref, bound, variant):
    """got, ref, bound [B, h, nq, d]; -> ratio (asserted <= 1)."""
    assert bool(torch.isfinite(got).all()), what
    r = R.ratio(got, ref, bound)
    PEAK[variant] = max(PEAK.get(variant, 0.0), r)
    assert r <= 1, "%s scale %g: max err/bound %.3f" % (what, s, r)
    return r


def run_group(ctx, family, d):
    """Every row of the table with this (family, head dim): all scales, both layouts, every waves-per-workgroup count."""
    top, n_launch = 0.0, 0
    for row in ROWS:
        if (row["family"], row["d"]) != (family, d):
            continue
        Bn, heads, nq, nkv, variant = row["B"], row["heads"], row["nq"], row["nkv"], row["variant"]
        for s in R.ATTN_VARIANT_SCALES:
            o = to_dev(R.attn_variant_case(row, s))
            if family == "qproj":
                dh = o["dh"]
                x, pack, k, v = qproj_operands(o, d)
                q = None
                ref, bound = R.qproj_case_ref(o)
            else:
                dh = d
                q, k, v = o["q"], o["k"], o["v"]
                ref, bound = R.attn_case_ref(o)
            assert float(ref.abs().max()) < 6e4
            outs = []
            for layout in LAYOUTS:
                for wpb in row["wpbs"]:
                    Lt = R.attn_layout(q, k, v, heads, d, nq, layout)
                    what = "%s wpb %d nq %d nkv %d%s %s" % (variant, wpb, nq, nkv, " causal" if row["causal"] else "", layout)
                    if family == "qproj":
                        run_qproj(ctx, Lt, o, x, pack, d, variant, wpb)
                    else:
                        run_attn(ctx, Lt, o, variant, wpb)
                    n_launch += 1
                    assert R.attn_outside_untouched(Lt), what + ": wrote outside its rows / columns"
                    got = R.attn_owned(Lt).view(Bn, nq, heads, d)
                    if dh < d:
                        assert not got[..., dh:].any(), what + ": padded head columns not zero"
                    top = max(top, check(what, s, got[..., :dh].transpose(1, 2), ref, bound, variant))
                    LAUNCHED.add((variant, wpb, row["causal"]))
                    outs.append(got.clone())
                    if nkv == 1:  # p = 1 and the denominator is 1: the value row, bit for bit
                        want = v.view(Bn, 1, heads, d).expand(Bn, nq, heads, d)
                        assert torch.equal(got, want), what + ": one key, but out is not the value row"
            # waves share nothing, and a layout changes addresses only
            assert all(torch.equal(outs[0], t) for t in outs[1:]), "%s nq %d nkv %d: bits differ between wpb / layouts" % (
                variant, nq, nkv)
            if family in ("direct", "lds") and d <= 128 and row["qt"] == 1 and s == 1:
                # the same operands through the two-query-groups form of the same kernel
                other = R.attn_variant_name(family, d, 2)
                Lt = R.attn_layout(q, k, v, heads, d, nq, "production")
                run_attn(ctx, Lt, o, other, row["wpbs"][-1])
                assert R.attn_outside_untouched(Lt)
                got2 = R.attn_owned(Lt).view(Bn, nq, heads, d)
                check("%s on %s's shape" % (other, variant), s, got2.transpose(1, 2), ref, bound, other)
                QT_SAME.setdefault((family, d), []).append((row["causal"], nq, torch.equal(got2, outs[0])))
    DONE.add((family, d))
    return top, n_launch


@pytest.mark.parametrize("family,d", GROUPS)
def test_every_variant_against_fp64(ctx, family, d):
    t0 = time.perf_counter()
    top, n = run_group(ctx, family, d)
    same = QT_SAME.get((family, d), [])
    differ = ["causal n %d" % nq if c else "n_q %d" % nq for c, nq, eq in same if not eq]
    print("\nattention variants %s d=%d: %d pinned launches, largest err/bound %.3f, %.1f s%s" % (
        family, d, n, top, time.perf_counter() - t0,
        "" if not same else "; one vs two query groups per wave bit-identical in %d of %d shapes%s" % (
            len(same) - len(differ), len(same), " (not: %s)" % ", ".join(differ) if differ else "")))
    # without the mask the per-query arithmetic is the same code on the same tiles (attn_tile's rescale is exact when
    # alpha = 1): bit-identical.  With it a wave's key range ends at q0 + 16 qt, so a query can meet other tile
    # boundaries under the other form: equal within the bound (checked above), not in bits, from n = 77 on.
    assert all(eq for c, nq, eq in same if not c or nq <= 32), differ


def test_closure_every_variant_at_every_wpb_has_run(ctx):
    """A variant added to the library fails this until range_ref.attn_variant_rows() names it."""
    for g in GROUPS:
        if g not in DONE:
            run_group(ctx, *g)
    have = names(ctx)
    assert len(have) == ctx.lib.upk_attention_num_variants() == len(set(have))
    missing = []
    for name in have:
        family = next((f for f in R.ATTN_WPB if name.startswith(f)), None)
        assert family is not None, "variant %s: a family the table does not know" % name
        for wpb in R.ATTN_WPB[family]:
            if not any((name, wpb, c) in LAUNCHED for c in (False, True)):
                missing.append((name, wpb))
        if family == "direct" and name.endswith(("q1", "q2")):  # head dim <= 128: the causal mask too
            missing += [(name, wpb, "causal") for wpb in (1, 2, 4) if (name, wpb, True) not in LAUNCHED]
    assert not missing, "never launched: %s" % missing
    print("\nlargest err/bound per variant: " + ", ".join("%s %.3f" % (n, PEAK[n]) for n in have))


# ------------------------------------------------------------------------------------------------------------ refusals
def _refusal_case(ctx, d, nq, nkv, heads, ldk_extra=0):
    o = to_dev(R.attn_case("refusal", 1, (d, nq, nkv, False), B=2, heads=heads))
    Lt = R.attn_layout(o["q"], o["k"], o["v"], heads, d, nq, "dense")
    if ldk_extra < 0:  # vt rows -ldk_extra halves further apart (vt_ld % 4 == 0 is all the other kernels ask for)
        vt = torch.zeros(2, heads, d, Lt["vt_ld"] - ldk_extra, device=DEV, dtype=torch.float16)
        vt[..., :Lt["vt_ld"]] = Lt["vt"]
        Lt.update(vt=vt, vt_ld=Lt["vt_ld"] - ldk_extra)
    elif ldk_extra:  # k rows ldk_extra halves further apart
        kb = torch.zeros(2 * nkv, heads * d + ldk_extra, device=DEV, dtype=torch.float16)
        kb[:, :heads * d] = o["k"].reshape(2 * nkv, -1)
        Lt.update(k=kb, ldk=heads * d + ldk_extra, kbs=nkv * (heads * d + ldk_extra))
    return o, Lt


@pytest.mark.parametrize("what,variant,wpb,d,nkv,heads,ldk_extra", [
    ("lds at n_kv = 352", "lds32q1", 0, 32, 320 + 32, 3, 0),
    ("two query groups at d = 256", "direct128q2", 0, 256, 64, 3, 0),
    ("wide with two heads", "wide512", 0, 512, 64, 2, 0),
    ("wide with ldk % 8 != 0", "wide512", 0, 512, 64, 1, 4),
    ("wide with vt_ld % 8 != 0", "wide512", 0, 512, 64, 1, -4),
    ("wpb = 3", None, 3, 64, 64, 3, 0),
    ("wpb = 2 for an lds variant", "lds64q2", 2, 64, 256, 3, 0),
    ("a qproj variant through upk_attention_f16", "qproj32q2", 0, 32, 64, 3, 0),
])
def test_forced_variant_that_cannot_run_is_refused(ctx, what, variant, wpb, d, nkv, heads, ldk_extra):
    o, Lt = _refusal_case(ctx, d, 40, nkv, heads, ldk_extra)
    a = attn_args(Lt, o) + (o["nq"], o["nkv"], o["d"], o["scale"])
    assert (ldk_extra <= 0 or Lt["ldk"] % 8 == 4) and (ldk_extra >= 0 or Lt["vt_ld"] % 8 == 4)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    try:
        ctx.attention_override(names(ctx).index(variant) if variant else -1, wpb)
        with pytest.raises(L.UpkError) as e_plan:
            ctx.attention_plan(*a, False)
        with pytest.raises(L.UpkError) as e_run:
            ctx.attention(*a)
    finally:
        ctx.attention_override(-1, 0)
    torch.cuda.synchronize()
    assert e_plan.value.code == -2 and e_run.value.code == -2, (what, str(e_run.value))  # UPK_ESHAPE
    assert ctx.lib.upk_kernel_launches(ctx.h, 0) == 0, what
    assert bool((Lt["out_buf"] == R.ATTN_FILL).all()), what
    if ldk_extra <= 0:  # the same arguments run once the override is gone (ldk % 8 != 0: no kernel takes that)
        ctx.attention(*a)
        torch.cuda.synchronize()
        assert ctx.lib.upk_kernel_launches(ctx.h, 0) == 1
        ref, bound = R.attn_case_ref(o)
        assert R.ratio(R.attn_owned(Lt).view(2, 40, heads, d).transpose(1, 2), ref, bound) <= 1


# -------------------------------------------------------------------------------------------------------------- census
def plan_attention(plan):
    """The recorded attention launches of a plan's programs, in order."""
    out = []
    for n in ("prep", "body", "prog"):
        p = getattr(plan, n, None)
        if p is not None and hasattr(p, "attn"):
            out += p.attn
    return out


def ref_per_head(q, k, v, scale, dq=None):
    """attention_ref one (sample, head) at a time on the operands' device: [B, h, n, d] -> (ref, bound)."""
    ref, bound = torch.empty(q.shape, dtype=F64, device=q.device), torch.empty(q.shape, dtype=F64, device=q.device)
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            ref[b, h], bound[b, h] = R.attention_ref(q[b, h].to(F64), k[b, h].to(F64), v[b, h].to(F64), scale,
                                                     dq=None if dq is None else dq[b, h])
    return ref, bound


def replica(ctx, a, variant, wpb):
    """The launch `a` (a dict of Program.attn) at batch 2 on operands of this test, with a's own leading dimensions and
    batch strides, under the pinned (variant, wpb); -> err/bound."""
    Bn, heads, nq, nkv, d = 2, a["heads"], a["nq"], a["nkv"], a["d"]
    hd, rup = heads * d, (nkv + 31) // 32 * 32
    nan = float("nan")
    new = lambda shape, val: torch.full(shape, val, dtype=torch.float16, device=DEV)
    if a["kind"] == "qproj":
        dh = R.QPROJ_VARIANT_SHAPES[d][1]
        assert a["cq"] == a["ln_dim"] == a["ldx"] and a["xbs"] == nq * a["ldx"]
        o = to_dev(R.qproj_case(1, dict(C=a["cq"], heads=heads, dh=dh, nq=nq, nkv=nkv), B=Bn))
        x, pack, k, v = qproj_operands(o, d)
        q = None
    else:
        dh = d
        o = to_dev(R.attn_case("census", 1, (d, nq, nkv, False), B=Bn, heads=heads))
        q, k, v = o["q"], o["k"], o["v"]
    assert a["ldk"] >= hd and a["kbs"] == nkv * a["ldk"] and a["vt_ld"] >= rup and a["ldo"] >= hd and a["obs"] == nq * a["ldo"]
    Lt = dict(nq=nq, nkv=nkv, hd=hd, ldk=a["ldk"], kbs=a["kbs"], vt_ld=a["vt_ld"], ldo=a["ldo"], obs=a["obs"], q=None, ldq=0, qbs=0)
    shared = q is not None and nq == nkv and a["ldq"] == a["ldk"] >= 2 * hd  # q | k: the column halves of one buffer
    kb = new((Bn * nkv, a["ldk"]), nan)
    koff = hd if shared else 0
    kb[:, koff:koff + hd] = k.reshape(Bn * nkv, hd)
    Lt["k"] = kb[:, koff:]
    if q is not None:
        assert a["ldq"] >= hd and a["qbs"] == nq * a["ldq"]
        qb = kb if shared else new((Bn * nq, a["ldq"]), nan)
        qb[:, :hd] = q.reshape(Bn * nq, hd)
        Lt.update(q=qb, ldq=a["ldq"], qbs=a["qbs"])
        assert (Lt["q"].data_ptr() | Lt["k"].data_ptr()) & 15 == 0 and a["align"] == 0
    vt = new((Bn, heads, d, a["vt_ld"]), nan)  # NaN at and beyond round_up(nkv, 32): never read
    vt[..., :rup] = 0
    vt[..., :nkv] = v.reshape(Bn, nkv, heads, d).permute(0, 2, 3, 1)
    buf = new((Bn * nq + 2, a["ldo"]), R.ATTN_FILL)
    Lt.update(vt=vt, out=buf)
    if q is not None:
        run_attn(ctx, Lt, dict(o, B=Bn), variant, wpb)
        ref, bound = ref_per_head(*(t.view(Bn, -1, heads, d).transpose(1, 2) for t in (q, k, v)), o["scale"])
    else:
        run_qproj(ctx, Lt, o, x, pack, d, variant, wpb)
        ref, bound = R.qproj_case_ref(o)
    owned = buf[:Bn * nq, :hd]
    rest = buf.clone()
    rest[:Bn * nq, :hd] = R.ATTN_FILL
    assert bool((rest == R.ATTN_FILL).all()), "wrote outside its rows / columns"
    got = owned.reshape(Bn, nq, heads, d)
    assert bool(torch.isfinite(got).all()) and not got[..., dh:].any()
    return R.ratio(got[..., :dh].transpose(1, 2), ref, bound)


def census(ctx, plan, title):
    """One line per distinct attention launch of the plan: what it takes at the production batch; then its replica."""
    launches = plan_attention(plan)
    assert launches, title + ": the plan records no attention launch"
    have = names(ctx)
    seen = {}
    for a in launches:
        key = tuple(sorted(a.items()))
        seen[key] = seen.get(key, 0) + 1
    lines = []
    for key, count in seen.items():
        a = dict(key)
        hd = a["heads"] * a["d"]
        if a["kind"] == "qproj":
            v, w = ctx.attention_qproj_plan(a["ldx"], a["cq"], a["ln_dim"], a["ldk"], a["vt_ld"], a["ldo"], a["B"], a["heads"],
                                            a["nq"], a["nkv"], a["d"])
        else:
            # (the pointers enter the choice through their alignment only: production's are 16-byte aligned, as asserted
            # in replica(); nothing is enqueued, nothing is read)
            p = torch.empty(8, device=DEV, dtype=torch.float16)
            assert p.data_ptr() % 16 == 0 and a["align"] == 0
            v, w = ctx.attention_plan(p, a["ldq"], a["qbs"], p, a["ldk"], a["kbs"], p, a["vt_ld"], p, a["ldo"], a["obs"],
                                      a["B"], a["heads"], a["nq"], a["nkv"], a["d"], a["scale"], False)
        name = have[v]
        family = next(f for f in R.ATTN_WPB if name.startswith(f))
        assert (name, w) in CLOSURE and w in R.ATTN_WPB[family], "%s wpb %d is not in the table's closure" % (name, w)
        r = replica(ctx, a, name, w)
        PEAK[name] = max(PEAK.get(name, 0.0), r)
        lines.append("    %-5s x%-2d B %d heads %d nq %4d nkv %4d d %3d ldq %4d ldk %4d vt_ld %4d -> %-11s wpb %d   replica (B = 2) "
                     "err/bound %.3f" % (a["kind"], count, a["B"], a["heads"], a["nq"], a["nkv"], a["d"], a.get("ldq", 0),
                                         a["ldk"], a["vt_ld"], name, w, r))
        assert r <= 1, lines[-1]
    print("\n%s: %d attention launches, %d distinct\n%s" % (title, len(launches), len(seen), "\n".join(lines)))


@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_census_of_the_unet_plans(ctx, model, H, W, lanes):
    census(ctx, unet_plan(model, H, W, lanes), "UNet %dx%d B = %d, %s" % (H, W, PROD_B, "shared_chip(4)" if lanes > 1 else
                                                                          "single forward"))


@pytest.mark.parametrize("h,w", [(32, 32), (32, 24)])
def test_census_of_the_vae_decoder_plans(ctx, model, h, w):
    census(ctx, model.first_stage_model._decode_plan(PROD_B, h, w, 0.18215), "VAE decoder %dx%d B = %d" % (h, w, PROD_B))


# ------------------------------------------------------------------- the plans beyond the headline (built as P names them)
@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_census_of_the_guided_unet_plans(ctx, model, H, W, lanes):
    plan = P.in_lanes(lanes, lambda: model.model.diffusion_model.plan(2 * PROD_B, H, W, P.NCTX, P.STEPS, "sampler"))
    census(ctx, plan, "guided UNet %dx%d 2B = %d, %s" % (H, W, 2 * PROD_B, P.lanes_title(lanes)))


@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("h,w", P.UP_LATENTS)
def test_census_of_the_upscale_unet_plans(ctx, upscale_models, h, w, lanes):
    unet = upscale_models((h, w)).model.diffusion_model
    plan = P.in_lanes(lanes, lambda: unet.plan(P.UP_B, h, w, P.UP_NCTX, P.STEPS, "sampler"))
    census(ctx, plan, "upscale UNet %dx%d B = %d, %s" % (h, w, P.UP_B, P.lanes_title(lanes)))


@pytest.mark.parametrize("H,W", [(256, 256), (256, 192)])
def test_census_of_the_vae_encoder_plans(ctx, model, H, W):
    census(ctx, model.first_stage_model._encode_plan(PROD_B, H, W), "VAE encoder %dx%d B = %d" % (H, W, PROD_B))


def test_census_of_the_image_tower_plan(ctx, towers):
    """ViT-L/14 at N = 8 x 9 crops: 24 launches of one shape, 16 heads of 64 over 257 tokens (vt_ld 288).  The laion
    stage's image tower has the same dimensions and so the same launch.  Not here: the text tower's causal kernel and the
    cross stage's few-keys kernel are single-variant; tests/test_clip_gpu.py and tests/test_laion_cond_gpu.py run them at
    their production head and token counts."""
    title, build = P.tower_plan(towers, "image")
    plan = build()
    assert len(plan_attention(plan)) == plan.cfg["layers"] == 24
    census(ctx, plan, title)
