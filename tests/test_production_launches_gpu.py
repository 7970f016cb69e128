"""Every conv / GEMM launch of the production plans, at the shape and the (tile configuration, split-K) it runs with,
against the fp64 reference of tests/launch_ref.py.

The plans are built, never run: bbox UNet at B = 8, 87 context tokens, latent 32x32 and 32x24, once under the single-forward
table and once inside shared_chip(4) (lanes overlay, other lowering), and the VAE decoder at B = 8 for both latents (one
case per resolution level: its 256x256 level alone is M = 524288 rows): the headline benchmark's.  Then the plans behind
its secondary figures and behind test_step / edit_region / validation_step: the guided sampler's UNet plan
(2B = 16 rows), the upscale UNet at B = 4 (64x64 and 128x96, one case per level) and its kl-f4 decoder, the VAE encoder,
the CLIP text tower (hidden states and pooled), the ViT-L/14 image tower at 72 crops, the laion stage's two towers and its
cross stage, and LPIPS for one pair.  Inside shared_chip(4) those plans launch only what differs from their single-forward
lowering.

For each distinct launch of a plan a REPLICA descriptor carries every shape, flag, stride, leading dimension and choice of
the production descriptor, while every pointer goes to operands this test owns: the production buffers and weights are
never touched.  One launch, then ``range_ref.ratio(got, ref, bound) <= 1`` for the output and for every by-product.
tests/test_launch_ref_host.py shows that this criterion fails on a subtly wrong output."""
import ctypes as C
import re
import time
import zlib

import pytest
import torch

import launch_ref as LR
import range_ref as R
from test_dynamic_range_gpu import check_mlp_tail, launch_cross_block, launch_head_block, launch_mlp_tail, report
from test_ops_gpu import _phase_weights, geglu_row_map
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
B, NCTX, STEPS = 8, 87, 50
FILL = 7.0  # what every output buffer holds before the launch: an element the launch must not write keeps it


@pytest.fixture(scope="module")
def model():
    import upgpt_amd
    from upgpt_amd import synth
    m = upgpt_amd.build_model("bbox")
    synth.fill_module_(m)
    return m.cuda()


def unet_plan(model, H, W, lanes):
    unet = model.model.diffusion_model
    if lanes > 1:
        with L.shared_chip(lanes):
            return unet.plan(B, H, W, NCTX, STEPS, "sampler")
    return unet.plan(B, H, W, NCTX, STEPS, "sampler")


# --------------------------------------------------------------------------------------------------------- the replica
class Replica:
    """A descriptor with the production descriptor's numbers and this test's operands."""

    def __init__(self, ctx, d, key, slots_in, cache):
        f = self.f = LR.fields(d)
        bad = LR.unhandled(f)
        assert not bad, "%s: the replica builder does not handle %s" % (key, "; ".join(bad))
        fl = f["flags"]
        Bn, H, W, n_out, n_pad = f["batch"], f["in_h"], f["in_w"], f["n_out"], f["n_pad"]
        Ho, Wo = LR.out_dims(f)
        M = self.M = Bn * Ho * Wo
        seed = zlib.crc32(key.encode()) & 0xFFFF
        geglu = bool(fl & L.F_GEGLU)
        N = 2 * n_out if geglu else (n_pad if f["vt"] else n_out)
        o = self.ops = {}
        r = self.d = L.ConvDesc()
        for n, _ in L.ConvDesc._fields_:
            if n not in LR.POINTERS:
                setattr(r, n, getattr(d, n))

        def act(name, shape, sd, norm=False):
            k = (shape, sd, norm)
            if k not in cache:  # (the launches of a level share their activation shapes)
                cache[k] = R.norm_input(shape, sd, 1, device=DEV) if norm else R.activations(shape, sd, device=DEV)
            o[name] = cache[k]
            return o[name].data_ptr()

        assert f["ld1"] >= f["c1"] and (not f["x2"] or f["ld2"] >= f["c2"])
        r.x1 = act("x1", (Bn, H, W, f["ld1"]), 1, norm=f["ln_colsum"])
        if f["x2"]:
            r.x2 = act("x2", (Bn, H, W, f["ld2"]), 2)
        if f["x3"]:
            assert f["ld3"] >= f["c3"] and (not f["x4"] or f["ld4"] >= f["c4"])
            r.x3 = act("x3", (Bn, Ho, Wo, f["ld3"]), 3)
            if f["x4"]:
                r.x4 = act("x4", (Bn, Ho, Wo, f["ld4"]), 4)
        cin, ks = f["c1"] + f["c2"], f["ksize"]
        w = o["w"] = R.weights((N, cin, ks, ks), ks * ks * cin, seed + 2).to(DEV).contiguous()
        rm = geglu_row_map(n_out).to(DEV) if geglu else None
        wp, npad = ctx.pack_weight(w, row_map=rm)
        assert npad == n_pad, (key, npad, n_pad)
        if f["x3"]:
            w2 = o["w_app"] = R.weights((N, f["c3"] + f["c4"], 1, 1), f["c3"] + f["c4"], seed + 3).to(DEV).contiguous()
            wp2, npad2 = ctx.pack_weight(w2)
            assert npad2 == n_pad
            wp = torch.cat([wp.reshape(-1), wp2.reshape(-1)]).contiguous()  # K order: main then appended
        self.wp = wp
        r.w_packed = wp.data_ptr()
        if f["w_phase"]:
            self.wph, npad3 = _phase_weights(ctx, w)
            assert npad3 == n_pad
            r.w_phase = self.wph.data_ptr()
        if f["pf_next"]:  # (a hint that reads: it gets a buffer of this test's, no longer than that buffer)
            r.pf_next, r.pf_bytes = wp.data_ptr(), min(int(f["pf_bytes"]), wp.numel() * 2)
        packed = lambda v: v[rm.long()] if geglu else v

        def vec_npad(v):
            out = torch.zeros(n_pad, device=DEV)
            out[:N] = packed(v)
            return out

        if f["bias"]:
            o["bias"] = R.vector(N, seed + 4).to(DEV)
            self.bias = vec_npad(o["bias"])
            r.bias = self.bias.data_ptr()
        if f["rowvec"]:
            o["step"] = 2 if f["step"] else 0
            need = o["step"] * f["rv_step_stride"] + (Bn - 1) * f["rv_batch_stride"] + n_pad + 4
            o["rowvec"] = R.vector(need, seed + 5, 1.0).to(DEV)
            r.rowvec = o["rowvec"].data_ptr()
            if f["step"]:
                self.step = torch.tensor([o["step"]], dtype=torch.int32, device=DEV)
                r.step = self.step.data_ptr()
        if f["residual"]:
            assert f["ld_res"] >= n_out
            r.residual = act("residual", (M, f["ld_res"]), 6)
        if f["ln_colsum"]:
            o["ln_colsum"] = w.half().float().sum(dim=(1, 2, 3))  # of the fp16-rounded packed rows
            self.colsum = vec_npad(o["ln_colsum"])
            r.ln_colsum = self.colsum.data_ptr()
        if f["ln_rows_in"]:
            # the producer's buffer [slots][M][2]: per row and column slot the sum and the sum of squares of the fp16 row
            slots = self.slots_in = slots_in
            x = o["x1"][..., :f["c1"]].reshape(M, f["c1"]).to(F64)
            self.rows_in = torch.zeros(8, M, 2, device=DEV)
            for s, part in enumerate(x.tensor_split(slots, dim=1)):
                self.rows_in[s, :, 0], self.rows_in[s, :, 1] = part.sum(1).float(), (part * part).sum(1).float()
            r.ln_rows_in, r.ln_rows_slots = self.rows_in.data_ptr(), slots
        # ---- what the launch writes
        if fl & L.F_OUT_NCHW_F32:
            self.y = torch.full((Bn, n_out, Ho, Wo), FILL, device=DEV)
        else:
            assert f["ldy"] >= n_out
            self.y = torch.full((M, f["ldy"]), FILL, device=DEV, dtype=torch.float32 if fl & L.F_OUT_F32 else torch.float16)
        r.y = self.y.data_ptr()
        if f["vt"]:
            assert M % f["vt_tokens"] == 0 and f["vt_ld"] >= f["vt_tokens"]
            self.vt = torch.full((M // f["vt_tokens"], f["vt_heads"], f["vt_dhead"], f["vt_ld"]), FILL, device=DEV,
                                 dtype=torch.float16)
            r.vt = self.vt.data_ptr()
        if f["gn_stats_ws"]:
            self.sws = torch.full((ctx.gn_stats_floats(Bn, n_pad, f["gn_stats_cap"] or 32),), float("nan"), device=DEV)
            r.gn_stats_ws = self.sws.data_ptr()
        if f["gno_y"]:
            assert f["gno_ld"] >= n_out
            o["gno_gamma"], o["gno_beta"] = (1 + R.vector(n_out, seed + 7, 0.2)).to(DEV), R.vector(n_out, seed + 8).to(DEV)
            self.gno_y = torch.full((M, f["gno_ld"]), FILL, device=DEV, dtype=torch.float16)
            r.gno_gamma, r.gno_beta, r.gno_y = o["gno_gamma"].data_ptr(), o["gno_beta"].data_ptr(), self.gno_y.data_ptr()
        if f["ln_rows_out"]:
            self.rows_out = torch.zeros(8, M, 2, device=DEV)
            r.ln_rows_out = self.rows_out.data_ptr()
        unset = [n for n in LR.POINTERS if bool(getattr(d, n)) != bool(getattr(r, n))]
        assert not unset, "%s: pointer fields the replica did not mirror: %s" % (key, unset)


def worst(got, ref, bound):
    """(ratio, index of the worst element)."""
    q = (got.to(F64) - ref).abs() / bound
    q = torch.where(torch.isfinite(got.to(F64)), q, torch.full_like(q, float("inf")))
    i = int(q.argmax())
    return float(q.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), q.shape))


def check_launch(ctx, plan, d, key, cache):
    """Builds the replica of `d`, launches it once and compares everything it wrote.
    -> (largest ratio, [failures], [what was compared])."""
    lib = ctx.lib
    slots_in = 0
    if d.ln_rows_in:
        # the slot count production runs with is the producer's answer (Emitter.conv run_lnr); a producer that cannot
        # leave the sums makes production take the other program, whose launches are in plan.convs too: one slot then
        prod = [p for p, _ in plan.convs if p.ln_rows_out == d.ln_rows_in]
        assert len(prod) == 1, key
        s = C.c_int(0)
        ctx._chk(lib.upk_conv_ln_rows(ctx.h, C.byref(prod[0]), C.byref(s)))
        slots_in = s.value or 1
    rep = Replica(ctx, d, key, slots_in, cache)
    f, r = rep.f, rep.d
    n_out, n_pad, Bn = f["n_out"], f["n_pad"], f["batch"]
    Ho, Wo = LR.out_dims(f)
    hw = Ho * Wo
    mode, nblk = ctx.conv_gn_fused(r) if (f["gn_stats_ws"] or f["gno_y"]) else (0, 0)
    slots = C.c_int(0)
    if f["ln_rows_out"]:
        ctx._chk(lib.upk_conv_ln_rows(ctx.h, C.byref(r), C.byref(slots)))
    lib.upk_kernel_launches(ctx.h, 1)
    ctx.conv(r)  # (a refusal is a finding: production pinned this configuration)
    kernels = lib.upk_kernel_launches(ctx.h, 0)
    torch.cuda.synchronize()
    name = lib.upk_conv_config_name(d.tune_cfg - 1).decode() if d.tune_cfg > 0 else "cost model"
    if name.startswith("as"):
        splitk = 1  # (A-stationary family: the second slot counts column passes per workgroup)
    elif d.tune_cfg > 0 and d.tune_splitk > 0:
        splitk = d.tune_splitk
    else:
        splitk = 1 if kernels == 1 else LR.SPLITK_MAX  # (a split launch is two kernels; the factor is the library's secret)
    what = "%s [%s, split-K %d%s]" % (key, name, d.tune_splitk, "" if d.tune_cfg else " -> %d kernel(s)" % kernels)
    refs = LR.launch_ref(f, rep.ops, splitk)
    fails, top, done = [], 0.0, []

    def cmp(label, got, ref, bound):
        nonlocal top
        done.append(label)
        assert got.shape == ref.shape, (what, label, got.shape, ref.shape)
        q, at = worst(got, ref, bound)
        top = max(top, q)
        if not q <= 1:
            fails.append("%s: %s ratio %.3g at %s (got %r, ref %r, bound %.3g)" % (
                what, label, q, at, float(got[at]), float(ref[at]), float(bound[at])))

    def untouched(label, t):
        if not bool((t == FILL).all()):
            fails.append("%s: %s was written (%d elements)" % (what, label, int((t != FILL).sum())))

    skip_y = mode == 3 and f["gno_skip_y"]
    if f["flags"] & L.F_OUT_NCHW_F32:
        cmp("y", rep.y, *refs["y"])
    elif skip_y:
        untouched("y (gno_skip_y)", rep.y)
    else:
        cmp("y", rep.y[:, :n_out], *refs["y"])
        untouched("y between n_out and ldy", rep.y[:, n_out:])
    if f["vt"]:
        cmp("vt", rep.vt[..., :f["vt_tokens"]], *refs["vt"])
        untouched("vt past vt_tokens", rep.vt[..., f["vt_tokens"]:])
    by = LR.byproduct_refs(f, rep.ops, None if skip_y else rep.y, refs["y"], gn_mode=mode, gn_nblk=nblk, ln_slots=slots.value,
                           finalize=mode == 2 and nblk > 32)
    if "ln_rows" in by:
        cmp("ln_rows_out", rep.rows_out[:slots.value].to(F64).sum(0), *by["ln_rows"])
    if "gn_part" in by:
        cmp("gn_stats_ws mode 2", rep.sws[:Bn * nblk * 2 * n_pad].reshape(Bn, nblk, 2, n_pad)[..., :n_out], *by["gn_part"])
    if "gn_group" in by:
        g, nch = f["gn_groups"], lib.upk_groupnorm_chunks(hw)
        if mode == 1:
            cmp("gn_stats_ws mode 1", rep.sws[:Bn * nch * g * 2].reshape(Bn, nch, g, 2).to(F64).sum(1), *by["gn_group"])
        else:  # more than 32 row blocks per sample: production folds them with upk_groupnorm_finalize_f32 (Emitter.groupnorm)
            ws = torch.full((ctx.groupnorm_ws_bytes(Bn, hw) // 4 + 64,), float("nan"), device=DEV)
            ctx._chk(lib.upk_groupnorm_finalize_f32(ctx.h, rep.sws.data_ptr(), nblk, n_pad, Bn, hw, n_out, g, ws.data_ptr(),
                                                    ctx._s()))
            torch.cuda.synchronize()
            fin = ws[:Bn * nch * g * 2].reshape(Bn, nch, g, 2)
            cmp("upk_groupnorm_finalize_f32", fin[:, 0], *by["gn_group"])
            if not bool((fin[:, 1:] == 0).all()):
                fails.append("%s: upk_groupnorm_finalize_f32 left something outside chunk 0" % what)
    if "gno_y" in by:
        cmp("gno_y", rep.gno_y[:, :n_out], *by["gno_y"])
        untouched("gno_y between n_out and gno_ld", rep.gno_y[:, n_out:])
    elif f["gno_y"]:
        untouched("gno_y (the launch reported mode %d)" % mode, rep.gno_y)
    return top, fails, done


def pinned_by(key, d, lanes):
    """Which table pinned the launch (Emitter.apply_tuning's order and fall-backs), or 'cost model'."""
    from upgpt_amd.tuning import TUNE_CACHE, TUNE_CACHE_LANES
    if d.tune_cfg == 0:
        return "cost model"
    alts = [key, key[:-3] if key.endswith("_gs") else key + "_gs"] + ([key[:-4]] if key.endswith("_lnr") else [])
    for table, cache in (("lanes table", TUNE_CACHE_LANES),) * (lanes > 1) + (("single-forward table", TUNE_CACHE),):
        for k in alts:
            e = cache.get(k)
            if e is not None and (int(e[0]) + 1, int(e[1])) == (d.tune_cfg, d.tune_splitk):
                return table
    return "a table (entry not traced)"


def launch_class(key, d):
    sfx = re.sub(r"\d+", "", key.split("_r", 1)[1][3:])
    return "k%ds%d f%#x%s" % (d.ksize, d.stride, d.flags, sfx)


def variant(d, key):
    """What makes two entries of plan.convs the same launch: the issue's triple, and the armed by-products on top (the
    key does not name them all), so that nothing two entries differ in goes unchecked."""
    return (key, d.tune_cfg, d.tune_splitk, bool(d.gn_stats_ws), d.gn_stats_cap, bool(d.gno_y), d.gno_silu, d.gno_skip_y,
            bool(d.ln_rows_out), bool(d.ln_rows_in), bool(d.bias), bool(d.pf_next))


def variants(plan):
    return {variant(d, key) for d, key in plan.convs}


def check_plan(ctx, plan, title, lanes, select=lambda d: True, known=None):
    """known: variants checked elsewhere (the single-forward plan's, when `plan` is the same network lowered under
    shared_chip): an entry that repeats one of them is covered by that check and only what differs is launched here —
    which may be nothing."""
    t0 = time.perf_counter()
    seen, triples, peak, fails, cache = set(known or ()), set(), {}, [], {}
    n_known = len(seen)
    tables = {"lanes table": 0, "single-forward table": 0, "cost model": 0}
    compared = {}
    n_sel = 0
    for d, key in plan.convs:
        if not select(d):
            continue
        n_sel += 1
        v = variant(d, key)
        if v in seen:
            continue
        seen.add(v)
        triples.add(v[:3])
        top, bad, done = check_launch(ctx, plan, d, key, cache)
        fails += bad
        for label in done:
            compared[label] = compared.get(label, 0) + 1
        cls = launch_class(key, d)
        peak[cls] = max(peak.get(cls, 0.0), top)
        tab = pinned_by(key, d, lanes)
        tables[tab] = tables.get(tab, 0) + 1
    # coverage: every selected entry is a checked variant, or a repeat of one
    assert all(variant(d, key) in seen for d, key in plan.convs if select(d))
    n_checked = len(seen) - n_known
    assert n_sel > 0 and n_checked >= len(triples) and (len(triples) > 0 or known is not None)
    print("\n%s: %d launches, %d distinct (key, tile configuration, split-K), %d checked (by-product variants apart)%s; "
          "pinned: %s; %.1f s" % (title, n_sel, len(triples), n_checked,
                                  "" if known is None else " = what differs from the single-forward plan's %d" % n_known,
                                  ", ".join("%d by the %s" % (n, t) for t, n in tables.items()), time.perf_counter() - t0))
    print("    compared: " + ", ".join("%s x %d" % kv for kv in sorted(compared.items())))
    print("    %d of the %d launches fall to the cost model" % (sum(d.tune_cfg == 0 for d, _ in plan.convs if select(d)), n_sel))
    for cls in sorted(peak):
        print("    %-40s largest ratio %.3f" % (cls, peak[cls]))
    assert not fails, "%d check(s) failed:\n%s" % (len(fails), "\n".join(fails))
    return n_sel


# ------------------------------------------------------------------------------------------------------------ the plans
@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_unet_plan_launches_against_fp64(ctx, model, H, W, lanes):
    plan = unet_plan(model, H, W, lanes)
    assert (plan.B, plan.H, plan.W, plan.n_ctx, plan.rows) == (B, H, W, NCTX, STEPS)
    n = check_plan(ctx, plan, "UNet %dx%d, %s" % (H, W, "shared_chip(4)" if lanes > 1 else "single forward"), lanes)
    assert n == len(plan.convs)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("h,w", [(32, 32), (32, 24)])
def test_vae_decoder_plan_launches_against_fp64(ctx, model, h, w, level):
    plan = model.first_stage_model._decode_plan(B, h, w, 0.18215)
    rows = lambda d: d.batch * LR.out_dims(LR.fields(d))[0] * LR.out_dims(LR.fields(d))[1]
    by_level = [B * h * w * 4 ** k for k in range(4)]
    assert all(rows(d) in by_level for d, _ in plan.convs), "a launch outside the four resolution levels"
    n = check_plan(ctx, plan, "VAE decoder %dx%d, level %d (M = %d)" % (h, w, level, by_level[level]), 1,
                   select=lambda d: rows(d) == by_level[level])
    assert sum(rows(d) == by_level[level] for d, _ in plan.convs) == n


# ------------------------------------------------------------------------------------------- the plans beyond the headline
# Each is built through the call the product makes (the call site is named), on synthetic weights as bench.py's
# encoders_secondary / upscale_secondary fill them, and never run.
UP_B, UP_NCTX = 4, 86                  # bench.py upscale_secondary: bs = 4, 86 context tokens
UP_LATENTS = [(64, 64), (128, 96)]     # the latent BASELINE words, and the one the upscale config states
N_STYLES = 9                           # style crops per sample (bench.py encoders_secondary; the laion stage's golden)
LPIPS_SIZES = [(256, 176)]             # crop_size of the bbox config: the pictures test_step writes and run_metrics scores


def rows_of(d):
    Ho, Wo = LR.out_dims(LR.fields(d))
    return d.batch * Ho * Wo


def in_lanes(lanes, build):
    if lanes > 1:
        with L.shared_chip(lanes):
            return build()
    return build()


def lanes_title(lanes):
    return "shared_chip(4)" if lanes > 1 else "single forward"


def check_lowerings(ctx, build, title, lanes):
    """lanes = 1: every launch of the plan.  lanes = 4: the same network lowered inside shared_chip(4); only the launches
    whose variant() differs from the single-forward plan's are launched (none is a valid result, and is printed)."""
    single = build() if lanes > 1 else None
    plan = in_lanes(lanes, build)
    assert lanes == 1 or plan is not single
    known = None if single is None else variants(single)
    n = check_plan(ctx, plan, "%s, %s" % (title, lanes_title(lanes)), lanes, known=known)
    if known is not None:
        print("    %d of the %d variants of the shared_chip(4) plan differ from the single-forward plan's" % (
            len(variants(plan) - known), len(variants(plan))))
    return plan, n


def check_levels(ctx, plan, title, levels, level, lanes=1, known=None):
    """One resolution level of a plan: `levels` maps a case name to the row counts it owns; a launch that belongs to no
    case fails every case, so the cases of a plan cover len(plan.convs) together."""
    owned = [m for ms in levels.values() for m in ms]
    assert len(owned) == len(set(owned))
    stray = sorted({rows_of(d) for d, _ in plan.convs} - set(owned))
    assert not stray, "%s: launches of %s rows belong to no case" % (title, stray)
    assert sum(sum(rows_of(d) in ms for d, _ in plan.convs) for ms in levels.values()) == len(plan.convs)
    mine = levels[level]
    n = check_plan(ctx, plan, "%s, %s (M = %s)" % (title, level, " / ".join(str(m) for m in mine)), lanes,
                   select=lambda d: rows_of(d) in mine, known=known)
    assert n == sum(rows_of(d) in mine for d, _ in plan.convs)
    return n


def drop_plans(*modules):
    """Module end: the plans (buffers, packed weights) of the fixtures' modules go, and the allocator's cache with them."""
    from upgpt_amd.plancache import PlanCache
    torch.cuda.synchronize()
    for m in modules:
        for sub in m.modules():
            for v in list(vars(sub).values()):
                if isinstance(v, PlanCache):
                    v.drop(device=DEV)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_guided_unet_plan_launches_against_fp64(ctx, model, H, W, lanes):
    """DDIMSampler._fast_sampling with unconditional guidance: unet.plan(2 b, H, W, n_ctx, S, "sampler"), b = 8."""
    build = lambda: model.model.diffusion_model.plan(2 * B, H, W, NCTX, STEPS, "sampler")
    plan, n = check_lowerings(ctx, build, "guided UNet %dx%d (2B = %d rows)" % (H, W, 2 * B), lanes)
    assert (plan.B, plan.H, plan.W, plan.n_ctx, plan.rows) == (2 * B, H, W, NCTX, STEPS)
    assert n == len(plan.convs)


@pytest.fixture(scope="module")
def upscale_models():
    """{(h, w): the upscale model as bench.py's upscale_secondary builds it}, built on first use."""
    import upgpt_amd
    from upgpt_amd import synth
    made = {}

    def get(hw):
        if hw not in made:
            m = upgpt_amd.build_model("upscale", overrides={"image_size": list(hw)})
            synth.fill_module_(m)
            made[hw] = m.cuda()
        return made[hw]

    yield get
    drop_plans(*made.values())
    made.clear()
    torch.cuda.empty_cache()


def upscale_unet_levels(h, w):
    lv = {"prep": (STEPS, UP_B * UP_NCTX)}  # time embedding / emb_layers rows, and the context k | v projections
    lv.update({"level %d" % k: (UP_B * h * w // 4 ** k,) for k in range(4)})
    return lv


@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("level", ["prep", "level 0", "level 1", "level 2", "level 3"])
@pytest.mark.parametrize("h,w", UP_LATENTS)
def test_upscale_unet_plan_launches_against_fp64(ctx, upscale_models, h, w, level, lanes):
    """DDIMSampler._fast_sampling on the upscale model without guidance (bench.py upscale_secondary):
    unet.plan(4, h, w, 86, 50, "sampler")."""
    unet = upscale_models((h, w)).model.diffusion_model
    build = lambda: unet.plan(UP_B, h, w, UP_NCTX, STEPS, "sampler")
    plan = in_lanes(lanes, build)
    assert (plan.B, plan.H, plan.W, plan.n_ctx, plan.rows, plan.arch.in_channels) == (UP_B, h, w, UP_NCTX, STEPS, 6)
    known = variants(build()) if lanes > 1 else None
    check_levels(ctx, plan, "upscale UNet %dx%d, %s" % (h, w, lanes_title(lanes)), upscale_unet_levels(h, w), level, lanes, known)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_upscale_first_stage_decoder_plan_launches_against_fp64(ctx, upscale_models, level):
    """LatentDiffusion.decode_first_stage of the upscale model: its kl-f4 decoder, 4 x 128x96 -> 512x384."""
    m = upscale_models((128, 96))
    plan = m.first_stage_model._decode_plan(UP_B, 128, 96, float(m.scale_factor))  # (decode_first_stage's sf)
    assert plan.arch.factor == 4
    levels = {k: (UP_B * 128 * 96 * 4 ** k,) for k in range(3)}
    assert levels[2] == (786432,)
    check_levels(ctx, plan, "upscale first-stage decoder 128x96", levels, level)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W", [(256, 256), (256, 192)])
def test_vae_encoder_plan_launches_against_fp64(ctx, model, H, W, level):
    """AutoencoderKL.encode of the bbox model at B = 8 (encode_first_stage: img2img, edit_region, p_losses)."""
    plan = model.first_stage_model._encode_plan(B, H, W)
    levels = {k: (B * H * W // 4 ** k,) for k in range(4)}
    check_levels(ctx, plan, "VAE encoder %dx%d" % (H, W), levels, level)


def synth_stage(module, prefix):
    from upgpt_amd import synth
    module.load_state_dict({k: synth.synth_tensor(prefix + k, tuple(v.shape)) for k, v in module.state_dict().items()})
    return module.cuda()


@pytest.fixture(scope="module")
def towers():
    """The conditioning stages, on the recipe's weights under the checkpoint's names, built on first use:
    'text' FrozenCLIPEmbedder, 'pooled' CLIPTextTower, 'image' FrozenClipImageEmbedder2, 'laion' CLIPTextImageCrossAtten."""
    from upgpt_amd.clip_cross import CLIPTextImageCrossAtten
    from upgpt_amd.clip_image import FrozenClipImageEmbedder2
    from upgpt_amd.clip_text import CLIPTextTower, FrozenCLIPEmbedder
    make = {"text": lambda: synth_stage(FrozenCLIPEmbedder(), "cond_stage_model."),
            "pooled": lambda: synth_stage(CLIPTextTower(), "clip_text_encoder.model."),
            "image": lambda: synth_stage(FrozenClipImageEmbedder2(), "extra_cond_models.0."),
            "laion": lambda: synth_stage(CLIPTextImageCrossAtten(), "cond_stage_model.")}
    made = {}

    def get(name):
        if name not in made:
            made[name] = make[name]()
        return made[name]

    yield get
    drop_plans(*made.values())
    for m in made.values():  # (the laion stage keeps its tower objects outside the module tree)
        for t in getattr(getattr(m, "model", None), "towers", ()):
            drop_plans(t)
    made.clear()
    torch.cuda.empty_cache()


def tower_plan(towers, which):
    """(title, build) of a tower plan; build() is the call the product makes."""
    if which == "text":  # FrozenCLIPEmbedder.encode_tokens -> CLIPTextTransformer._run -> _plan(B)
        return "CLIP text tower B = 8 (hidden states)", lambda: towers("text").transformer._plan(B)
    if which == "pooled":  # CLIPTextTower.encode_text -> _run -> _plan(n)
        return "CLIP text tower B = 8 (pooled)", lambda: towers("pooled")._plan(B)
    if which == "image":  # FrozenClipImageEmbedder2.forward -> encode_image -> CLIPVisual.forward -> _plan(b n)
        return "CLIP image tower N = 72", lambda: towers("image").model.visual._plan(B * N_STYLES)
    if which == "laion text":  # CLIPTextImageCrossAtten._plan: text_tower._plan(B) (hidden_act "gelu": plain fc1 launches)
        return "laion text tower B = 8", lambda: towers("laion").model.text_tower._plan(B)
    assert which == "laion image"  # CLIPTextImageCrossAtten._plan: vision_tower._plan(B n)
    return "laion image tower N = 72", lambda: towers("laion").model.vision_tower._plan(B * N_STYLES)


@pytest.mark.parametrize("which,lanes", [("text", 1), ("text", 4), ("pooled", 1), ("image", 1), ("image", 4), ("laion text", 1),
                                         ("laion image", 1)])
def test_clip_tower_plan_launches_against_fp64(ctx, towers, which, lanes):
    title, build = tower_plan(towers, which)
    plan, n = check_lowerings(ctx, build, title, lanes)
    assert n == len(plan.convs)
    f = [LR.fields(d) for d, _ in plan.convs]
    qkv = [x for x in f if x["vt"]]
    assert qkv and all(x["ln_colsum"] and x["vt_tokens"] % 32 for x in qkv)  # folded LayerNorm, V^T tail, odd token count
    if which == "pooled":
        assert (f[-1]["batch"], f[-1]["in_h"], f[-1]["in_w"]) == (B, 1, 1) and f[-1]["flags"] & L.F_OUT_F32
    if "image" in which:
        assert (qkv[0]["vt_tokens"], qkv[0]["vt_ld"], qkv[0]["vt_heads"], qkv[0]["vt_dhead"]) == (257, 288, 16, 64)
        assert f[0]["c1"] == 608 and f[-1]["batch"] == B * N_STYLES
    if which in ("text", "pooled", "image"):
        assert any(x["ln_colsum"] and x["flags"] & L.F_QUICKGELU for x in f)


def test_cross_stage_plan_launches_against_fp64(ctx, towers):
    """CLIPTextImageCrossAtten._plan(8, 9): to_q over the 8 x 77 text rows, to_k | to_v over the 72 feature rows, to_out."""
    text_plan, image_plan, plan = towers("laion")._plan(B, N_STYLES)
    n = check_plan(ctx, plan, "cross stage B = 8, n = 9", 1)
    assert n == len(plan.convs) == 3
    assert sorted(rows_of(d) for d, _ in plan.convs) == [B * N_STYLES, B * 77, B * 77]
    assert text_plan is towers("laion").model.text_tower._plan(B)  # (the towers' plans: the two laion cases above)
    assert image_plan is towers("laion").model.vision_tower._plan(B * N_STYLES)


@pytest.fixture(scope="module")
def lpips_net():
    from upgpt_amd import synth
    from upgpt_amd.lpips import LPIPS
    net = LPIPS()
    net.load_state_dict(synth.synthetic_lpips_state(0))
    net = net.cuda()
    yield net
    drop_plans(net)


@pytest.mark.parametrize("H,W", LPIPS_SIZES)
def test_lpips_plan_launches_against_fp64(ctx, lpips_net, H, W):
    """LPIPS._layers -> _plan(pairs, h, w): per pair thirteen 3x3 launches at batch 2, none pinned (LpipsPlan never calls
    apply_tuning): each keeps the SPLITK_MAX bound when the library splits it."""
    plan = lpips_net._plan(1, H, W)
    n = check_plan(ctx, plan, "LPIPS one pair of %dx%d" % (H, W), 1)
    assert n == len(plan.convs) == 13
    assert all(d.tune_cfg == 0 and d.batch == 2 and d.ksize == 3 for d, _ in plan.convs)


# --------------------------------------------------- the branches of the harness that no plan takes with today's tables
@pytest.mark.parametrize("hw,cin,cout,cap,want", [((64, 64), 64, 128, 64, "upk_groupnorm_finalize_f32"),
                                                  ((8, 8), 896, 896, 0, "y")])
def test_harness_on_cost_model_launches(ctx, hw, cin, cout, cap, want):
    """Every launch of the six headline plans is pinned by a table and none leaves more than 32 row blocks of GroupNorm
    partials, so two hand-made descriptors take check_launch through what those plans leave idle: tune_cfg = 0 (the split-K
    factor read off the kernel count) and gn_stats_cap > 32 followed by upk_groupnorm_finalize_f32.  (The upscale UNet's
    level 0 and the LPIPS / cross-stage plans reach both by themselves; these two stay as the harness's own cases.)  The
    pointers only say 'set': the replica replaces every one of them."""
    d = L.ConvDesc()
    d.x1 = d.w_packed = d.y = d.bias = d.gn_stats_ws = 1
    d.c1 = d.ld1 = cin
    d.batch, (d.in_h, d.in_w), d.ksize, d.stride = 2, hw, 3, 1
    d.n_out = d.n_pad = d.ldy = cout
    d.gn_groups, d.gn_stats_cap = 32, cap
    top, fails, done = check_launch(ctx, None, d, "hand-made %dx%d %d->%d" % (*hw, cin, cout), {})
    print("\nhand-made cost-model launch %dx%d %d -> %d: compared %s, largest ratio %.3f" % (*hw, cin, cout, done, top))
    assert not fails, fails
    assert want in done


# ------------------------------------------------------------------- the row-chain kernels at the production row count
@pytest.mark.parametrize("lanes", [1, 4], ids=["single", "shared_chip4"])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 24)])
def test_row_chain_kernels_at_the_production_row_count(ctx, model, H, W, lanes):
    """upk_head_block_f16 / upk_cross_block_f16 / upk_geglu_mlp_f16 of the 32x32-level transformer blocks: M = 8 H W rows at
    the tile height the plan's descriptors carry (under shared_chip(4) the lanes table's __row_chain_rows__ / __mlp_rows__
    choose it), on range_ref's operands against range_ref's fp64 references.  The other tests of these kernels stop at a few
    hundred rows: an m / 128 grid of two or four workgroups."""
    from upgpt_amd.tuning import TUNE_CACHE_LANES
    plan = unet_plan(model, H, W, lanes)
    hw, M = H * W, B * H * W
    kinds = {L.HblockDesc: "hblock", L.XblockDesc: "xblock", L.MlpDesc: "mlp"}
    found = {}
    for k in plan.body.keep:
        if type(k) in kinds and k.m == M and k.c == 224:
            found.setdefault((kinds[type(k)], k.rows_per_wg), k)
    print("\nrow-chain launches at M = %d (%s): %s" % (M, "shared_chip(4)" if lanes > 1 else "single forward",
                                                        sorted(found) or "none in this plan"))
    if lanes > 1:  # what the table stores for this row count must be what the plan runs
        meta = TUNE_CACHE_LANES.meta
        want = {(k, int(v[str(M)])) for k, v in meta.get("__row_chain_rows__", {}).items() if str(M) in v}
        if str(M) in meta.get("__mlp_rows__", {}):
            r = int(meta["__mlp_rows__"][str(M)])
            want.add(("mlp", r | (L.MLP_STREAM if r == 128 else 0)))
        assert want <= set(found), (want, sorted(found))
        assert (H, W) != (32, 32) or len(want) == 3, want
    for (kind, rows), d in sorted(found.items()):
        assert d.hw == hw
        if kind == "hblock":
            o = R.head_case(1, B=B, hw=hw)
            t0o, got_qk, got_v = launch_head_block(ctx, o, rows)
            (t0, dt0), (qkv, dqkv) = R.head_case_ref(o)
            inner = R.HEADS * R.DH
            assert report("head block t0, M %d rows %d" % (M, rows), 1, R.ratio(t0o, t0, dt0)) <= 1
            assert report("head block q | k", 1, R.ratio(got_qk, qkv[:, :2 * inner], dqkv[:, :2 * inner])) <= 1
            assert report("head block v", 1, R.ratio(got_v, qkv[:, 2 * inner:], dqkv[:, 2 * inner:])) <= 1
        elif kind == "xblock":
            assert (d.n_kv, d.vt_ld) == (NCTX, 96)
            o = R.cross_case(1, B=B, hw=hw, nkv=NCTX)
            ref, bound = R.cross_case_ref(o)
            assert report("cross block, M %d rows %d" % (M, rows), 1, R.ratio(launch_cross_block(ctx, o, rows), ref, bound)) <= 1
        else:
            tile = rows & ~L.MLP_STREAM or 64
            o = R.mlp_case("production", 1, B=B, hw=hw, rows=tile)
            if not d.gn_stats_ws:
                o["hw"] = 0  # (the plan's launch leaves no GroupNorm partials)
            check_mlp_tail(o, *launch_mlp_tail(ctx, o, rows), "mlp tail, M %d rows_per_wg %#x" % (M, rows), 1)
