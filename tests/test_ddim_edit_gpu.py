"""DDIM editing on the captured-graph path on a real MI355X: upk_ddim_step_edit_f32 through the C ABI against its fp64
restatement (tests/edit_ref.py), and the sampler calls built on it — sample(mask=, x0=), decode, log_images(inpaint=True)
— against the step-by-step general path, the reference's goldens and the CPU oracle; that they replay captured graphs
(no apply_model call, no new graph or upload on a repeat), on any lane, and that close() releases what they hold.

Bounds: a launch is held to |got - ref64| <= 32 * 2^-24 * A (oracle/steps.py; edit_ref.py extends A by the blend's two
products); runs that differ only in plan and tile choice to the project's mse < 1e-4 (test_model_gpu.py), runs against
the reference's goldens and the oracle to its mse < 1e-3."""
import os

import numpy as np
import pytest
import torch

import edit_ref as er
import upgpt_amd
from oracle import ddim as o_ddim
from oracle import schedule as o_sched
from oracle import steps as st
from oracle import unet as o_unet
from test_sampler_steps_gpu import LD, Guarded, _bits, _make_xin, _nhwc
from upgpt_amd import _lib as L
from upgpt_amd import synth
from upgpt_amd.ddim import DDIMSampler

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
HW = (32, 24)
_cache = {}


def get_model(kind):
    if kind not in _cache:
        m = upgpt_amd.build_model(kind)
        sd = synth.fill_module_(m)
        _cache[kind] = (m.cuda(), sd)
    return _cache[kind]


def mse(a, b):
    return float(((a.float().cpu() - torch.as_tensor(b).float().cpu()) ** 2).mean())


# ---------------------------------------------------------------------------------------------------- the kernel itself
def _upload(inp, mode):
    kw = er.operands(inp, mode)
    B, C, H, W = inp["shape"]
    n, Gd = inp["n"], inp["n"] + 256
    d = {"x": Guarded(inp["x"], Gd), "coefs": Guarded(inp["coefs"], Gd), "eps": Guarded(kw["eps"], Gd),
         "done": Guarded(torch.zeros(1, dtype=torch.int32), 64)}
    for k in ("noise", "keep", "mask"):
        if kw[k] is not None:
            d[k] = Guarded(kw[k], Gd)
    if mode["pred"]:
        d["pred"] = Guarded(torch.full(inp["shape"], 5.0), Gd)
    if mode["plain"]:
        d["plain"] = Guarded(torch.full(inp["shape"], 7.0), Gd)
    if mode["xin"]:
        d["xin"] = Guarded(_make_xin(B * H * W * (2 if mode["cfg"] else 1), C, n), Gd)
    if mode["step"] is not None:
        d["step"] = Guarded(torch.tensor([mode["step"]], dtype=torch.int32), 64)
    return d, kw


def _launch(ctx, d, mode, inp, step_t):
    B, C, H, W = inp["shape"]
    p = lambda k: d[k].live if k in d else None
    ctx.ddim_step_edit(p("x"), p("eps"), p("coefs"), p("noise"), p("keep"), p("mask"), inp["rows"], step_t, p("pred"),
                       p("plain"), p("xin"), LD, B, C, H * W, er.SCALE, mode["cfg"])


def _check_launch(ctx, inp, mode):
    B, C, H, W = inp["shape"]
    hw = H * W
    d, kw = _upload(inp, mode)
    ref = er.ddim_step_edit(**kw)
    for b in d.values():
        b.snapshot()
    torch.cuda.synchronize()
    ctx.step_autoadvance(d["done"].live)
    try:
        _launch(ctx, d, mode, inp, d["step"].live if "step" in d else None)
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    tag = (inp["shape"], mode)
    assert int(d["done"].live.item()) == 0, tag
    if "step" in d:
        assert int(d["step"].live.item()) == mode["step"] + 1, tag
    x = d["x"].live
    assert bool(st.within(x, ref.x, ref.A["x"]).all()), tag
    if "pred" in d:
        assert bool(st.within(d["pred"].live, ref.pred_x0, ref.A["pred_x0"]).all()), tag
    if "plain" in d:
        assert bool(st.within(d["plain"].live, ref.x_plain, ref.A["x_plain"]).all()), tag
        row = mode["step"] or 0
        if not mode["mask"] or row == inp["rows"] - 1:  # nothing blended: x IS the unblended value
            assert torch.equal(_bits(d["plain"].live), _bits(x)), tag
        else:  # the mask's zeros keep x_prev, its ones take the keep row bit for bit
            mk = d["mask"].live.reshape(x.shape)
            assert torch.equal(_bits(x[mk == 0]), _bits(d["plain"].live[mk == 0])), tag
            assert torch.equal(_bits(x[mk == 1]), _bits(d["keep"].live[row + 1].reshape(x.shape)[mk == 1])), tag
    if "xin" in d:
        xin, was = d["xin"].live, d["xin"].live_before()
        assert torch.equal(_bits(xin[:, C:]), _bits(was[:, C:])), tag  # static concat channels and pad
        lat = xin[:B * hw, :C]
        want = _nhwc(ref.xin, B, C, hw)
        tol = st.BOUND * _nhwc(ref.A["xin"], B, C, hw) + 2.0 ** -11 * want.abs() + 2.0 ** -25  # + the fp16 rounding
        assert bool(((lat.double().cpu() - want).abs() <= tol).all()), tag
        assert torch.equal(_bits(lat), _bits(_nhwc(x, B, C, hw).half())), tag  # .half() of the x the kernel wrote
        if mode["cfg"]:
            assert torch.equal(_bits(xin[B * hw:, :C]), _bits(lat)), tag  # both halves refreshed identically
    for name, b in d.items():
        assert b.guards_intact(), tag + (name,)
    for name in ("eps", "coefs", "noise", "keep", "mask"):
        if name in d:
            assert d[name].unchanged(), tag + (name,)


@pytest.mark.parametrize("shape", st.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edit_step_single_launch_parity(ctx, shape):
    inp = er.make_inputs(shape)
    for mode in er.modes():
        _check_launch(ctx, inp, mode)


def test_edit_step_refuses_a_mask_without_keep_rows(ctx):
    inp = er.make_inputs(st.SHAPES[2])
    mode = dict(cfg=False, noise=False, mask=True, plain=True, step=0, pred=True, xin=True)
    d, _ = _upload(inp, mode)
    del d["keep"]
    for b in d.values():
        b.snapshot()
    with pytest.raises(L.UpkError) as ei:
        _launch(ctx, d, mode, inp, d["step"].live)
    torch.cuda.synchronize()
    assert ei.value.code == -1 and all(b.unchanged() for b in d.values())


def test_edit_step_counter_armed_disarmed_null(ctx):
    inp = er.make_inputs(st.SHAPES[2])  # two workgroups, the second ragged
    mode = dict(cfg=True, noise=True, mask=True, plain=True, step=3, pred=True, xin=True)
    d, _ = _upload(inp, mode)
    step, done = d["step"].live, d["done"].live
    seen = []
    for armed, with_step, advance in ((True, True, False), (False, True, False), (False, True, True), (True, False, False),
                                      (True, True, False)):
        ctx.step_autoadvance(done if armed else None)
        try:
            _launch(ctx, d, mode, inp, step if with_step else None)
        finally:
            ctx.step_autoadvance(None)
        if advance:  # disarmed, the separate increment kernel does it
            ctx.advance_step(step)
        torch.cuda.synchronize()
        seen.append((int(step.item()), int(done.item())))
    assert seen == [(4, 0), (4, 0), (5, 0), (5, 0), (6, 0)]
    assert all(b.guards_intact() for b in d.values())


# ------------------------------------------------------------------------------------------------- the sampler calls
def _case(kind, B, S, seed=5):
    inp = synth.synth_inputs(B, HW, 4, 87, 768, seed=seed, steps=S)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    x0 = (0.7 * synth.synth_inputs(B, HW, 4, 87, 768, seed=seed + 1)["x_T"]).cuda()
    mask = (synth.person_mask(B, *HW) > 0.5).float().cuda()
    return inp, cond, uc, x0, mask


def _general(monkeypatch):
    monkeypatch.setattr(DDIMSampler, "_fast_ok", lambda self, *a, **k: False)


def _count_apply_model(model, monkeypatch):
    calls = []
    orig = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    return calls


def _same_run(a, b, what):
    (za, ia, ra), (zb, ib, rb) = a, b
    for k in ("x_inter", "pred_x0"):
        assert len(ia[k]) == len(ib[k]), (what, k)
        for j, (u, v) in enumerate(zip(ia[k], ib[k])):
            e = mse(u, v)
            print("%s %s[%d]: mse fast vs general %.3e" % (what, k, j, e))
            assert e < 1e-4, (what, k, j, e)
    e = mse(za, zb)
    print("%s: final latent mse fast vs general %.3e" % (what, e))
    assert e < 1e-4 and torch.isfinite(za).all(), (what, e)
    assert torch.equal(ra, rb), what + ": the device generator ends elsewhere"


@pytest.mark.parametrize("kind,B", [("tiny", 2), ("bbox", 1)])
def test_masked_sample_and_decode_equal_the_general_path(kind, B, monkeypatch):
    model, _ = get_model(kind)
    S = 10
    inp, cond, uc, x0, mask = _case(kind, B, S)
    x_T = inp["x_T"].cuda()

    def sample(eta, guided):
        torch.manual_seed(123)
        kw = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc) if guided else {}
        z, inter = DDIMSampler(model).sample(S, B, (4,) + HW, cond, eta=eta, x_T=x_T, mask=mask, x0=x0, verbose=False,
                                             log_every_t=3, **kw)
        return z, inter, torch.cuda.get_rng_state()

    def decode(guided):
        torch.manual_seed(321)
        s = DDIMSampler(model)
        s.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        kw = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc) if guided else {}
        z = s.decode(x_T, cond, 6, **kw)
        return z, {"x_inter": [], "pred_x0": []}, torch.cuda.get_rng_state()

    runs = [("sample eta=%g guided=%d" % (e, g), lambda e=e, g=g: sample(e, g)) for e in (0.0, 1.0) for g in (0, 1)]
    runs += [("decode guided=%d" % g, lambda g=g: decode(g)) for g in (0, 1)]
    calls = _count_apply_model(model, monkeypatch)
    fast = [fn() for _, fn in runs]
    assert not calls, "the fast path called apply_model"
    assert len(fast[0][1]["x_inter"]) == 5  # x_T and the DDIM indices 9 (the first step), 6, 3, 0
    _general(monkeypatch)
    slow = [fn() for _, fn in runs]
    assert len(calls) == 4 * S + 2 * 6
    for (what, _), a, b in zip(runs, fast, slow):
        _same_run(a, b, kind + " " + what)
    assert mse(fast[0][0], fast[2][0]) > 1e-4  # eta does change the result ...
    assert mse(fast[0][0], fast[1][0]) > 1e-6  # ... and so does guidance


def test_shortened_timesteps_and_watched_steps_equal_the_general_path(monkeypatch):
    """ddim_sampling(timesteps=) is the start-row mechanism too; callbacks end a graph and see every step; x_inter holds
    the unblended values."""
    model, _ = get_model("tiny")
    B, S = 2, 10
    inp, cond, uc, x0, mask = _case("tiny", B, S, seed=8)
    x_T = inp["x_T"].cuda()

    def run(**kw):
        torch.manual_seed(9)
        s = DDIMSampler(model)
        s.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        seen = []
        z, inter = s.ddim_sampling(cond, (B, 4) + HW, x_T=x_T, log_every_t=2, callback=lambda i: seen.append(i),
                                   img_callback=lambda p, i: seen.append(tuple(p.shape)), **kw)
        return (z, inter, torch.cuda.get_rng_state()), seen

    calls = _count_apply_model(model, monkeypatch)
    fast = [run(timesteps=7), run(timesteps=7, mask=mask, x0=x0), run(mask=mask, x0=x0)]
    assert not calls
    _general(monkeypatch)
    slow = [run(timesteps=7), run(timesteps=7, mask=mask, x0=x0), run(mask=mask, x0=x0)]
    for i, (a, b) in enumerate(zip(fast, slow)):
        assert a[1] == b[1] and len(a[1]) == 2 * (6 if i < 2 else S), i  # int(0.7 * 10) - 1 = 6 steps
        _same_run(a[0], b[0], "ddim_sampling case %d" % i)


def test_goldens_of_the_reference_through_the_graph_path(monkeypatch):
    """blend/z and dec/x_dec (tiny model, dict conditioning) and xattn/x_dec_cfg (crossattn model, tensor conditioning,
    guided decode) of tests/golden/extra.npz, with apply_model never called."""
    g = np.load(os.path.join(G, "extra.npz"))
    model, _ = get_model("tiny")
    B, S = 2, 10
    inp, cond, _, x0, mask = _case("tiny", B, S)
    calls = _count_apply_model(model, monkeypatch)
    feed = iter(inp["noise"])
    q_orig = type(model).q_sample
    monkeypatch.setattr(model, "q_sample", lambda x_start, t, noise=None: q_orig(model, x_start, t, next(feed).cuda()),
                        raising=False)
    with model.ema_scope():
        z, _ = DDIMSampler(model).sample(S, B, (4,) + HW, cond, eta=0.0, x_T=inp["x_T"].cuda(), mask=mask, x0=x0,
                                         verbose=False)
    assert mse(z, g["blend/z"]) < 1e-3
    sampler = DDIMSampler(model)
    sampler.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
    with model.ema_scope():
        x_dec = sampler.decode(inp["x_T"].cuda(), cond, 6)
    assert mse(x_dec, g["dec/x_dec"]) < 1e-3
    assert not calls
    unet_cfg = dict(synth.TINY_UNET)
    unet_cfg["in_channels"] = 4
    xm = upgpt_amd.build_model("tiny", overrides={
        "conditioning_key": "crossattn", "concat_key": None, "extra_cond_stages": None,
        "unet_config": {"target": "upgpt_amd.unet.UNetModel", "params": unet_cfg}})
    synth.fill_module_(xm)
    xm = xm.cuda()
    xcalls = _count_apply_model(xm, monkeypatch)
    xi = synth.synth_inputs(B, HW, 4, 77, 768, seed=9)
    c, start = xi["c_crossattn"].cuda(), xi["x_T"].cuda()
    uc = (0.1 * synth.synth_inputs(B, HW, 4, 77, 768, seed=10)["c_crossattn"]).cuda()
    sampler = DDIMSampler(xm)
    sampler.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
    with xm.ema_scope():
        x_dec = sampler.decode(start, c, 6, unconditional_guidance_scale=2.5, unconditional_conditioning=uc)
    assert mse(x_dec, g["xattn/x_dec_cfg"]) < 1e-3
    assert not xcalls


def test_guided_masked_sampling_vs_the_cpu_oracle(monkeypatch):
    """Dict conditioning, guidance scale 3, mask: oracle.ddim.ddim_sample with mask, x0, q_sample and its uncond branch
    (two passes), both sides fed the same q_sample noise."""
    model, sd = get_model("tiny")
    B, S = 2, 5
    inp = synth.synth_inputs(B, HW, 4, 87, 768, seed=13, steps=S)
    cond = {"c_crossattn": inp["c_crossattn"], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": torch.zeros_like(inp["c_crossattn"]), "c_concat": [inp["c_concat"]]}
    x0 = 0.7 * synth.synth_inputs(B, HW, 4, 87, 768, seed=14)["x_T"]
    mask = (synth.person_mask(B, *HW) > 0.5).float()
    acp = o_sched.ddpm_tables(o_sched.linear_betas(1000, 0.00085, 0.012))["alphas_cumprod"]
    eps_fn = lambda x, t, c: o_unet.diffusion_wrapper(sd, synth.TINY_UNET, x, t, c["c_concat"], c["c_crossattn"])
    z_ref, _ = o_ddim.ddim_sample(eps_fn, acp, (B, 4) + HW, S, 0.0, inp["x_T"].clone(), cond=cond, uncond=uc,
                                  guidance_scale=3.0, mask=mask, x0=x0, q_sample=er.q_sample_fn(acp, inp["noise"]))
    dev = lambda d: {"c_crossattn": d["c_crossattn"].cuda(), "c_concat": [d["c_concat"][0].cuda()]}
    calls = _count_apply_model(model, monkeypatch)
    feed = iter(inp["noise"])
    q_orig = type(model).q_sample
    monkeypatch.setattr(model, "q_sample", lambda x_start, t, noise=None: q_orig(model, x_start, t, next(feed).cuda()),
                        raising=False)
    z, _ = DDIMSampler(model).sample(S, B, (4,) + HW, dev(cond), eta=0.0, x_T=inp["x_T"].cuda(), verbose=False,
                                     mask=mask.cuda(), x0=x0.cuda(), unconditional_guidance_scale=3.0,
                                     unconditional_conditioning=dev(uc))
    assert not calls
    e = mse(z, z_ref)
    print("guided masked sampling vs the CPU oracle: mse %.3e" % e)
    assert e < 1e-3


def test_a_repeat_captures_no_graph_and_uploads_no_schedule(monkeypatch):
    model, _ = get_model("tiny")
    B, S = 2, 10
    inp, cond, uc, x0, mask = _case("tiny", B, S, seed=17)
    x_T = inp["x_T"].cuda()
    unet = model.model.diffusion_model
    sampler = DDIMSampler(model)

    def both():
        za, _ = sampler.sample(S, B, (4,) + HW, cond, eta=0.0, x_T=x_T, mask=mask, x0=x0, verbose=False)
        zb = sampler.decode(x_T, cond, 6)
        zc, _ = sampler.sample(S, B, (4,) + HW, cond, eta=0.0, x_T=x_T, mask=mask, x0=x0, verbose=False,
                               unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        return za, zb, zc

    def state():
        out = []
        for (_, pb, *_rest), plan in unet._plans.items():
            for guided in (False, True):
                s_ = plan.sampler_states.get(("ddim", guided))
                if s_ is not None:
                    out.append((guided, pb, dict(s_.graphs), getattr(s_, "_coef_key", None),
                                getattr(plan, "_t_rows_key", None), None if s_.keep is None else s_.keep.data_ptr()))
        return out

    torch.manual_seed(5)
    first = both()
    before = state()
    # (a graph's key ends in the step variant it was captured for: engine.SamplerState.graph)
    assert any(k[-1] == "masked" for _, _, gs, *_ in before for k in gs)
    assert any(k[-1] == "plain" for _, _, gs, *_ in before for k in gs)
    begins = []
    lib = L.get_context(0).lib
    orig = lib.upk_graph_begin
    monkeypatch.setattr(lib, "upk_graph_begin", lambda *a: (begins.append(1), orig(*a))[1], raising=False)
    uploads = []
    table = upgpt_amd.ddim.ddim_coefficient_table
    monkeypatch.setattr(upgpt_amd.ddim, "ddim_coefficient_table", lambda *a: (uploads.append(1), table(*a))[1])
    torch.manual_seed(5)
    second = both()
    assert not begins and not uploads
    after = state()
    assert len(after) == len(before)
    for a, b in zip(before, after):
        assert a[:2] == b[:2] and a[2] == b[2] and a[3] is b[3] and a[4] is b[4] and a[5] == b[5]
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def _batch(B, seed=3):
    g0 = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
            "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
            "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}


@pytest.mark.parametrize("guided", [False, True])
def test_log_images_inpaint_runs_on_the_graph_path(guided, monkeypatch):
    model, _ = get_model("tiny")
    B = 2
    batch = _batch(B)
    kw = dict(unconditional_guidance_scale=3., unconditional_guidance_label=[""]) if guided else {}

    def run():
        torch.manual_seed(31)
        return model.log_images(batch, N=B, ddim_steps=10, ddim_eta=1.0, inpaint=True, **kw)

    calls = _count_apply_model(model, monkeypatch)
    fast = run()
    assert not calls
    _general(monkeypatch)
    slow = run()
    assert calls
    assert {"samples", "samples_inpainting", "samples_outpainting", "mask"} <= set(fast)
    assert fast["mask"].shape == (B, 1, 32, 24) and torch.equal(fast["mask"], slow["mask"])
    for k in ("samples", "samples_inpainting", "samples_outpainting"):
        assert fast[k].shape == (B, 3, 256, 192) and torch.isfinite(fast[k]).all(), k
        e = mse(fast[k], slow[k])
        print("log_images(inpaint=True, guided=%d) %s: image mse fast vs general %.3e" % (guided, k, e))
        assert e < 1e-4, (k, e)
    assert not torch.equal(fast["samples_inpainting"], fast["samples_outpainting"])  # (a second draw of the same task)


def test_a_masked_chain_on_another_lane_is_bit_identical(monkeypatch):
    from upgpt_amd.lanes import LanePool
    model, _ = get_model("tiny")
    B, S, lanes = 2, 10, 2
    inp, cond, uc, x0, mask = _case("tiny", B, S, seed=23)
    x_T = inp["x_T"].cuda()
    # q_sample's noise by timestep: the lanes share the device generator, so its draws are no basis for a comparison
    ts = synth.synth_inputs(B, HW, 4, 87, 768, seed=24, steps=S)["noise"].cuda()
    steps = sorted(int(t) for t in upgpt_amd.schedule.make_ddim_timesteps("uniform", S, 1000, verbose=False))
    table = {t: ts[i] for i, t in enumerate(steps)}
    q_orig = type(model).q_sample
    monkeypatch.setattr(model, "q_sample", lambda x_start, t, noise=None: q_orig(model, x_start, t, table[int(t[0])]),
                        raising=False)
    seen = []

    def step(k):
        seen.append((k, L.current_lane()))
        s = DDIMSampler(model)
        with model.ema_scope():
            z, inter = s.sample(S, B, (4,) + HW, cond, eta=0.0, x_T=x_T, mask=mask, x0=x0, verbose=False, log_every_t=4,
                                unconditional_guidance_scale=3.0 if k % 2 else 1.0,
                                unconditional_conditioning=uc if k % 2 else None)
        return z, inter["x_inter"][-2]

    K = 2 * lanes
    with L.shared_chip(lanes):
        serial = [step(k) for k in range(K)]
    torch.cuda.synchronize()
    with LanePool(lanes) as pool:
        for rep in range(2):
            outs = pool.run(step, K)
            torch.cuda.synchronize()
            for k, (a, b) in enumerate(zip(serial, outs)):
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "step %d (lane %d)" % (k, k % lanes)
    assert sorted(seen) == sorted([(k, 0) for k in range(K)] + [(k, k % lanes) for k in range(K)] * 2)


def test_close_and_eviction_release_the_edit_buffers(monkeypatch):
    model, _ = get_model("tiny")
    B, S = 2, 5  # (a divisor of 1000: the uniform schedule has exactly S steps)
    inp, cond, _, x0, mask = _case("tiny", B, S, seed=29)
    x_T = inp["x_T"].cuda()
    unet = model.model.diffusion_model
    feed_noise = inp["noise"].cuda()
    q_orig = type(model).q_sample

    def run():
        feed = iter(feed_noise)
        monkeypatch.setattr(model, "q_sample", lambda x_start, t, noise=None: q_orig(model, x_start, t, next(feed)),
                            raising=False)
        return DDIMSampler(model).sample(S, B, (4,) + HW, cond, eta=0.0, x_T=x_T, mask=mask, x0=x0, verbose=False)[0]

    z1 = run()
    plan = unet.plan(B, HW[0], HW[1], 87, S, "sampler")
    state = plan._sampler_state
    assert state.keep is not None and tuple(state.keep.shape) == (S, B * 4 * HW[0] * HW[1])
    assert state.edit_mask is not None and state.x_plain is not None and state.graphs
    plan.close()
    assert state.keep is None and state.edit_mask is None and state.x_plain is None and not state.graphs
    assert not hasattr(plan, "_sampler_state")
    z2 = run()  # a fresh state on the same plan
    assert torch.equal(z1, z2) and plan._sampler_state is not state
    # eviction: the plan leaves the cache the way UNetModel.plan drops its oldest one
    key = next(k for k, p in unet._plans.items() if p is plan)
    state = plan._sampler_state
    unet._plans.pop(key).close()
    assert state.keep is None and not state.graphs
    assert torch.equal(run(), z1)
