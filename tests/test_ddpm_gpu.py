"""The DDPM ancestral sampler (LatentDiffusion.p_sample_loop / progressive_denoising / sample / p_sample and the DDPM
and plotting branches of log_images) on the MI355X, against the reference's own runs (tests/golden/ddpm.npz, made by
tests/golden/make_ddpm_golden.py with the recipe weights and the recipe noise) and against itself: fused captured-graph
chain vs the step-by-step path, graph grouping, lanes, generator consumption, callbacks."""
import os

import numpy as np
import pytest
import torch

import upgpt_amd
from upgpt_amd import ddim as ddim_mod
from upgpt_amd import ddpm as ddpm_mod
from upgpt_amd import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
HW, C, NTOK = (32, 24), 4, 87
_cache = {}


def get_model(kind, ema_salt=None):
    key = (kind, ema_salt)
    if key not in _cache:
        m = upgpt_amd.build_model(kind)
        synth.fill_module_(m)
        if ema_salt is not None:
            synth.fill_ema_(m, salt=ema_salt)
        _cache[key] = m.cuda()
    return _cache[key]


def golden():
    return np.load(os.path.join(G, "ddpm.npz"))


def inputs(B, seed, T):
    inp = synth.synth_inputs(B, HW, C, NTOK, 768, seed=seed, steps=T)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    return inp, cond


def mse(a, b):
    return float(((torch.as_tensor(a).float().cpu() - torch.as_tensor(b).float().cpu()) ** 2).mean())


def pool2(x):
    """The stored form of the logged intermediates (make_ddpm_golden.py): 2x2 average pooling."""
    return torch.nn.functional.avg_pool2d(x.float(), 2)


def centre_mask(B):
    mask = torch.ones(B, *HW)
    h, w = HW
    mask[:, h // 4:3 * h // 4, w // 4:3 * w // 4] = 0.
    return mask[:, None]


def test_full_chain_vs_reference():
    """Golden item 1: tiny, B = 2, the full 1000-step chain, intermediates every 200 steps.  Measured on the MI355X:
    final latent MSE 1.2e-4, growing steadily along the chain (2x2-pooled intermediates: 1.2e-6 at t = 600, 2.1e-5 at
    t = 200); bound 1e-3, the DDIM goldens' bound."""
    g = golden()
    m = get_model("tiny")
    inp, cond = inputs(2, 40, 1000)
    z, inter = m.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(), verbose=False,
                               log_every_t=200, normals_sequence=inp["noise"])
    ref = g["chain/inter_pool2"]
    assert len(inter) == ref.shape[0] == 7
    errs = [mse(pool2(a), b) for a, b in zip(inter, ref)]
    print("chain MSE final %.3e, intermediates %s" % (mse(z, g["chain/z"]), ["%.1e" % e for e in errs]))
    assert mse(z, g["chain/z"]) < 1e-3 and max(errs) < 1e-3, errs


def test_progressive_denoising_vs_reference():
    """Golden item 2: progressive_denoising(start_T=200, temperature=0.7): the x0 intermediates."""
    g = golden()
    m = get_model("tiny")
    inp, cond = inputs(2, 41, 200)
    z, inter = m.progressive_denoising(cond, (C,) + HW, verbose=False, batch_size=2, x_T=inp["x_T"].cuda(),
                                       start_T=200, temperature=0.7, log_every_t=50, normals_sequence=inp["noise"])
    ref = g["prog/inter_pool2"]
    assert len(inter) == ref.shape[0]
    errs = [mse(pool2(a), b) for a, b in zip(inter, ref)]
    assert mse(z, g["prog/z"]) < 1e-3 and max(errs) < 1e-3, errs


def _mask_case():
    inp, cond = inputs(2, 42, 200)
    q = synth.synth_inputs(2, HW, C, NTOK, 768, seed=43, steps=200)
    x0 = 0.18215 * 4.0 * q["x_T"]
    normals = torch.stack([inp["noise"], q["noise"]], 1).reshape(400, 2, C, *HW)  # posterior, q_sample per step
    return inp, cond, x0, normals


def test_masked_chain_vs_reference():
    """Golden item 3: p_sample_loop(timesteps=200) with the centre-square mask and x0 (q_sample blend every step)."""
    g = golden()
    m = get_model("tiny")
    inp, cond, x0, normals = _mask_case()
    z, inter = m.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(), verbose=False,
                               timesteps=200, mask=centre_mask(2).cuda(), x0=x0.cuda(), log_every_t=50,
                               normals_sequence=normals)
    errs = [mse(pool2(a), b) for a, b in zip(inter, g["mask/inter_pool2"])]
    assert len(inter) == g["mask/inter_pool2"].shape[0]
    assert mse(z, g["mask/z"]) < 1e-3 and max(errs) < 1e-3, errs


def test_bbox_chain_vs_reference():
    """Golden item 4: the bbox UNet, B = 1, p_sample_loop(timesteps=100).  Measured on the MI355X: MSE 1.0e-7."""
    g = golden()
    m = get_model("bbox")
    inp, cond = inputs(1, 44, 100)
    z, inter = m.p_sample_loop(cond, (1, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(), verbose=False,
                               timesteps=100, normals_sequence=inp["noise"])
    assert len(inter) == g["bbox/inter_pool2"].shape[0]
    assert max(mse(pool2(a), b) for a, b in zip(inter, g["bbox/inter_pool2"])) < 1e-3
    print("bbox MSE final %.3e" % mse(z, g["bbox/z"]))
    assert mse(z, g["bbox/z"]) < 1e-3, mse(z, g["bbox/z"])


class _RandnFeed:
    """torch.randn((1, C, H, W), device=...) -> the recipe x_T, as tests/golden/make_goldens.py::RandnFeed fed the
    reference (log_images draws its seeded x_T from the device generator)."""

    def __init__(self, x_T):
        self.x_T, self.hits = x_T, 0

    def __enter__(self):
        self.orig = torch.randn
        feed = self

        def randn(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
            if shape == tuple(feed.x_T.shape) and kw.get("generator") is None:
                feed.hits += 1
                return feed.x_T.clone().to(kw.get("device") or "cpu")
            return feed.orig(*size, **kw)

        torch.randn = randn
        return self

    def __exit__(self, *exc):
        torch.randn = self.orig


def test_log_images_vs_reference(monkeypatch):
    """Golden item 5: log_images(ddim_steps=None) — the DDPM chain under the EMA scope — and the plotting branches of
    a 5-step DDIM log_images: the reference's key sets, grid input shapes and the denoise-row stack.  The values of the
    inpainting / outpainting samples and of the diffusion row are not compared: they depend on the posterior sample z
    of get_input and on x_T / noise drawn inside those runs, which the fixture does not pin; they are checked for
    shape (through the grid inputs) and finiteness only."""
    g = golden()
    m = get_model("tiny", ema_salt=1)
    B = 2
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
             "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
             "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}
    x_T = synth.synth_inputs(1, HW, C, NTOK, 768, seed=11)["x_T"]
    noise = synth.synth_inputs(B, HW, C, NTOK, 768, seed=45, steps=50)["noise"]
    with _RandnFeed(x_T) as feed:
        log = m.log_images(batch, N=B, ddim_steps=None, seed=11, timesteps=50, normals_sequence=noise)
    assert feed.hits == 1
    assert sorted(log) == list(g["log_ddpm/keys"])
    pooled = torch.nn.functional.avg_pool2d(log["samples"].cpu(), 8)
    assert mse(pooled, g["log_ddpm/samples_pool8"]) < 1e-3
    _, c = m.get_input(batch, "image", force_c_encode=True, bs=B)[:2]
    with m.ema_scope():
        zs, inter = m.sample_log(cond=c, batch_size=B, ddim=False, ddim_steps=None, x_T=x_T.repeat(B, 1, 1, 1).cuda(),
                                 timesteps=50, normals_sequence=noise)
    assert mse(zs, g["log_ddpm/samples_z"]) < 1e-3 and len(inter) == int(g["log_ddpm/n_inter"])

    grids = []
    real = ddpm_mod.make_grid

    def recording(t, nrow=8, **k):
        grids.append((tuple(t.shape), int(nrow), t.detach().cpu().clone()))
        return real(t, nrow=nrow, **k)

    monkeypatch.setattr(ddpm_mod, "make_grid", recording)
    with _RandnFeed(x_T):
        log = m.log_images(batch, N=B, ddim_steps=5, seed=11, inpaint=True, plot_diffusion_rows=True,
                           plot_denoise_rows=True, normals_sequence=torch.zeros(5, B, C, *HW))
    assert sorted(log) == list(g["log_ddim/keys"])
    assert torch.equal(log["mask"].cpu(), torch.as_tensor(g["log_ddim/mask"]))
    assert [s for s, _, _ in grids] == [tuple(s) for s in g["log_ddim/grid_shapes"]]
    assert [n for _, n, _ in grids] == list(g["log_ddim/grid_nrow"])
    den = torch.nn.functional.avg_pool2d(grids[1][2], 8)
    assert mse(den, g["log_ddim/denoise_stack_pool8"]) < 1e-3
    for k in ("samples_inpainting", "samples_outpainting", "diffusion_row", "denoise_row"):
        assert torch.isfinite(log[k]).all(), k


def test_log_images_progressive_rows_ddpm_denoise_rows_and_quantize_noop():
    """The two branches that crash in the reference (a list indexed with 'x_inter') work here, and quantize_denoised
    is a no-op for the AutoencoderKL first stage."""
    m = get_model("tiny")
    B = 2
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
             "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
             "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}
    log = m.log_images(batch, N=B, ddim_steps=None, timesteps=20, plot_denoise_rows=True, plot_progressive_rows=True)
    assert {"samples", "denoise_row", "progressive_row"} <= set(log)
    # p_sample_loop logs x_T and then t = 19 and t = 0 (log_every_t = 1000): three images per row
    assert log["denoise_row"].shape == (3, 2 * (256 + 2) + 2, 3 * (192 + 2) + 2)
    # progressive_denoising runs the full 1000 steps and logs x0 at t = 999 and t = 0
    assert log["progressive_row"].shape == (3, 2 * (256 + 2) + 2, 2 * (192 + 2) + 2)
    x_T = torch.randn(1, C, *HW)
    outs = []
    for q in (False, True):
        with _RandnFeed(x_T):
            outs.append(m.log_images(batch, N=B, ddim_steps=4, ddim_eta=0.0, seed=5, quantize_denoised=q))
    assert sorted(outs[0]) == sorted(outs[1])
    assert torch.equal(outs[0]["samples"], outs[1]["samples"])


class _Identity:
    def modify_score(self, model, e_t, x, t, c, **kw):
        return e_t


def _torch_chain(m, cond, x, T, normals, mask=None, x0=None):
    """The reference's loop (ddpm.py:1157-1187, 1273-1283) in plain torch on the device: p_mean_variance (UNet forward,
    fp32 torch posterior), the posterior noise and the q_sample blend — no DDPM kernel involved."""
    per = 1 if mask is None else 2
    for k, i in enumerate(range(T - 1, -1, -1)):
        ts = torch.full((x.shape[0],), i, device="cuda", dtype=torch.long)
        mean, _, logvar = m.p_mean_variance(x, cond, ts, clip_denoised=False)
        n = normals[per * k].cuda()
        x = mean + (1 - (ts == 0).float()).reshape(-1, 1, 1, 1) * (0.5 * logvar).exp() * n
        if mask is not None:
            x = m.q_sample(x0, ts, noise=normals[2 * k + 1].cuda()) * mask + (1. - mask) * x
    return x


def test_fused_chain_equals_torch_and_general_paths():
    """On the same injected noise, with and without a mask: the captured-graph chain equals the reference's loop written
    in torch (checks the step kernel's arithmetic inside the chain), and equals the step-by-step p_sample path (forced
    by a score corrector that changes nothing; checks the chaining, graph grouping and logging)."""
    m = get_model("tiny")
    inp, cond, x0, normals = _mask_case()
    shape = (2, C) + HW
    x_T = inp["x_T"].cuda()
    mask, x0 = centre_mask(2).cuda(), x0.cuda()
    for kw, T, ns in ((dict(), 50, inp["noise"][:50]), (dict(mask=mask, x0=x0), 30, normals[:60])):
        fast = m.p_sample_loop(cond, shape, x_T=x_T, verbose=False, timesteps=T, normals_sequence=ns, **kw)
        assert mse(fast, _torch_chain(m, cond, x_T, T, ns, **kw)) < 1e-6, kw.keys()
        zf, xf = m.progressive_denoising(cond, shape[1:], verbose=False, batch_size=2, x_T=x_T, start_T=T,
                                         log_every_t=10, normals_sequence=ns, **kw)
        zg, xg = m.progressive_denoising(cond, shape[1:], verbose=False, batch_size=2, x_T=x_T, start_T=T,
                                         log_every_t=10, normals_sequence=ns, score_corrector=_Identity(), **kw)
        assert mse(zf, fast) == 0.0  # (the same fused chain behind both loops)
        assert mse(zf, zg) < 1e-6 and len(xf) == len(xg) and max(mse(a, b) for a, b in zip(xf, xg)) < 1e-6
    # p_sample: one t for the batch (upk_ddpm_step_f32) vs per-sample t (torch), row by row
    n = inp["noise"][0].cuda()
    for t in (0, 1, 500, 999):
        ts = torch.full((2,), t, device="cuda", dtype=torch.long)
        a, a0 = m.p_sample(x_T, cond, ts, return_x0=True, noise=n)
        mean, _, logvar, b0 = m.p_mean_variance(x_T, cond, ts, clip_denoised=False, return_x0=True)
        b = mean + (1 - (ts == 0).float()).reshape(2, 1, 1, 1) * (0.5 * logvar).exp() * n
        assert mse(a, b) < 1e-10 and mse(a0, b0) < 1e-10, t
    ts = torch.tensor([500, 0], device="cuda")
    a = m.p_sample(x_T, cond, ts, noise=n)
    b0 = m.p_sample(x_T[:1], {"c_crossattn": cond["c_crossattn"][:1], "c_concat": [cond["c_concat"][0][:1]]},
                    ts[:1], noise=n[:1])
    assert mse(a[:1], b0) < 1e-6


def test_steps_per_graph_does_not_change_results(monkeypatch):
    m = get_model("tiny")
    inp, cond, x0, normals = _mask_case()
    outs = []
    for spg in (1, 8):
        monkeypatch.setattr(ddim_mod, "STEPS_PER_GRAPH", spg)
        outs.append(m.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(),
                                    verbose=False, timesteps=37, mask=centre_mask(2).cuda(), x0=x0.cuda(),
                                    log_every_t=10, normals_sequence=normals[:74]))
    (z1, i1), (z8, i8) = outs
    assert torch.equal(z1, z8) and len(i1) == len(i8) == 6
    assert all(torch.equal(a, b) for a, b in zip(i1, i8))


def test_chain_advances_the_generator_like_the_reference():
    """x_T, then per step the posterior noise_like (also at t = 0), then with a mask q_sample's randn_like."""
    m = get_model("tiny")
    _, cond = inputs(2, 0, 0)
    shape = (2, C) + HW
    for masked, ndraw in ((False, 1 + 4), (True, 1 + 2 * 4)):
        kw = dict(mask=centre_mask(2).cuda(), x0=torch.zeros(shape, device="cuda")) if masked else {}
        torch.manual_seed(77)
        m.p_sample_loop(cond, shape, verbose=False, timesteps=4, **kw)
        after = torch.randn(8, device="cuda")
        torch.manual_seed(77)
        for _ in range(ndraw):
            torch.randn(shape, device="cuda")
        assert torch.equal(after, torch.randn(8, device="cuda")), masked


def test_chain_in_a_lane_is_bit_identical():
    m = get_model("tiny")
    inp, cond = inputs(2, 40, 40)
    run = lambda: m.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(),
                                  verbose=False, timesteps=40, log_every_t=10, normals_sequence=inp["noise"])
    z0, i0 = run()
    with upgpt_amd.lane(1):
        z1, i1 = run()
        torch.cuda.synchronize()
    assert torch.equal(z0, z1) and all(torch.equal(a, b) for a, b in zip(i0, i1))


def test_callbacks_order_and_counts():
    """callback(i) gets the timestep, img_callback(x, i) gets x (not x0); p_sample_loop logs, then calls back."""
    m = get_model("tiny")
    inp, cond = inputs(2, 40, 12)
    calls = []
    z, inter = m.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].cuda(), verbose=False,
                               timesteps=12, log_every_t=5, normals_sequence=inp["noise"],
                               callback=lambda i: calls.append(("cb", i)),
                               img_callback=lambda x, i: calls.append(("img", i, x.clone())))
    assert [c[:2] for c in calls] == [(k, i) for i in range(11, -1, -1) for k in ("cb", "img")]
    assert torch.equal(calls[-1][2], z)
    assert len(inter) == 1 + 4  # x_T, then t = 11, 10, 5, 0
    z2 = m.p_sample_loop(cond, (2, C) + HW, x_T=inp["x_T"].cuda(), verbose=False, timesteps=12,
                         normals_sequence=inp["noise"])
    assert torch.equal(z, z2)


def test_bbox_full_chain_batch8():
    """bbox UNet, B = 8, 32x24, the full 1000-step chain: finite, deterministic across two calls, and 1000 steps in
    ceil-grouped graph launches (STEPS_PER_GRAPH per launch, logged steps end a graph)."""
    m = get_model("bbox")
    inp, cond = inputs(8, 50, 0)
    x_T = inp["x_T"].cuda()
    launches = []
    from upgpt_amd import engine
    orig = engine.SamplerState.launch

    def counting(self, with_noise, scale=1.0, nsteps=1):
        launches.append(nsteps)
        return orig(self, with_noise, scale, nsteps)

    engine.SamplerState.launch = counting
    try:
        with m.ema_scope():
            torch.manual_seed(3)
            a = m.sample(cond, batch_size=8, x_T=x_T, verbose=False)
            torch.manual_seed(3)
            b = m.sample(cond, batch_size=8, x_T=x_T, verbose=False)
    finally:
        engine.SamplerState.launch = orig
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # log_every_t = 1000: only k = 0 (t = 999) and t = 0 are logged -> a single step, then groups of STEPS_PER_GRAPH
    spg = ddim_mod.STEPS_PER_GRAPH
    per_call = 1 + -(-999 // spg)
    assert sum(launches) == 2000 and len(launches) == 2 * per_call, (len(launches), per_call)


def test_plan_close_releases_the_ddpm_state(monkeypatch):
    """UNetPlan.close() (plan eviction, UNetModel.invalidate()) destroys the DDPM state's captured graphs and drops
    the state with its noise tables."""
    from upgpt_amd import _lib
    m = get_model("tiny")
    inp, cond = inputs(2, 40, 20)
    unet = m.model.diffusion_model
    m.p_sample_loop(cond, (2, C) + HW, x_T=inp["x_T"].cuda(), verbose=False, timesteps=20,
                    normals_sequence=inp["noise"])
    plans = [pl for pl in unet._plans.values() if ("ddpm", False) in pl.sampler_states]
    assert plans
    graphs = [g for pl in plans for g in pl.sampler_state("ddpm", C).graphs.values()]
    assert graphs
    destroyed = []
    orig = _lib.Context.graph_destroy
    monkeypatch.setattr(_lib.Context, "graph_destroy", lambda self, g: (destroyed.append(g), orig(self, g))[1])
    unet.invalidate()
    assert all(not pl.sampler_states for pl in plans)
    assert all(any(g is d for d in destroyed) for g in graphs)
