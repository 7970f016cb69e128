"""DPMSolverSampler (upgpt_amd/dpm_solver.py) on a real MI355X: the captured-graph fast path against the step-by-step
general path, against the fp64 chain of tests/dpm_ref.py (driven by the model's own apply_model, and by the fp32 CPU UNet of
oracle/unet.py), and the surfaces that reach it.  Tiny model, 16x8 latent, B = 2; S = 6 (the last row is first-order) and
S = 16 (it is second-order).  Tolerances: 1e-4 latent MSE between two runs of the same kernels (the figure of the PLMS
fast / general test), 1e-3 against the fp32 CPU model (the project's latent tolerance)."""
import numpy as np
import pytest
import torch

import dpm_ref as R
import upgpt_amd
from oracle import unet as o_unet
from upgpt_amd import rng, synth
from upgpt_amd.ddim import DDIMSampler
from upgpt_amd.dpm_solver import DPMSolverSampler

pytestmark = pytest.mark.gpu
HW = (16, 8)
B = 2
SHAPE = (4,) + HW
ACP = R.linear_alphas_cumprod()  # the configs' schedule, fp32 widened: what the model holds
_cache = {}


def get_model(kind="tiny"):
    if kind not in _cache:
        if kind == "tiny":
            m = upgpt_amd.build_model("tiny")
        else:  # the upscale model's channel layout (3 latent + 3 concat channels, no pose stage) on the tiny topology
            unet = dict(synth.TINY_UNET, in_channels=6, out_channels=3)
            m = upgpt_amd.build_model("tiny", overrides={"channels": 3, "concat_key": "lr", "unet_config": {
                "target": "upgpt_amd.unet.UNetModel", "params": unet}})
        sd = synth.fill_module_(m)
        _cache[kind] = (m.cuda(), sd)
    return _cache[kind]


def mse(a, b):
    return float(((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()) ** 2).mean())


def _case(seed=5, hw=HW, C=4, cc=1, b=B):
    inp = synth.synth_inputs(b, hw, C, 87, 768, seed=seed, concat_channels=cc)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    return inp, cond, uc, inp["x_T"].cuda()


def _general(monkeypatch):
    monkeypatch.setattr(DDIMSampler, "_fast_ok", lambda self, *a, **k: False)


def _count_apply_model(model, monkeypatch):
    calls = []
    orig = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    return calls


def _ref_tables(S):
    ts = R.logsnr_nodes(ACP, S)[1:]
    return ts[::-1], R.coefficient_table(*R.tables(ACP, ts)).astype(np.float32)  # the fp32 rows the kernel reads


def _device_eps(model, cond, uc=None, scale=1.0):
    def fn(x, t, i):
        xx = torch.from_numpy(x).float().cuda()
        tt = torch.full((xx.shape[0],), t, device="cuda", dtype=torch.long)
        if uc is None:
            return model.apply_model(xx, tt, cond).double().cpu().numpy()
        # one pass over [uncond ; cond], the batch the sampler evaluates (another batch size takes other tiles, and at
        # scale 3 the fp16 roundings of two separate passes do not cancel: 6e-4 on latents of magnitude 30)
        e_u, e = model.apply_model(torch.cat([xx] * 2), torch.cat([tt] * 2), DDIMSampler._cat_cond(uc, cond)).double().chunk(2)
        return (e_u + scale * (e - e_u)).cpu().numpy()
    return fn


@pytest.fixture(scope="module")
def runs():
    """The fast-path results every comparison shares: {S: (z, intermediates)} on one x_T and conditioning."""
    model, _ = get_model()
    _, cond, _, x_T = _case()
    out = {}
    for S in (6, 16):
        out[S] = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2)
    return out


@pytest.mark.parametrize("S", [6, 16])
def test_fast_path_is_deterministic_and_runs_no_python_step(runs, S, monkeypatch):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    calls = _count_apply_model(model, monkeypatch)
    z, inter = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2)
    assert not calls
    assert z.shape == (B,) + SHAPE and torch.isfinite(z).all()
    assert torch.equal(z, runs[S][0])
    for k in ("x_inter", "pred_x0"):
        assert len(inter[k]) == len(runs[S][1][k]) and all(torch.equal(u, v) for u, v in zip(inter[k], runs[S][1][k]))


@pytest.mark.parametrize("S", [6, 16])
def test_fast_against_general_path(runs, S, monkeypatch):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    calls = _count_apply_model(model, monkeypatch)
    _general(monkeypatch)
    zg, ig = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2)
    assert len(calls) == S
    zf, iff = runs[S]
    e = mse(zf, zg)
    print("S = %d: latent mse fast vs general %.3e" % (S, e))
    assert e < 1e-4
    for k in ("x_inter", "pred_x0"):  # the logged steps line up
        assert len(iff[k]) == len(ig[k]) == 1 + len([i for i in range(S) if i % 2 == 0 or i == S - 1])
        for u, v in zip(iff[k], ig[k]):
            assert mse(u, v) < 1e-4


@pytest.mark.parametrize("S", [6, 16])
def test_fast_path_against_the_fp64_chain_on_the_device_model(runs, S):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    ts, tab = _ref_tables(S)
    z_ref = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab)[0]
    e = mse(runs[S][0], z_ref)
    print("S = %d: latent mse fast path vs fp64 chain (device model) %.3e" % (S, e))
    assert e < 1e-4


@pytest.mark.parametrize("S", [6, 16])
def test_fast_path_against_the_fp64_chain_on_the_cpu_oracle_unet(runs, S):
    model, sd = get_model()
    inp, _, _, x_T = _case()

    def eps(x, t, i):
        xx = torch.from_numpy(x).float()
        tt = torch.full((xx.shape[0],), t, dtype=torch.long)
        return o_unet.diffusion_wrapper(sd, synth.TINY_UNET, xx, tt, [inp["c_concat"]], inp["c_crossattn"]).double().numpy()

    ts, tab = _ref_tables(S)
    z_ref = R.chain(eps, inp["x_T"].numpy(), ts, tab)[0]
    e = mse(runs[S][0], z_ref)
    print("S = %d: latent mse fast path vs fp64 chain (fp32 CPU UNet) %.3e" % (S, e))
    assert e < 1e-3


def test_guidance_fast_general_and_reference(runs, monkeypatch):
    model, _ = get_model()
    _, cond, uc, x_T = _case()
    S = 6
    kw = dict(x_T=x_T, verbose=False, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    calls = _count_apply_model(model, monkeypatch)
    zf, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, **kw)
    assert not calls
    ts, tab = _ref_tables(S)
    z_ref = R.chain(_device_eps(model, cond, uc, 3.0), x_T.cpu().numpy(), ts, tab)[0]
    del calls[:]
    _general(monkeypatch)
    zg, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, **kw)
    assert len(calls) == S  # (one pass over [uncond ; cond] per step)
    print("guided: fast vs general %.3e, fast vs fp64 chain %.3e, guided vs plain %.3e" % (
        mse(zf, zg), mse(zf, z_ref), mse(zf, runs[S][0])))
    assert mse(zf, zg) < 1e-4 and mse(zf, z_ref) < 1e-4
    assert mse(zf, runs[S][0]) > 1e-3


def test_order_one_on_the_uniform_grid_is_ddim():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    S = 10
    zd, _ = DDIMSampler(model).sample(S, B, SHAPE, cond, eta=0.0, x_T=x_T, verbose=False)
    z1, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, order=1, discretize="uniform")
    z2, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, order=2, discretize="uniform")
    print("order 1 / uniform vs DDIM: %.3e; order 2 vs DDIM: %.3e" % (mse(z1, zd), mse(z2, zd)))
    assert mse(z1, zd) < 1e-6
    assert mse(z2, zd) > 1e-6  # (the order argument does something)


def test_upscale_channel_layout_fast_against_general(monkeypatch):
    """C = 3 latent + 3 concat channels, 32x24, B = 1: the step kernel's element-wise xin rows inside the captured loop."""
    model, _ = get_model("upscale3")
    _, cond, _, x_T = _case(seed=7, hw=(32, 24), C=3, cc=3, b=1)
    S = 6
    calls = _count_apply_model(model, monkeypatch)
    zf, _ = DPMSolverSampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False)
    assert not calls and zf.shape == (1, 3, 32, 24) and torch.isfinite(zf).all()
    _general(monkeypatch)
    zg, _ = DPMSolverSampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False)
    assert len(calls) == S
    print("C = 3: latent mse fast vs general %.3e" % mse(zf, zg))
    assert mse(zf, zg) < 1e-4


def test_masked_chain_and_decode_take_the_general_path(monkeypatch):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    S = 6
    ts, tab = _ref_tables(S)
    x0 = (0.7 * synth.synth_inputs(B, HW, 4, 87, 768, seed=6)["x_T"]).cuda()
    mask = torch.zeros(B, 1, *HW, device="cuda")
    mask[:, :, :, :HW[1] // 2] = 1.0  # the left half is kept
    keys = rng.NoiseKeys(11, [3, 4], device="cuda")
    calls = _count_apply_model(model, monkeypatch)
    z, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, mask=mask, x0=x0, noise_keys=keys)
    assert len(calls) == S  # (the captured loop has no mask blend: refused)

    x0_64, m64 = x0.double().cpu().numpy(), mask.double().cpu().numpy()

    def blend(x, t, i):
        nz = rng.randn(keys, (B,) + SHAPE, rng.STREAM_QSAMPLE, row0=i).double().cpu().numpy()
        return (np.sqrt(ACP[t]) * x0_64 + np.sqrt(1 - ACP[t]) * nz) * m64 + (1 - m64) * x

    z_ref = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab, blend=blend)[0]
    print("masked chain vs fp64 chain %.3e" % mse(z, z_ref))
    assert mse(z, z_ref) < 1e-4
    assert mse(z, DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False)[0]) > 1e-3

    # decode: the last 4 rows of the 6-row schedule; the chain's first row is first-order
    del calls[:]
    sampler = DPMSolverSampler(model)
    sampler.make_schedule(S, verbose=False)
    x_dec = sampler.decode(x_T, cond, 4)
    assert len(calls) == 4
    d_ref = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab, start=S - 4)[0]
    print("decode(t_start = 4) vs fp64 chain %.3e" % mse(x_dec, d_ref))
    assert mse(x_dec, d_ref) < 1e-4


def test_noise_keys_give_x_T():
    model, _ = get_model()
    _, cond, _, _ = _case()
    S = 6
    run = lambda keys, c=cond: DPMSolverSampler(model).sample(S, len(keys), SHAPE, c, verbose=False, noise_keys=keys)[0]
    g0 = torch.cuda.get_rng_state()
    a = run(rng.NoiseKeys(7, [10, 11], device="cuda"))
    assert torch.equal(torch.cuda.get_rng_state(), g0)  # the generator is not touched
    assert torch.equal(a, run(rng.NoiseKeys(7, [10, 11], device="cuda")))
    flip = lambda d: {"c_crossattn": d["c_crossattn"].flip(0), "c_concat": [d["c_concat"][0].flip(0)]}
    b = run(rng.NoiseKeys(7, [11, 10], device="cuda"), flip(cond))  # the same samples at the other batch position
    print("same key, other batch position: %.3e" % mse(a, b.flip(0)))
    assert mse(a, b.flip(0)) < 1e-4  # (the same picture; tiles may differ with the position, bits need not agree)
    assert mse(a, run(rng.NoiseKeys(8, [10, 11], device="cuda"))) > 1e-3


def test_callbacks_and_logged_steps_match_the_general_path(monkeypatch):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    S = 6

    def run():
        seen, imgs = [], []
        z, inter = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=3,
                                                  callback=seen.append, img_callback=lambda p, i: imgs.append((i, p.clone())))
        return z, inter, seen, imgs

    zf, iff, sf, mf = run()
    _general(monkeypatch)
    zg, ig, sg, mg = run()
    assert sf == sg == list(range(S)) and [i for i, _ in mf] == [i for i, _ in mg] == list(range(S))
    assert mse(zf, zg) < 1e-4
    for (_, u), (_, v) in zip(mf, mg):
        assert mse(u, v) < 1e-4
    for k in ("x_inter", "pred_x0"):
        assert len(iff[k]) == len(ig[k]) == 4  # x_T, then indices 5 (first), 3, 0
        for u, v in zip(iff[k], ig[k]):
            assert mse(u, v) < 1e-4
    assert torch.equal(iff["x_inter"][-1], zf)


def test_refusals():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    with pytest.raises(ValueError):
        DPMSolverSampler(model).sample(6, B, SHAPE, cond, x_T=x_T, verbose=False, eta=0.5)
    with pytest.raises(ValueError):
        DPMSolverSampler(model).make_schedule(6, ddim_eta=0.5, verbose=False)
    with pytest.raises(ValueError):
        model.sample_log(cond, B, True, 6, sampler="euler")


def test_log_images_takes_the_sampler(monkeypatch):
    model, _ = get_model()
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
             "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
             "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}
    seen = []
    orig = DPMSolverSampler.sample
    monkeypatch.setattr(DPMSolverSampler, "sample", lambda self, *a, **k: (seen.append((a[0], k.get("eta", 0.))), orig(self, *a, **k))[1])
    torch.manual_seed(1)
    log = model.log_images(batch, N=B, sampler="dpmpp_2m", ddim_steps=6)  # (ddim_eta's default of 1 is DDIM's: dropped)
    assert seen == [(6, 0.)]
    assert log["samples"].shape == (B, 3, 256, 192) and torch.isfinite(log["samples"]).all()
    torch.manual_seed(1)
    ddim = model.log_images(batch, N=B, ddim_steps=6, ddim_eta=0.0)
    assert len(seen) == 1 and mse(log["samples"], ddim["samples"]) > 1e-6  # the default is still DDIM
