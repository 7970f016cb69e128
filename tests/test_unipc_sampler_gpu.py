"""UniPCSampler (upgpt_amd/unipc.py) on a real MI355X: the captured-graph fast path against the step-by-step general path
and against the fp64 chain of tests/unipc_ref.py driven by the model's own apply_model, the predictor alone against
DPMSolverSampler, and the surfaces that reach the sampler.  Tiny model, 16x8 latent, B = 2, S = 6 (at order 3 the rows run
every corrector and predictor order).  Tolerances are test_dpm_sampler_gpu.py's: 1e-4 latent MSE between two runs of the
same kernels and against the fp64 chain on the device model."""
import numpy as np
import pytest
import torch

import unipc_ref as R
import upgpt_amd
from upgpt_amd import rng, synth
from upgpt_amd.ddim import DDIMSampler
from upgpt_amd.dpm_solver import DPMSolverSampler
from upgpt_amd.unipc import UniPCSampler

pytestmark = pytest.mark.gpu
HW = (16, 8)
B = 2
S = 6
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
        synth.fill_module_(m)
        _cache[kind] = m.cuda()
    return _cache[kind]


def mse(a, b):
    return float(((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()) ** 2).mean())


def _case(seed=5, hw=HW, C=4, cc=1, b=B):
    inp = synth.synth_inputs(b, hw, C, 87, 768, seed=seed, concat_channels=cc)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    return cond, uc, inp["x_T"].cuda()


def _general(monkeypatch):
    monkeypatch.setattr(DDIMSampler, "_fast_ok", lambda self, *a, **k: False)


def _count_apply_model(model, monkeypatch):
    calls = []
    orig = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    return calls


def _ref_tables(start=0, **kw):
    ts = R.logsnr_nodes(ACP, S)[1:]
    tab = R.coefficient_table(*R.tables(ACP, ts), start=start, **kw).astype(np.float32)  # the fp32 rows the kernel reads
    return ts[::-1][start:], tab


def _device_eps(model, cond, uc=None, scale=1.0):
    def fn(x, t, i):
        xx = torch.from_numpy(x).float().cuda()
        tt = torch.full((xx.shape[0],), t, device="cuda", dtype=torch.long)
        if uc is None:
            return model.apply_model(xx, tt, cond).double().cpu().numpy()
        # one pass over [uncond ; cond], the batch the sampler evaluates (test_dpm_sampler_gpu.py)
        e_u, e = model.apply_model(torch.cat([xx] * 2), torch.cat([tt] * 2), DDIMSampler._cat_cond(uc, cond)).double().chunk(2)
        return (e_u + scale * (e - e_u)).cpu().numpy()
    return fn


@pytest.fixture(scope="module")
def runs():
    """The fast-path results every comparison shares: {order: (z, intermediates)} on one x_T and conditioning."""
    model = get_model()
    cond, _, x_T = _case()
    return {o: UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2, order=o) for o in (2, 3)}


@pytest.mark.parametrize("order", [2, 3])
def test_fast_path_is_deterministic_and_runs_no_python_step(runs, order, monkeypatch):
    model = get_model()
    cond, _, x_T = _case()
    calls = _count_apply_model(model, monkeypatch)
    z, inter = UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2, order=order)
    assert not calls
    assert z.shape == (B,) + SHAPE and torch.isfinite(z).all()
    assert torch.equal(z, runs[order][0])
    for k in ("x_inter", "pred_x0"):
        assert len(inter[k]) == len(runs[order][1][k]) and all(torch.equal(u, v) for u, v in zip(inter[k], runs[order][1][k]))
    assert mse(runs[2][0], runs[3][0]) > 1e-8  # (the order argument does something)


@pytest.mark.parametrize("order", [2, 3])
def test_fast_against_general_path(runs, order, monkeypatch):
    model = get_model()
    cond, _, x_T = _case()
    calls = _count_apply_model(model, monkeypatch)
    _general(monkeypatch)
    zg, ig = UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=2, order=order)
    assert len(calls) == S
    zf, iff = runs[order]
    e = mse(zf, zg)
    print("order %d: latent mse fast vs general %.3e" % (order, e))
    assert e < 1e-4
    for k in ("x_inter", "pred_x0"):  # the logged steps line up
        assert len(iff[k]) == len(ig[k]) == 1 + len([i for i in range(S) if i % 2 == 0 or i == S - 1])
        for u, v in zip(iff[k], ig[k]):
            assert mse(u, v) < 1e-4


@pytest.mark.parametrize("kw", [dict(order=2), dict(order=3), dict(order=3, variant="bh1")], ids=["o2", "o3", "o3-bh1"])
def test_fast_path_against_the_fp64_chain_on_the_device_model(runs, kw):
    model = get_model()
    cond, _, x_T = _case()
    z = runs[kw["order"]][0] if len(kw) == 1 else UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, **kw)[0]
    ts, tab = _ref_tables(**kw)
    z_ref, _, ms = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab)
    e = mse(z, z_ref)
    print("%s: latent mse fast path vs fp64 chain (device model) %.3e" % (kw, e))
    assert e < 1e-4
    if len(kw) == 1:  # the last logged pred_x0 is m of the last evaluation
        assert mse(runs[kw["order"]][1]["pred_x0"][-1], ms[-1]) < 1e-4


def test_guidance_fast_general_and_reference(runs, monkeypatch):
    model = get_model()
    cond, uc, x_T = _case()
    kw = dict(x_T=x_T, verbose=False, unconditional_guidance_scale=3.0, unconditional_conditioning=uc, order=3)
    calls = _count_apply_model(model, monkeypatch)
    zf, _ = UniPCSampler(model).sample(S, B, SHAPE, cond, **kw)
    assert not calls
    ts, tab = _ref_tables(order=3)
    z_ref = R.chain(_device_eps(model, cond, uc, 3.0), x_T.cpu().numpy(), ts, tab)[0]
    del calls[:]
    _general(monkeypatch)
    zg, _ = UniPCSampler(model).sample(S, B, SHAPE, cond, **kw)
    assert len(calls) == S  # (one pass over [uncond ; cond] per step)
    print("guided: fast vs general %.3e, fast vs fp64 chain %.3e, guided vs plain %.3e" % (
        mse(zf, zg), mse(zf, z_ref), mse(zf, runs[3][0])))
    assert mse(zf, zg) < 1e-4 and mse(zf, z_ref) < 1e-4
    assert mse(zf, runs[3][0]) > 1e-3


def test_predictor_of_order_two_is_dpmpp_2m(runs):
    model = get_model()
    cond, _, x_T = _case()
    zp, _ = UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, order=2, corrector=False)
    zd, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, lower_order_final=True)
    print("UniP-2 vs DPM-Solver++(2M): %.3e; UniPC-2 vs UniP-2: %.3e" % (mse(zp, zd), mse(runs[2][0], zp)))
    assert mse(zp, zd) < 1e-4
    assert mse(runs[2][0], zp) > 100 * max(mse(zp, zd), 1e-12)  # (the corrector does something)


def test_upscale_channel_layout_fast_against_general(monkeypatch):
    """C = 3 latent + 3 concat channels, 32x24, B = 1: the step kernel's element-wise xin rows inside the captured loop."""
    model = get_model("upscale3")
    cond, _, x_T = _case(seed=7, hw=(32, 24), C=3, cc=3, b=1)
    calls = _count_apply_model(model, monkeypatch)
    zf, _ = UniPCSampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False, order=3)
    assert not calls and zf.shape == (1, 3, 32, 24) and torch.isfinite(zf).all()
    _general(monkeypatch)
    zg, _ = UniPCSampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False, order=3)
    assert len(calls) == S
    print("C = 3: latent mse fast vs general %.3e" % mse(zf, zg))
    assert mse(zf, zg) < 1e-4


def test_decode_runs_a_table_of_its_own(monkeypatch):
    """The last 4 rows of the 6-row schedule: no corrector and a first-order predictor on the chain's first row."""
    model = get_model()
    cond, _, x_T = _case()
    calls = _count_apply_model(model, monkeypatch)
    sampler = UniPCSampler(model)
    sampler.make_schedule(S, verbose=False, order=3)
    x_dec = sampler.decode(x_T, cond, 4)
    assert len(calls) == 4
    ts, tab = _ref_tables(start=S - 4, order=3)
    assert tab.shape == (4, 12)
    d_ref = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab)[0]
    print("decode(t_start = 4) vs fp64 chain %.3e" % mse(x_dec, d_ref))
    assert mse(x_dec, d_ref) < 1e-4 and torch.isfinite(x_dec).all()


def test_noise_keys_give_x_T():
    model = get_model()
    cond, _, _ = _case()
    run = lambda keys, c=cond: UniPCSampler(model).sample(S, len(keys), SHAPE, c, verbose=False, noise_keys=keys)[0]
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
    model = get_model()
    cond, _, x_T = _case()

    def run():
        seen, imgs = [], []
        z, inter = UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, log_every_t=3, order=3,
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
    assert torch.equal(iff["x_inter"][-1], zf)  # the logged latent is the predicted one
    assert torch.equal(iff["pred_x0"][-1], mf[-1][1])  # pred_x0 = m of the evaluation


def test_refusals():
    model = get_model()
    cond, _, x_T = _case()
    x0 = torch.zeros((B,) + SHAPE, device="cuda")
    mask = torch.ones(B, 1, *HW, device="cuda")
    with pytest.raises(NotImplementedError, match="dpmpp_2m"):
        UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, mask=mask, x0=x0)
    with pytest.raises(NotImplementedError, match="dpmpp_2m"):
        model.sample_log(cond, B, True, S, sampler="unipc", x_T=x_T, mask=mask, x0=x0)
    with pytest.raises(ValueError):
        UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, eta=0.5)
    with pytest.raises(ValueError):
        UniPCSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, order=4)
    with pytest.raises(ValueError):
        model.sample_log(cond, B, True, S, sampler="unipc", x_T=x_T, variant="bh3")


def test_log_images_takes_the_sampler(monkeypatch):
    model = get_model()
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
             "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
             "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}
    seen = []
    orig = UniPCSampler.sample
    monkeypatch.setattr(UniPCSampler, "sample", lambda self, *a, **k: (seen.append((a[0], k.get("eta", 0.), k.get("order"))), orig(self, *a, **k))[1])
    torch.manual_seed(1)
    log = model.log_images(batch, N=B, sampler="unipc", ddim_steps=S)  # (ddim_eta's default of 1 is DDIM's: dropped)
    assert seen == [(S, 0., None)]
    assert log["samples"].shape == (B, 3, 256, 192) and torch.isfinite(log["samples"]).all()
    torch.manual_seed(1)
    dpm = model.log_images(batch, N=B, sampler="dpmpp_2m", ddim_steps=S)
    assert len(seen) == 1 and mse(log["samples"], dpm["samples"]) > 1e-8  # another solver, another picture
