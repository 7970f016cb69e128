"""DPMSolverSDESampler (upgpt_amd/dpm_sde.py) on a real MI355X: the captured-graph fast path (the whole chain, guided, masked,
decode) against the step-by-step general path under the same seed and the same keys, against the fp64 chain of
tests/sde_ref.py fed the same keyed normals (tests/rng_ref.py), keep rows and the device model's eps, against
DPMSolverSampler at eta = 0, and the surfaces that reach it.  Tiny model, 16x8 latent, B = 2, S = 6 (the last row is
first-order).  Tolerance: 1e-4 latent MSE, the project's path-against-path figure."""
import numpy as np
import pytest
import torch

import rng_ref
import sde_ref as R
import upgpt_amd
from test_dpm_sampler_gpu import B, HW, SHAPE, _case, _count_apply_model, _device_eps, _general, get_model, mse
from upgpt_amd import _lib as L
from upgpt_amd import rng, synth
from upgpt_amd.dpm_sde import DPMSolverSDESampler
from upgpt_amd.dpm_solver import DPMSolverSampler

pytestmark = pytest.mark.gpu
S = 6
N = int(np.prod(SHAPE))
ACP = R.linear_alphas_cumprod()
SEED, IDS = 11, [3, 4]


def _keys(seed=SEED):
    return rng.NoiseKeys(seed, IDS, device="cuda")


def _edit():
    x0 = (0.7 * synth.synth_inputs(B, HW, 4, 87, 768, seed=6)["x_T"]).cuda()
    mask = torch.zeros(B, 1, *HW, device="cuda")
    mask[:, :, :, :HW[1] // 2] = 1.0  # the left half is kept
    return x0, mask


def _state(model, guided=False, shape=(B,) + SHAPE):
    """The model's "dpm_sde" sampler state for latents of `shape`."""
    return [s for p in model.model.diffusion_model._plans.values() for k, s in p.sampler_states.items()
            if k == ("dpm_sde", guided) and tuple(s.x.shape) == tuple(shape)][0]


def _ref(eta, start=0):
    ts = R.logsnr_nodes(ACP, S)[1:]
    return ts[::-1], R.coefficient_table(*R.tables(ACP, ts), eta=eta, start=start).astype(np.float32)


def _normals(stream, seed=SEED):
    return rng_ref.normals(rng_ref.keys_of(seed, IDS), N, 0, S, stream, 0).reshape((S, B) + SHAPE)


def _keep_rows(x0, ts):
    """keep[i] = q_sample(x0, t_i) with the keyed normals of STREAM_QSAMPLE, row i, fp64."""
    nz, x64 = _normals(rng.STREAM_QSAMPLE), x0.double().cpu().numpy()
    return np.stack([np.sqrt(ACP[t]) * x64 + np.sqrt(1 - ACP[t]) * nz[i] for i, t in enumerate(ts)])


def _cases():
    """name -> (run(sampler, **noise) -> (z, intermediates), model evaluations of the general path)."""
    model, _ = get_model()
    _, cond, uc, x_T = _case()
    x0, mask = _edit()
    kw = dict(x_T=x_T, verbose=False, log_every_t=2)
    guided = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)

    def decode(s, **noise):
        s.make_schedule(S, verbose=False)
        return s.decode(x_T, cond, 4, **noise), {"x_inter": [], "pred_x0": []}

    return {"plain": (lambda s, **n: s.sample(S, B, SHAPE, cond, **kw, **n), S),
            "guided": (lambda s, **n: s.sample(S, B, SHAPE, cond, **kw, **guided, **n), S),
            "masked": (lambda s, **n: s.sample(S, B, SHAPE, cond, mask=mask, x0=x0, **kw, **n), S),
            "decode": (decode, 4)}


@pytest.mark.parametrize("keyed", [False, True], ids=["seeded", "keyed"])
@pytest.mark.parametrize("name", ["plain", "guided", "masked", "decode"])
def test_fast_against_general_path(name, keyed, monkeypatch):
    model, _ = get_model()
    run, evals = _cases()[name]
    noise = (lambda: {"noise_keys": _keys()}) if keyed else (lambda: {})
    calls = _count_apply_model(model, monkeypatch)
    torch.manual_seed(9)
    g0 = torch.cuda.get_rng_state()
    zf, fi = run(DPMSolverSDESampler(model), **noise())
    gf = torch.cuda.get_rng_state()
    assert not calls  # the captured chain runs no model evaluation from Python
    assert keyed == torch.equal(g0, gf)  # keyed: the generator is not touched; seeded: one draw per step
    _general(monkeypatch)
    torch.manual_seed(9)
    zg, gi = run(DPMSolverSDESampler(model), **noise())
    assert len(calls) == evals
    assert torch.equal(torch.cuda.get_rng_state(), gf)  # both paths leave the device generator at the same state
    e = mse(zf, zg)
    print("%s %s: latent mse fast vs general %.3e" % (name, "keyed" if keyed else "seeded", e))
    assert torch.isfinite(zf).all() and e < 1e-4
    for k in ("x_inter", "pred_x0"):
        assert len(fi[k]) == len(gi[k]) == (0 if name == "decode" else 1 + len([i for i in range(S) if i % 2 == 0 or i == S - 1]))
        for u, v in zip(fi[k], gi[k]):
            assert mse(u, v) < 1e-4


@pytest.mark.parametrize("name", ["plain", "masked", "guided"])
def test_keyed_fast_path_against_the_fp64_chain(name):
    model, _ = get_model()
    _, cond, uc, x_T = _case()
    x0, mask = _edit()
    z, _ = _cases()[name][0](DPMSolverSDESampler(model), noise_keys=_keys())
    ts, tab = _ref(1.0)
    eps = _device_eps(model, cond, uc, 3.0) if name == "guided" else _device_eps(model, cond)
    edit = dict(keep=_keep_rows(x0, ts), mask=mask.double().cpu().numpy()) if name == "masked" else {}
    z_ref = R.chain(eps, x_T.cpu().numpy(), ts, tab, 0, _normals(rng.STREAM_STEP), **edit)[0]
    e = mse(z, z_ref)
    print("%s: latent mse keyed fast path vs fp64 chain %.3e" % (name, e))
    assert e < 1e-4


def test_keyed_decode_against_the_fp64_chain():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    z = _cases()["decode"][0](DPMSolverSDESampler(model), noise_keys=_keys())[0]
    ts, tab = _ref(1.0, start=2)
    assert tab[0, 4] == 0  # the chain's first row is first-order
    z_ref = R.chain(_device_eps(model, cond), x_T.cpu().numpy(), ts, tab, 2, _normals(rng.STREAM_STEP))[0]
    print("decode(t_start = 4): latent mse vs fp64 chain %.3e" % mse(z, z_ref))
    assert mse(z, z_ref) < 1e-4


def test_eta_zero_is_dpm_solver_and_draws_nothing(monkeypatch):
    model, _ = get_model()
    _, cond, _, x_T = _case()
    zd, _ = DPMSolverSampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False)
    torch.manual_seed(4)
    g0 = torch.cuda.get_rng_state()
    noisy = []
    launch = upgpt_amd.engine.SamplerState.launch
    monkeypatch.setattr(upgpt_amd.engine.SamplerState, "launch", lambda self, with_noise, *a: (
        noisy.append(with_noise), launch(self, with_noise, *a))[1])
    z0, _ = DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, eta=0.0)
    assert torch.equal(torch.cuda.get_rng_state(), g0)  # no generator state is consumed after x_T
    assert noisy and not any(noisy)  # ... and no launch reads a noise table
    print("eta = 0 vs DPMSolverSampler: latent mse %.3e" % mse(z0, zd))
    assert mse(z0, zd) < 1e-4
    z1, _ = DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, eta=1.0)
    assert mse(z1, zd) > 1e-3  # (eta does something)


def test_keys_repeat_bit_for_bit_and_seeds_differ():
    model, _ = get_model()
    _, cond, _, _ = _case()
    run = lambda keys, **kw: DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, verbose=False, noise_keys=keys, **kw)[0]
    a = run(_keys())
    assert torch.equal(a, run(_keys()))
    assert mse(a, run(_keys(SEED + 1))) > 1e-3
    assert mse(a, run(_keys(), temperature=0.5)) > 1e-5  # (the noise scale reaches the table)


def test_masked_chain_all_kept_and_none_kept():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    x0, _ = _edit()
    s = DPMSolverSDESampler(model)
    kw = dict(x_T=x_T, verbose=False, log_every_t=1, noise_keys=_keys())
    ones, zeros = torch.ones(B, 1, *HW, device="cuda"), torch.zeros(B, 1, *HW, device="cuda")
    z, inter = s.sample(S, B, SHAPE, cond, mask=ones, x0=x0, **kw)
    st = _state(model)
    keep = st.keep.view((S, B) + SHAPE)
    assert len(inter["x_inter"]) == S + 1
    for i in range(S):  # the logged latent is the unblended step: the model ran, its result is not the keep row
        assert mse(inter["x_inter"][i + 1], keep[i]) > 1e-6
        if i + 1 < S:
            assert mse(inter["x_inter"][i + 1], keep[i + 1]) > 1e-6
    assert torch.equal(z, inter["x_inter"][-1]) and torch.equal(z, st.x_plain)  # the final latent is the unblended last step
    zz, _ = s.sample(S, B, SHAPE, cond, mask=zeros, x0=x0, **kw)
    zp, _ = s.sample(S, B, SHAPE, cond, **kw)
    assert torch.equal(zz, zp)  # nothing kept: the unmasked keyed chain, bit for bit


def test_callbacks_end_a_graph_group_and_see_every_position():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    launches, seen, imgs = [], [], []
    lib = L.get_context(0).lib
    orig = lib.upk_graph_launch
    z0, _ = DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, noise_keys=_keys())
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "upk_graph_launch", lambda *a: (launches.append(1), orig(*a))[1], raising=False)
        z, _ = DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, x_T=x_T, verbose=False, noise_keys=_keys(),
                                                 callback=seen.append, img_callback=lambda p, i: imgs.append(i))
    assert seen == imgs == list(range(S)) and len(launches) == S  # one graph per watched step
    assert mse(z, z0) < 1e-4


def test_a_repeat_captures_no_graph_and_uploads_no_table(monkeypatch):
    model, _ = get_model()
    _, cond, uc, x_T = _case()
    x0, mask = _edit()
    sampler = DPMSolverSDESampler(model)
    kw = dict(x_T=x_T, verbose=False, noise_keys=_keys())
    guided = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    calls = [lambda: sampler.sample(S, B, SHAPE, cond, **kw)[0],
             lambda: sampler.sample(S, B, SHAPE, cond, mask=mask, x0=x0, **kw)[0],
             lambda: sampler.sample(S, B, SHAPE, cond, mask=mask, x0=x0, **guided, **kw)[0],
             lambda: sampler.decode(x_T, cond, 4, noise_keys=_keys())]
    begins, loads = [], []
    lib = L.get_context(0).lib
    orig = lib.upk_graph_begin
    monkeypatch.setattr(lib, "upk_graph_begin", lambda *a: (begins.append(1), orig(*a))[1], raising=False)
    load = upgpt_amd.engine.SamplerState.load_coefs
    monkeypatch.setattr(upgpt_amd.engine.SamplerState, "load_coefs", lambda self, *a, **k: (loads.append(1), load(self, *a, **k))[1])
    for call in calls:
        first = call()
        st = _state(model, call is calls[2])
        graphs, keep = dict(st.graphs), None if st.keep is None else st.keep.data_ptr()
        del begins[:], loads[:]
        second = call()
        assert not begins and not loads  # every graph is replayed, the table the state holds is the call's
        assert torch.equal(first, second)
        assert dict(st.graphs) == graphs and (None if st.keep is None else st.keep.data_ptr()) == keep
    # (a graph's key ends in the step variant it was captured for: engine.SamplerState.graph)
    assert {k[-1] for k in _state(model).graphs} == {None, "masked"}
    assert loads == [] and sampler.decode(x_T, cond, 3, noise_keys=_keys()) is not None and loads == [1]  # another table


def test_close_releases_the_keep_table():
    model, _ = get_model()
    _, cond, _, x_T = _case()
    x0, mask = _edit()
    DPMSolverSDESampler(model).sample(S, B, SHAPE, cond, x_T=x_T, mask=mask, x0=x0, verbose=False, noise_keys=_keys())
    st = _state(model)
    assert st.keep is not None and st.graphs
    plan = st.plan
    plan.close()
    assert st.keep is None and st.edit_mask is None and st.x_plain is None and not st.graphs
    assert not plan.sampler_states


def test_upscale_channel_layout_fast_against_general(monkeypatch):
    """C = 3 latent + 3 concat channels, 32x24, B = 1: the step kernel's element-wise xin rows inside the captured loop."""
    model, _ = get_model("upscale3")
    _, cond, _, x_T = _case(seed=7, hw=(32, 24), C=3, cc=3, b=1)
    keys = lambda: rng.NoiseKeys(5, [9], device="cuda")
    calls = _count_apply_model(model, monkeypatch)
    zf, _ = DPMSolverSDESampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False, noise_keys=keys())
    assert not calls and zf.shape == (1, 3, 32, 24) and torch.isfinite(zf).all()
    _general(monkeypatch)
    zg, _ = DPMSolverSDESampler(model).sample(S, 1, (3, 32, 24), cond, x_T=x_T, verbose=False, noise_keys=keys())
    assert len(calls) == S
    print("C = 3: latent mse fast vs general %.3e" % mse(zf, zg))
    assert mse(zf, zg) < 1e-4


def _batch():
    g0 = torch.Generator().manual_seed(3)
    return {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
            "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
            "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24)}


def test_log_images_inpaint_and_edit_images_run_on_the_captured_path(monkeypatch):
    model, _ = get_model()
    seen = []
    orig = DPMSolverSDESampler.sample
    monkeypatch.setattr(DPMSolverSDESampler, "sample", lambda self, *a, **k: (
        seen.append((a[0], k.get("eta"), k.get("mask") is not None)), orig(self, *a, **k))[1])
    calls = _count_apply_model(model, monkeypatch)
    torch.manual_seed(1)
    log = model.log_images(_batch(), N=B, sampler="dpmpp_2m_sde", ddim_steps=S, inpaint=True)
    assert seen == [(S, 1.0, False), (S, 1.0, True), (S, 1.0, True)]  # log_images' eta of 1 passes through
    for k in ("samples", "samples_inpainting", "samples_outpainting"):
        assert log[k].shape == (B, 3, 256, 192) and torch.isfinite(log[k]).all()
    keep = torch.ones(B, 1, 32, 24, device="cuda")
    keep[:, :, 8:24, 6:18] = 0.0
    out = model.edit_images(_batch(), keep, N=B, ddim_steps=S, ddim_eta=0.5, sampler="dpmpp_2m_sde",
                            noise_keys=rng.NoiseKeys(2, [0, 1], device="cuda"))
    assert seen[-1] == (S, 0.5, True) and torch.isfinite(out["samples"]).all()
    assert not calls


def test_edit_region_returns_the_input_outside_the_region():
    import test_edit_region_gpu as E
    from upgpt_amd.inference import InferenceModel
    model, _ = get_model()
    im = object.__new__(InferenceModel)
    im.device, im.model = E.DEV, model
    picture, segm = E.inputs()
    out = im.edit_region(picture, segm, "top", E.conditioning(), steps=3, sampler="dpmpp_2m_sde", dilate=E.DILATE,
                         feather=E.FEATHER, noise_keys=E.keys())
    assert out["edited"].shape == picture.shape and out["edited"].dtype == np.uint8
    outside = out["alpha"] == 0
    assert outside.any() and (~outside).any()
    assert np.array_equal(out["edited"][outside], picture[outside])  # the input's bytes wherever alpha is 0
    assert not np.array_equal(out["edited"][~outside], picture[~outside])
