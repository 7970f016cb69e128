"""Sampling with keyed noise (noise_keys=, upgpt_amd/rng.py) on a real MI355X: a keyed DDIM call is BIT-equal to the same
call through the existing injected-noise path (x_T=, normals_sequence=, q_sample's noise) fed the keyed normals, with and
without guidance and a mask; the captured-loop and the step-by-step paths agree under keys by the criteria the existing
fast-vs-general tests use (mse < 1e-4 for DDIM, tests/test_ddim_edit_gpu.py; < 1e-6 for the DDPM chain,
tests/test_ddpm_gpu.py); the torch generator is left alone; a warm keyed call never enters host_io()."""
import numpy as np
import pytest
import torch

import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import rng, synth
from upgpt_amd.ddim import DDIMSampler
from upgpt_amd.plms import PLMSSampler

pytestmark = pytest.mark.gpu
HW, C, B, S = (32, 24), 4, 2, 4
SHAPE = (B, C) + HW
_cache = {}


def get_model():
    if "m" not in _cache:
        m = upgpt_amd.build_model("tiny")
        synth.fill_module_(m)
        _cache["m"] = m.cuda()
    return _cache["m"]


def case(seed=5):
    inp = synth.synth_inputs(B, HW, C, 87, 768, seed=seed)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    x0 = (0.7 * synth.synth_inputs(B, HW, C, 87, 768, seed=seed + 1)["x_T"]).cuda()
    mask = torch.ones(B, 1, *HW, device="cuda")  # the centre is filled in (0), the border kept (1)
    mask[:, :, HW[0] // 4:3 * HW[0] // 4, HW[1] // 4:3 * HW[1] // 4] = 0.
    return cond, uc, x0, mask


def keys(draw=0):
    return rng.NoiseKeys(77, [12, 5], device="cuda:0", draw=draw)


def mse(a, b):
    return float(((a.float() - b.float()) ** 2).mean())


def keyed_tables(K):
    x_T = rng.randn(K, SHAPE, rng.STREAM_XT)
    steps = torch.stack([rng.randn(K, SHAPE, rng.STREAM_STEP, row0=i) for i in range(S)])
    qs = [rng.randn(K, SHAPE, rng.STREAM_QSAMPLE, row0=i) for i in range(S)]
    return x_T, steps, qs


def same_bits(a, b):
    (za, ia), (zb, ib) = a, b
    assert torch.equal(za, zb) and torch.isfinite(za).all()
    for k in ("x_inter", "pred_x0"):
        assert len(ia[k]) == len(ib[k]) == S + 1
        assert all(torch.equal(u, v) for u, v in zip(ia[k], ib[k])), k


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "cfg"])
def test_keyed_sample_is_bit_equal_to_the_injected_path(guided):
    model = get_model()
    cond, uc, _, _ = case()
    K = keys()
    kw = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc) if guided else {}
    run = lambda **n: DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, log_every_t=1, **kw, **n)
    x_T, steps, _ = keyed_tables(K)
    keyed = run(noise_keys=K)
    same_bits(keyed, run(x_T=x_T, normals_sequence=steps))
    # a sample's chain does not depend on its neighbour, another draw is another chain
    assert mse(keyed[0], run(noise_keys=K.fork(1))[0]) > 1e-3
    assert torch.equal(run(noise_keys=K, x_T=x_T)[0], keyed[0])  # (a given x_T is used; the step noise stays keyed)


def test_keyed_masked_sample_is_bit_equal_to_the_injected_path(monkeypatch):
    """What the existing masked-path tests inject: x_T, the step normals, and q_sample's noise by timestep."""
    model = get_model()
    cond, uc, x0, mask = case()
    K = keys(draw=2)
    x_T, steps, qs = keyed_tables(K)
    run = lambda **n: DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, log_every_t=1, mask=mask,
                                                x0=x0, **n)
    keyed = run(noise_keys=K)
    s = DDIMSampler(model)
    s.make_schedule(ddim_num_steps=S, ddim_eta=1.0, verbose=False)
    by_t = {int(t): qs[i] for i, t in enumerate(np.asarray(s.ddim_timesteps)[::-1])}  # loop position i runs timestep t
    q_orig = type(model).q_sample
    monkeypatch.setattr(model, "q_sample", lambda x_start, t, noise=None: q_orig(model, x_start, t, by_t[int(t[0])]),
                        raising=False)
    same_bits(keyed, run(x_T=x_T, normals_sequence=steps))


def test_keyed_fast_path_equals_the_step_by_step_path(monkeypatch):
    model = get_model()
    cond, uc, x0, mask = case(seed=8)
    K = keys()
    guided = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    calls = []
    orig = model.apply_model
    monkeypatch.setattr(model, "apply_model", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)

    def runs():
        out = []
        for kw in (dict(), guided, dict(mask=mask, x0=x0), dict(mask=mask, x0=x0, **guided)):
            out.append(DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, log_every_t=1,
                                                 noise_keys=K, **kw))
        s = DDIMSampler(model)  # a tail chain: rows S - 3 .. S - 1 of the same tables
        s.make_schedule(ddim_num_steps=S, ddim_eta=1.0, verbose=False)
        out.append((s.decode(x0, cond, 3, noise_keys=K), {"x_inter": [], "pred_x0": []}))
        return out

    fast = runs()
    assert not calls, "the fast path called apply_model"
    # noise_dropout > 0 / a score corrector take the step-by-step path under keys too; here it is forced for every call
    monkeypatch.setattr(DDIMSampler, "_fast_ok", lambda self, *a, **k: False)
    slow = runs()
    assert len(calls) == 4 * S + 3
    for i, ((za, ia), (zb, ib)) in enumerate(zip(fast, slow)):
        errs = [mse(u, v) for k in ("x_inter", "pred_x0") for u, v in zip(ia[k], ib[k])] + [mse(za, zb)]
        print("case %d: mse fast vs step-by-step, worst %.3e" % (i, max(errs)))
        assert max(errs) < 1e-4 and len(ia["x_inter"]) == len(ib["x_inter"]), (i, errs)
    assert mse(fast[0][0], fast[1][0]) > 1e-6 and mse(fast[0][0], fast[2][0]) > 1e-6


class _Identity:
    def modify_score(self, model, e_t, x, t, c, **kw):
        return e_t


def test_keyed_ddpm_chain_fast_vs_step_by_step():
    model = get_model()
    cond, _, x0, _ = case(seed=9)
    mask = torch.ones(B, 1, *HW, device="cuda")
    mask[:, :, 8:24, 6:18] = 0.
    K = keys(draw=3)
    T = 6
    for kw in (dict(), dict(mask=mask, x0=x0), dict(temperature=0.7)):
        run = lambda **n: model.progressive_denoising(cond, (C,) + HW, verbose=False, batch_size=B, start_T=T,
                                                      log_every_t=2, noise_keys=K, **kw, **n)
        (zf, xf), (zg, xg) = run(), run(score_corrector=_Identity())
        errs = [mse(zf, zg)] + [mse(a, b) for a, b in zip(xf, xg)]
        print("ddpm %s: worst mse %.3e" % (sorted(kw), max(errs)))
        assert len(xf) == len(xg) and max(errs) < 1e-6 and torch.isfinite(zf).all()
    a = model.p_sample_loop(cond, SHAPE, verbose=False, timesteps=T, noise_keys=K)
    assert torch.equal(a, model.p_sample_loop(cond, SHAPE, verbose=False, timesteps=T, noise_keys=K))
    assert mse(a, model.p_sample_loop(cond, SHAPE, verbose=False, timesteps=T, noise_keys=K.fork(4))) > 1e-3


def test_a_sample_does_not_depend_on_its_batch_position_noise():
    """The noise a sample is given is that of its key, wherever it sits: swapping the keys swaps the rows."""
    K = keys()
    swapped = rng.NoiseKeys(77, [5, 12], device="cuda:0")
    a, b = rng.randn(K, SHAPE, rng.STREAM_XT), rng.randn(swapped, SHAPE, rng.STREAM_XT)
    assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0])


def test_generator_state_is_untouched_by_keyed_calls():
    model = get_model()
    cond, uc, x0, mask = case()
    K = keys()
    torch.manual_seed(3)
    before = torch.cuda.get_rng_state()
    DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, noise_keys=K)
    DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, noise_keys=K, mask=mask, x0=x0)
    PLMSSampler(model).sample(S, B, (C,) + HW, cond, verbose=False, noise_keys=K)
    model.p_sample_loop(cond, SHAPE, verbose=False, timesteps=3, noise_keys=K)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    DDIMSampler(model).sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False)  # without keys: S + 1 draws, as before
    assert not torch.equal(torch.cuda.get_rng_state(), before)


def test_a_warm_keyed_call_never_enters_host_io(monkeypatch):
    """Everything on the device, schedule / scale tables and graphs warm: with a pool alive (so that host_io() is a real
    lock) the keyed fast path does not enter it; the unkeyed call at eta = 1 does, for its draws."""
    import contextlib

    from upgpt_amd import chain as chain_mod
    from upgpt_amd import ddim as ddim_mod
    from upgpt_amd import engine
    model = get_model()
    cond, _, _, _ = case()
    K = keys()
    sampler = DDIMSampler(model)
    run = lambda **n: sampler.sample(S, B, (C,) + HW, cond, eta=1.0, verbose=False, **n)
    entered = []
    orig = L.host_io

    @contextlib.contextmanager
    def counted():
        entered.append(1)
        with orig():
            yield

    with L.shared_chip(2):  # (host_io() is live, as inside a lane of a pool)
        warm = run(noise_keys=K)[0]
        assert engine.L is L  # (the graph capture reaches the lock as L.host_io)
        for mod in (L, ddim_mod, chain_mod):
            monkeypatch.setattr(mod, "host_io", counted)
        again = run(noise_keys=K)[0]
        assert not entered, "a warm keyed call took the host_io lock"
        assert torch.equal(warm, again)
        run()
        assert entered, "the unkeyed eta = 1 call is expected to take the lock for its draws"


def test_log_images_with_keys_forks_per_call_and_leaves_the_generator_alone():
    """noise_keys= on log_images: 'samples' is draw 0 of the keys cut to the n samples produced, the in- and outpainting are
    draws 1 and 2 (different pictures of one task), the reconstruction's posterior sample is keyed too; a repeat gives
    the same bits whatever the generator's state, a sample's pictures do not depend on its neighbour's key, and the keyed
    'samples' equal the sampler called with fork(0) on the same conditioning."""
    model = get_model()
    g0 = torch.Generator().manual_seed(3)
    n = 3
    batch = {"image": (torch.rand(n, 256, 192, 3, generator=g0) * 2 - 1).cuda(),
             "txt": torch.randn(n, 77, 768, generator=g0).cuda(), "styles": (0.45 * torch.randn(n, 9, 768, generator=g0)).cuda(),
             "smpl": (0.5 * torch.randn(n, 1, 85, generator=g0)).cuda(), "person_mask": synth.person_mask(n, 32, 24).cuda()}
    K = rng.NoiseKeys(21, [4, 9, 2], device="cuda:0")
    run = lambda keys, **kw: model.log_images(batch, N=2, ddim_steps=S, ddim_eta=1.0, inpaint=True, noise_keys=keys, **kw)
    torch.manual_seed(1)
    before = torch.cuda.get_rng_state()
    a = run(K)  # (three keys for N = 2 samples: the keys are cut, not refused)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    torch.manual_seed(2)
    b = run(K)
    for k in ("reconstruction", "samples", "samples_inpainting", "samples_outpainting"):
        assert a[k].shape == (2, 3, 256, 192) and torch.equal(a[k], b[k]), k
    assert not torch.equal(a["samples_inpainting"], a["samples_outpainting"])
    assert not torch.equal(a["samples"][0], a["samples"][1])
    # sample 0 keeps its noise when its neighbour's key changes (the latent; pictures share GEMM tiles over the batch)
    z, cond, *_ = model.get_input(batch, model.first_stage_key, return_first_stage_outputs=True, force_c_encode=True,
                                  return_original_cond=True, bs=2, noise_keys=K)
    z2 = model.get_input(batch, model.first_stage_key, bs=2, noise_keys=rng.NoiseKeys(21, [4, 77], device="cuda:0"))[0]
    assert torch.equal(z[0], z2[0]) and not torch.equal(z[1], z2[1])
    with model.ema_scope():
        zs, _ = DDIMSampler(model).sample(S, 2, (C,) + HW, cond, eta=1.0, verbose=False, noise_keys=K[:2].fork(0))
    assert torch.equal(model.decode_first_stage(zs), a["samples"])
    with pytest.raises(ValueError, match="keys"):
        run(K[:1])
