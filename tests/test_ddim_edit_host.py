"""DDIM editing on the captured-graph path, the parts that need no GPU: the C ABI declares and exports the new step
entry, DDIMSampler._fast_ok lets a masked call through, and the kernel's contract (tests/edit_ref.py, fp64) chained the
way the sampler chains it reproduces oracle.ddim's masked sampling and decode on a toy denoiser — the blend placed at the
end of the step before, the unblended last step, the start row."""
import os
import re

import numpy as np
import pytest
import torch

import edit_ref as er
from oracle import ddim as o_ddim
from oracle import steps as st
from upgpt_amd import _lib
from upgpt_amd.ddim import DDIMSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "upk_ddim_step_edit_f32"


def test_header_declares_and_library_exports_the_edit_step():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    assert NAME in set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    assert NAME in _lib.SYMBOLS
    lib = _lib.load_library()
    assert hasattr(lib, NAME) and lib.upk_version() == 100  # additive: the ABI version stays
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 19  # ctx + 18 (include/upk.h)
    # the auto-advance note names every step kernel that honours it
    note = header[header.index("With done != NULL"):header.index("int upk_step_autoadvance")]
    assert NAME in note
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


class _Model:
    num_timesteps = 1000

    def _split_cond(self, c):
        return None, c


def test_fast_ok_accepts_a_mask_and_still_rejects_the_rest():
    s = DDIMSampler(_Model())
    cond, mask = {"c_crossattn": torch.zeros(1, 2, 3)}, torch.ones(1, 1, 4, 4)
    ok = lambda **kw: s._fast_ok(**dict(dict(cond=cond, ddim_use_original_steps=False, quantize_denoised=False, mask=None,
                                             noise_dropout=0., score_corrector=None, ucg_scale=1., uc=None), **kw))
    assert ok() and ok(mask=mask)
    assert ok(mask=mask, ucg_scale=3., uc=dict(cond))
    assert not ok(mask=mask, noise_dropout=0.1)
    assert not ok(mask=mask, score_corrector=object())
    assert not ok(mask=mask, ddim_use_original_steps=True)
    assert not ok(mask=mask, quantize_denoised=True)
    assert not ok(mask=mask, ucg_scale=3., uc=torch.zeros(1, 2, 3))  # guided conditioning of another type
    assert not ok(mask=mask, cond=None)


def test_a_chain_that_is_not_a_tail_of_the_schedule_stays_on_the_general_path():
    s = DDIMSampler(_Model())
    s.ddim_timesteps = np.arange(1, 1000, 100)
    assert s._is_tail(s.ddim_timesteps) and s._is_tail(s.ddim_timesteps[:6]) and s._is_tail(s.ddim_timesteps[:1])
    assert not s._is_tail(s.ddim_timesteps[:0])       # decode(t_start = 0): nothing to run
    assert not s._is_tail(s.ddim_timesteps[2:])       # not the LAST steps of the loop
    assert not s._is_tail(np.arange(1, 1200, 100))    # longer than the schedule


def test_mask_without_x0_raises_like_the_general_path():
    s = DDIMSampler(_Model())
    s.ddim_timesteps = np.arange(1, 1000, 100)
    with pytest.raises(ValueError, match="mask given without x0"):
        s._fast_sampling({"c_crossattn": torch.zeros(1, 2, 3)}, (1, 4, 4, 4), None, s.ddim_timesteps, None, None, 100, 1.,
                         None, mask=torch.ones(1, 1, 4, 4), x0=None)


# ------------------------------------------------------------------------------------------ the kernel's contract, chained
def toy_eps(x, t, cond):
    """oracle/steps.py's smooth bounded denoiser without its fp16 rounding of the latent: both sides run in fp64 here
    and have to agree far below a rounding flip."""
    tt = t.to(x.dtype).reshape(-1, *([1] * (x.dim() - 1)))
    return 0.8 * torch.sin(1.3 * x + 0.013 * tt) + 0.1 * torch.cos(0.7 * x - 0.013 * tt) + cond.to(x.dtype)


def _tol(S, eta):
    """The restatement reads the fp32 coefficient rows the kernel reads (upgpt_amd.schedule.ddim_coefficient_table), the
    oracle forms the same four factors in fp64 from fp32 alphas: up to 2^-24 relative on each of 4 coefficients per step
    (a few for the sqrt / reciprocal chains behind them: 2 each), S steps, each amplified by at most max 1/sqrt(a_t) on
    its way through pred_x0; the toy denoiser's Lipschitz constant (~1.1) is covered by a further factor 2.  Relative
    to max |z|."""
    c1 = float(st.kernel_tables(S, eta)[1][:, 1].max())
    return 2 * 2 * 4 * S * 2.0 ** -24 * c1


def _masked_case(shape, S, eta, guided, seed=0):
    g = torch.Generator().manual_seed(900 + seed + S)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x_T, x0 = rn(*shape), 0.7 * rn(*shape)
    cond, uncond = 0.1 * rn(*shape), 0.1 * rn(*shape)
    noise, qnoise = rn(S, *shape), rn(S, *shape)
    B, _, H, W = shape
    mask = torch.ones(B, 1, H, W, dtype=torch.float64)
    mask[:, :, H // 4:3 * H // 4, W // 4:3 * W // 4] = 0.0
    mask[:, :, 0, 0] = 0.35  # a soft edge
    return dict(x_T=x_T, x0=x0, cond=cond, uncond=uncond if guided else None, noise=noise, qnoise=qnoise, mask=mask)


@pytest.mark.parametrize("S,eta,guided", [(10, 0.0, False), (10, 1.0, False), (10, 0.0, True), (50, 1.0, True)])
def test_chained_restatement_reproduces_the_oracles_masked_sampling(S, eta, guided):
    shape = (2, 4, 6, 5)
    c = _masked_case(shape, S, eta, guided)
    acp = st.alphas_cumprod()
    scale = 3.0 if guided else 1.0
    z_ref, inter = o_ddim.ddim_sample(toy_eps, acp, shape, S, eta, c["x_T"], noise=c["noise"] if eta > 0 else None,
                                      cond=c["cond"], uncond=c["uncond"], guidance_scale=scale, log_every_t=1,
                                      mask=c["mask"], x0=c["x0"], q_sample=er.q_sample_fn(acp, c["qnoise"]))
    z, xs, preds = er.edit_chain(toy_eps, S, eta, c["x_T"], c["cond"], c["uncond"], scale, c["noise"], c["mask"],
                                 c["x0"], er.q_sample_fn(acp, c["qnoise"]))
    assert len(xs) == len(inter["x_inter"]) - 1 == S
    ref = (z_ref, inter["x_inter"][1:], inter["pred_x0"][1:])
    dev = st.chain_deviation((z, xs, preds), ref)
    print("masked chain S=%d eta=%g guided=%d: deviation / max|z| = %.3e (bound %.3e)" % (S, eta, guided, dev, _tol(S, eta)))
    assert dev <= _tol(S, eta)
    # the last step's result is the unblended one
    assert torch.equal(z, xs[-1])


def test_the_placement_matters_to_the_bound():
    """Power of the chain test: the blend with the row of the SAME step, a blended last step, or rows filled in another
    order each miss the bound by more than a factor of ten."""
    S, eta, shape = 10, 0.0, (2, 4, 6, 5)
    c = _masked_case(shape, S, eta, False)
    acp = st.alphas_cumprod()
    z_ref, inter = o_ddim.ddim_sample(toy_eps, acp, shape, S, eta, c["x_T"], cond=c["cond"], log_every_t=1,
                                      mask=c["mask"], x0=c["x0"], q_sample=er.q_sample_fn(acp, c["qnoise"]))
    ref = (z_ref, inter["x_inter"][1:], inter["pred_x0"][1:])
    real = er.ddim_step_edit

    def run(step_fn, qnoise):
        er.ddim_step_edit = step_fn
        try:
            return er.edit_chain(toy_eps, S, eta, c["x_T"], c["cond"], None, 1.0, None, c["mask"], c["x0"],
                                 er.q_sample_fn(acp, qnoise))
        finally:
            er.ddim_step_edit = real

    def same_row(x, eps, coefs, noise, keep, mask, n_rows, step, scale, cfg):
        return real(x, eps, coefs, noise, torch.roll(keep, 1, 0), mask, n_rows, step, scale, cfg)

    def blended_last(x, eps, coefs, noise, keep, mask, n_rows, step, scale, cfg):
        return real(x, eps, coefs, noise, torch.cat([keep, keep[-1:]]), mask, n_rows + 1, step, scale, cfg)

    assert st.chain_deviation(run(real, c["qnoise"]), ref) <= _tol(S, eta)
    assert st.chain_deviation(run(same_row, c["qnoise"]), ref) > 10 * _tol(S, eta)
    assert st.chain_deviation(run(blended_last, c["qnoise"]), ref) > 10 * _tol(S, eta)
    assert st.chain_deviation(run(real, c["qnoise"].flip(0)), ref) > 10 * _tol(S, eta)


@pytest.mark.parametrize("t_start,guided", [(6, False), (6, True), (1, False), (10, True)])
def test_a_chain_from_a_start_row_reproduces_the_oracles_decode(t_start, guided):
    """decode(x_latent, cond, t_start) = the last t_start rows of the S-row tables, the step counter preset to
    S - t_start; no mask: the kernel is the plain update."""
    S, shape = 10, (2, 4, 6, 5)
    c = _masked_case(shape, S, 0.0, guided, seed=3)
    acp = st.alphas_cumprod()
    scale = 2.5 if guided else 1.0
    ref = o_ddim.ddim_decode(toy_eps, acp, c["x_T"], S, t_start, c["cond"], uncond=c["uncond"], guidance_scale=scale)
    z, xs, _ = er.edit_chain(toy_eps, S, 0.0, c["x_T"], c["cond"], c["uncond"], scale, t_steps=t_start)
    assert len(xs) == t_start
    dev = float((z - ref).abs().max() / ref.abs().max())
    print("decode t_start=%d guided=%d: deviation / max|z| = %.3e (bound %.3e)" % (t_start, guided, dev, _tol(S, 0.0)))
    assert dev <= _tol(S, 0.0)


def test_single_launch_restatement_modes():
    """The restatement itself: mask == NULL is oracle/steps.py's DDIM update (guided and not), the last row is never
    blended, x_plain is the unblended value, and the blend reads row step + 1."""
    inp = er.make_inputs(st.SHAPES[1])
    for mode in er.modes():
        r = er.ddim_step_edit(**er.operands(inp, mode))
        base = (st.ddim_step_cfg(inp["x"], inp["eps"], inp["coefs"], inp["noise"] if mode["noise"] else None, mode["step"],
                                 er.SCALE) if mode["cfg"] else
                st.ddim_step(inp["x"], inp["eps"][0], inp["coefs"], inp["noise"] if mode["noise"] else None, mode["step"]))
        assert torch.equal(r.x_plain, base.x) and torch.equal(r.pred_x0, base.pred_x0), mode
        row = 0 if mode["step"] is None else mode["step"]
        if not mode["mask"] or row == er.ROWS - 1:
            assert torch.equal(r.x, base.x) and torch.equal(r.A["x"], base.A["x"]), mode
        else:
            mk = inp["mask"].double().reshape(base.x.shape)
            kp = inp["keep"][row + 1].double().reshape(base.x.shape)
            assert torch.equal(r.x, mk * kp + (1 - mk) * base.x), mode
            assert torch.equal(r.x[mk == 0], base.x[mk == 0]) and torch.equal(r.x[mk == 1], kp[mk == 1]), mode
            assert bool((r.A["x"] >= r.x.abs() - 1e-12).all()), mode
