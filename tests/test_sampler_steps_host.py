"""CPU pins of oracle/steps.py, the fp64 restatement of one launch of each sampler step kernel, and of its bound:
chained, the restatement reproduces the sampler oracles (oracle/ddim.py) and the model's own DDPM update; an fp32
evaluation in another association order stays inside 32 * 2^-24 * A on every input set the GPU test uses; and each
of eight deliberately wrong variants leaves it on at least 1 % of the elements of those same inputs."""
import numpy as np
import pytest
import torch

import upgpt_amd
from oracle import steps as st
from oracle.ddim import ddim_sample, plms_sample
from upgpt_amd import schedule

SHAPE = (2, 4, 6, 5)


def _smooth_eps(x, t, cond):
    tt = t.to(x.dtype).reshape(-1, 1, 1, 1)
    return 0.8 * torch.sin(1.3 * x + 0.013 * tt) + 0.1 * torch.cos(0.7 * x - 0.013 * tt) + cond


def _chain_tol(S, ref):
    """The table of schedule.ddim_coefficient_table holds fp32 1 / sqrt(a_t) where the sampler oracle divides by the
    fp32 sqrt(a_t) in fp64: one fp32 rounding (2^-24 relative) on pred_x0 per step, carried through S steps of a map
    whose gain is close to 1; 4 covers that gain and the fp32 sigma * noise product."""
    return 4.0 * max(S, 2) * 2.0 ** -24 * max(float(r.abs().max()) for r in ref)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("S,eta", [(50, 0.0), (50, 1.0), (10, 1.0)])
def test_ddim_steps_chain_to_ddim_sample(S, eta, guided):
    x_T, cond, uncond, noise = (t.double() for t in st.chain_inputs(SHAPE, S))
    ts, coefs, sig = st.kernel_tables(S, eta)
    table = sig[:, None] * noise.reshape(S, -1).float() if eta > 0 else None  # sigma_t * randn, fp32 as the sampler's
    x, xs, preds = x_T, [], []
    for i in range(S):
        t = torch.full((SHAPE[0],), int(ts[i]), dtype=torch.long)
        if guided:
            r = st.ddim_step_cfg(x, torch.stack([_smooth_eps(x, t, uncond), _smooth_eps(x, t, cond)]), coefs, table, i, 3.0)
        else:
            r = st.ddim_step(x, _smooth_eps(x, t, cond), coefs, table, i)
        assert r.commit and torch.equal(r.x, r.xin)
        x = r.x
        xs.append(r.x)
        preds.append(r.pred_x0)
    z, inter = ddim_sample(_smooth_eps, st.alphas_cumprod(), SHAPE, S, eta, x_T, noise=noise if eta > 0 else None,
                           cond=cond, uncond=uncond if guided else None, guidance_scale=3.0 if guided else 1.0, log_every_t=1)
    ref = inter["x_inter"][1:] + inter["pred_x0"][1:]
    assert z.dtype == torch.float64 and len(ref) == 2 * S
    tol = _chain_tol(S, ref)
    for got, want in zip(xs + preds, ref):
        assert float((got - want).abs().max()) <= tol
    assert float((x - z).abs().max()) <= tol


@pytest.mark.parametrize("S", [1, 2, 4, 5, 10, 50])
def test_plms_steps_chain_to_plms_sample(S):
    x_T, cond, _, _ = (t.double() for t in st.chain_inputs(SHAPE, S))
    ts, coefs, _ = st.kernel_tables(S, 0.0)
    n = x_T.numel()
    hist = torch.full((3, n), float("nan"), dtype=torch.float64)  # the ring needs no initialisation
    x, xs, preds = x_T, [], []
    for k in range(S + 1):
        t = torch.full((SHAPE[0],), int(ts[0] if k == 0 else ts[min(1, S - 1)] if k == 1 else ts[k - 1]), dtype=torch.long)
        if k == 0:
            r = st.plms_step(x, _smooth_eps(x, t, cond), coefs, 0, hist)
            assert not r.commit and torch.equal(r.x, x) and r.pred_x0 is None and r.slot == 0
            predictor = r.xin
        else:
            r = st.plms_step(x, _smooth_eps(predictor if k == 1 else x, t, cond), coefs, k, hist)
            assert r.commit and torch.equal(r.x, r.xin) and r.slot == (None if k == 1 else (k - 1) % 3)
            x = r.x
            xs.append(r.x)
            preds.append(r.pred_x0)
        hist = r.hist
    z, inter = plms_sample(_smooth_eps, st.alphas_cumprod(), SHAPE, S, x_T, cond=cond, log_every_t=1)
    ref = inter["x_inter"][1:] + inter["pred_x0"][1:]
    assert len(ref) == 2 * S
    tol = _chain_tol(S, ref)
    for got, want in zip(xs + preds, ref):
        assert float((got - want).abs().max()) <= tol
    assert float((x - z).abs().max()) <= tol


def test_ddpm_step_matches_the_models_update():
    """ddpm.py:1137-1148, 1178-1185 and 1282-1283 evaluated the reference's way (fp32 torch, its op order, the model's
    own predict_start_from_noise / q_posterior / q_sample) on the first, a middle, the t = 1 and the t = 0 row."""
    m = upgpt_amd.build_model("tiny")
    order = np.asarray([999, 500, 1, 0])
    tab = schedule.ddpm_coefficient_table(m, order)
    gen = torch.Generator().manual_seed(3)
    shape = (2, 4, 4, 3)
    x, mo, x0 = (1.5 * torch.randn(*shape, generator=gen) for _ in range(3))
    nz, nz2 = torch.randn(4, *shape, generator=gen), torch.randn(4, *shape, generator=gen)
    mask = torch.rand(*shape, generator=gen).round_(decimals=1)  # 0, 1 and values between
    for k, t in enumerate(order):
        tt = torch.full((shape[0],), int(t), dtype=torch.long)
        nonzero = (1 - (tt == 0).float()).reshape(-1, 1, 1, 1)
        for flags in range(4):
            for masked in (False, True):
                xr = mo.clone() if flags & st.UPK_DDPM_X0 else m.predict_start_from_noise(x, tt, mo)
                if flags & st.UPK_DDPM_CLIP:
                    xr.clamp_(-1.0, 1.0)
                mean, _, logvar = m.q_posterior(xr, x, tt)
                want = mean + nonzero * (0.5 * logvar).exp() * nz[k]
                if masked:
                    want = m.q_sample(x0, tt, noise=nz2[k]) * mask + (1.0 - mask) * want
                r = st.ddpm_step(x, mo, tab, nz, nz2 if masked else None, x0 if masked else None,
                                 mask if masked else None, k, flags)
                assert r.commit and torch.equal(r.x, r.xin)
                assert torch.allclose(r.pred_x0.float(), xr, rtol=1e-6, atol=1e-6), (t, flags, masked)
                assert torch.allclose(r.x.float(), want, rtol=1e-5, atol=1e-5), (t, flags, masked)
    r = st.ddpm_step(x, mo, tab, nz, None, x0, mask, 1, 0)  # a mask without the q_sample noise: row[5] * x0 alone
    plain = st.ddpm_step(x, mo, tab, nz, None, None, None, 1, 0)
    assert torch.allclose(r.x, tab[1, 5].double() * x0.double() * mask + (1.0 - mask.double()) * plain.x, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# the bound: an fp32 evaluation in ANOTHER association order than include/upk.h states passes it
# ---------------------------------------------------------------------------------------------------------------------
def _f32_update(x, e, row, nz):
    c0, c1, c2, c3 = (row[i] for i in range(4))
    p0 = x * c1 - (c0 * c1) * e
    xp = c3 * e + c2 * p0 if nz is None else (nz + c3 * e) + c2 * p0
    return xp, p0


def _f32_step(kernel, kw):
    """-> dict of fp32 outputs (x, pred_x0, xin, and e for the history slot)."""
    f = lambda t: None if t is None else t.float()
    x = f(kw["x"])
    n = x.numel()
    st_ = 0 if kw["step"] is None else int(kw["step"])
    row_of = lambda tab, i: None if tab is None else f(tab).reshape(-1, n)[i].reshape(x.shape)
    guided = lambda e2, s: (1.0 - s) * f(e2).reshape(2, *x.shape)[0] + s * f(e2).reshape(2, *x.shape)[1]
    if kernel in ("ddim", "ddim_cfg"):
        e = f(kw["eps"]).reshape(x.shape) if kernel == "ddim" else guided(kw["eps2"], kw["scale"])
        xp, p0 = _f32_update(x, e, f(kw["coefs"])[st_], row_of(kw["noise"], st_))
        return {"x": xp, "pred_x0": p0, "xin": xp}
    if kernel == "plms":
        e = guided(kw["eps"], kw["cfg_scale"]) if kw["cfg"] else f(kw["eps"]).reshape(x.shape)
        H = f(kw["hist"]).reshape(3, *x.shape)
        k = st_
        j = max(k - 1, 0)
        h1, h2, h3 = (H[(j - i) % 3] for i in (1, 2, 3))
        if k == 0:
            ep = e
        elif k == 1:
            ep = 0.5 * e + 0.5 * H[0]
        elif j == 1:
            ep = e + 0.5 * (e - h1)
        elif j == 2:
            ep = (5.0 / 12.0) * h2 + ((23.0 / 12.0) * e - (16.0 / 12.0) * h1)
        else:
            ep = ((55.0 / 24.0) * e - (9.0 / 24.0) * h3) + ((37.0 / 24.0) * h2 - (59.0 / 24.0) * h1)
        xp, p0 = _f32_update(x, ep, f(kw["coefs"])[j], None)
        return {"x": x if k == 0 else xp, "pred_x0": None if k == 0 else p0, "xin": xp, "e": e}
    r, m = f(kw["coefs"])[st_], f(kw["model_out"])
    xr = m if kw["flags"] & st.UPK_DDPM_X0 else -(r[1] * m - r[0] * x)
    if kw["flags"] & st.UPK_DDPM_CLIP:
        xr = xr.clamp(-1.0, 1.0)
    nz = row_of(kw["noise"], st_)
    xp = r[3] * x + r[2] * xr if nz is None else (r[4] * nz + r[3] * x) + r[2] * xr
    if kw["mask"] is not None:
        q = r[5] * f(kw["x0"]).reshape(x.shape)
        if kw["noise2"] is not None:
            q = r[6] * row_of(kw["noise2"], st_) + q
        xp = xp + f(kw["mask"]).reshape(x.shape) * (q - xp)
    return {"x": xp, "pred_x0": xr, "xin": xp}


@pytest.mark.parametrize("shape", st.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kernel", st.KERNELS)
def test_bound_admits_an_fp32_evaluation(kernel, shape):
    inp = st.make_inputs(kernel, shape)
    for mode in st.modes(kernel):
        if kernel == "plms" and mode["step"] is None:
            continue
        kw = st.operands(kernel, inp, mode)
        ref, got = st.STEP_FNS[kernel](**kw), _f32_step(kernel, kw)
        for name in ("x", "pred_x0", "xin"):
            if got[name] is not None:
                assert bool(st.within(got[name], getattr(ref, name), ref.A[name]).all()), (kernel, shape, mode, name)
        if ref.slot is not None:
            assert bool(st.within(got["e"], ref.hist[ref.slot], ref.A["hist"][ref.slot]).all()), (kernel, shape, mode)


# ---------------------------------------------------------------------------------------------------------------------
# the bound rejects the mutants: each is the correct fp64 step on operands altered so that it computes the wrong thing
# ---------------------------------------------------------------------------------------------------------------------
def _slot(kw, back):
    return (max(int(kw["step"]) - 1, 0) - back) % 3


def _scaled_h2(kw):  # Adams-Bashforth 4: 37 h2 -> 36 h2
    h = kw["hist"].double().clone()
    h[_slot(kw, 2)] *= 36.0 / 37.0
    return dict(kw, hist=h)


def _h2_from_h1(kw):
    h = kw["hist"].double().clone()
    h[_slot(kw, 2)] = h[_slot(kw, 1)]
    return dict(kw, hist=h)


def _euler_e_only(kw):  # (e0 + e) / 2 -> e
    h = kw["hist"].double().clone()
    e = kw["eps"].double()
    h[0] = (e[0] + kw["cfg_scale"] * (e[1] - e[0])).reshape(-1) if kw["cfg"] else e.reshape(-1)
    return dict(kw, hist=h)


def _swap56(kw):
    c = kw["coefs"].clone()
    c[:, 5], c[:, 6] = kw["coefs"][:, 6], kw["coefs"][:, 5]
    return dict(kw, coefs=c)


def _more_guidance(kw):  # e_c + s (e_c - e_u) = e_u + (s + 1) (e_c - e_u)
    key = "scale" if "scale" in kw else "cfg_scale"
    return dict(kw, **{key: kw[key] + 1.0})


MUTANTS = [
    # name, kernels, applies to (kernel, mode), operands -> mutated operands
    ("AB4 coefficient 37 -> 36", ("plms",), lambda m: m["step"] >= 4, _scaled_h2),
    ("h2 read from h1's slot", ("plms",), lambda m: m["step"] >= 3, _h2_from_h1),
    ("Euler pair (e0 + e)/2 -> e", ("plms",), lambda m: m["step"] == 1, _euler_e_only),
    ("the noise row of step - 1", ("ddim", "ddim_cfg", "ddpm"), lambda m: m["noise"],
     lambda kw: dict(kw, noise=torch.roll(kw["noise"], 1, 0))),
    ("cf[5] and cf[6] swapped in the masked blend", ("ddpm",), lambda m: m["mask"] is not None, _swap56),
    ("no clamp", ("ddpm",), lambda m: m["flags"] & st.UPK_DDPM_CLIP, lambda kw: dict(kw, flags=kw["flags"] & ~st.UPK_DDPM_CLIP)),
    ("guidance e_u + s (e_c - e_u) -> e_c + s (e_c - e_u)", ("ddim_cfg", "plms"), lambda m: m.get("cfg", True), _more_guidance),
    ("UPK_DDPM_X0 ignored", ("ddpm",), lambda m: m["flags"] & st.UPK_DDPM_X0, lambda kw: dict(kw, flags=kw["flags"] & ~st.UPK_DDPM_X0)),
]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_bound_rejects_the_mutant(mutant):
    name, kernels, applies, mutate = mutant
    seen = 0
    for kernel in kernels:
        for shape in st.SHAPES:
            inp = st.make_inputs(kernel, shape)
            for mode in st.modes(kernel):
                if (kernel == "plms" and mode["step"] is None) or not applies(mode):
                    continue
                kw = st.operands(kernel, inp, mode)
                ref, bad = st.STEP_FNS[kernel](**kw), st.STEP_FNS[kernel](**mutate(kw))
                out = ~st.within(bad.xin, ref.xin, ref.A["xin"])
                if ref.commit:
                    out |= ~st.within(bad.x, ref.x, ref.A["x"]) | ~st.within(bad.pred_x0, ref.pred_x0, ref.A["pred_x0"])
                if ref.slot is not None:
                    out |= ~st.within(bad.hist[ref.slot], ref.hist[ref.slot], ref.A["hist"][ref.slot])
                assert float(out.double().mean()) >= 0.01, (name, kernel, shape, mode, float(out.double().mean()))
                seen += 1
    assert seen >= len(st.SHAPES)


# ---------------------------------------------------------------------------------------------------------------------
# the chain tolerance of tests/test_sampler_steps_gpu.py is what the reference's own fp32 evaluation needs, times four
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_tolerance_is_the_references_own_error_times_four():
    """The GPU chains are held to st.CHAIN_TOL = 4 x the recorded fp32-vs-fp64 deviation of the sampler oracles.  fp16
    rounding flips of the stem input make the figure depend on the host's libm to within a small factor, so the
    re-measurement must pass the bound itself, and the bound may not be more than 16 x what is re-measured."""
    assert st.CHAIN_TOL == 4.0 * st.CHAIN_MEASURED
    measured = st.measure_chain_tolerance()
    assert measured <= st.CHAIN_TOL <= 16.0 * measured, measured
