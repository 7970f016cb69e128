"""fp64 restatement of ONE launch of each sampler step kernel (test oracle), with its rounding-error bound.

Written from the reference's sampler text and from the contract in include/upk.h:
  ddim_step      ldm/models/diffusion/ddim.py:165-204 (p_sample_ddim; the update is 189-203)
  ddim_step_cfg  the same with the guidance combination of ddim.py:173-178
  plms_step      ldm/models/diffusion/plms.py:177-236 (p_sample_plms; one call = one model evaluation)
  ddpm_step      ldm/models/diffusion/ddpm.py:1125-1187 (p_mean_variance, p_sample) and the masked blend of
                 ddpm.py:1282-1283 (q_sample at the SAME t)

Every function takes the operands of its C entry point (fp32 or fp64 torch tensors, any device) and returns a
StepResult holding, in float64 on the CPU, everything the launch may write: the new x, pred_x0, the values destined
for the UNet stem input xin BEFORE their fp16 rounding, the new eps history ring (PLMS), and whether x / pred_x0 are
committed (PLMS evaluation 0 commits neither: its predictor lives in xin only).

The bound.  Next to each output the result carries its elementwise magnitude A (StepResult.A[name]): the same
expression evaluated with every coefficient and operand replaced by its absolute value and every subtraction by an
addition.  Every intermediate of an fp32 evaluation, in whatever association order, is bounded by A (up to second
order), and each fp32 rounding adds at most 2^-24 relative to such an intermediate.  The longest path is PLMS with
guidance at order 4: 3 roundings for e_u + s (e_c - e_u), 8 for the four products and three sums / one scaling of
Adams-Bashforth, 6 for (x - c0 e) c1 and c2 p0 + c3 e: 17.  So a correct fp32 kernel satisfies

    |got - ref64| <= BOUND * A   elementwise,   BOUND = 32 * 2^-24,

32 being roughly double the count, which covers the second-order terms and the fp32-rounded constants 1/12 and 1/24
(one more relative 2^-24 each); FMA contraction only removes roundings.  The one constant serves all four kernels
(the others have shorter paths).  Where the launch does not write an element (an uncommitted x, a history slot the
step does not own) A is 0: the element must come back exactly.

The module also holds the seeded input sets and mode lists the host and the GPU tests share (make_inputs / modes /
operands / run), and the synthetic-denoiser chain cases with the measurement of their tolerance
(`python -m oracle.steps` prints it).
"""
import numpy as np
import torch

BOUND = 32.0 * 2.0 ** -24

UPK_DDPM_X0, UPK_DDPM_CLIP = 0x1, 0x2  # include/upk.h


class StepResult:
    """x, pred_x0, xin, hist: float64 CPU tensors (hist None outside PLMS); commit: bool; A: dict name -> magnitude;
    slot: the history slot the launch owns (None: none)."""

    def __init__(self, x, pred_x0, xin, A, hist=None, commit=True, slot=None):
        self.x, self.pred_x0, self.xin, self.hist, self.commit, self.slot, self.A = x, pred_x0, xin, hist, commit, slot, A


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


def _row(coefs, step, width):
    st = 0 if step is None else int(step)
    return st, _d(coefs).reshape(-1, width)[st]


def _table_row(table, st, like):
    return None if table is None else _d(table).reshape(-1, like.numel())[st].reshape(like.shape)


def within(got, ref, A, bound=BOUND):
    """Elementwise |got - ref| <= bound * A, as a bool tensor (got: any float dtype / device)."""
    return (_d(got).reshape(ref.shape) - ref).abs() <= bound * A


def _ddim_update(x, e, Ae, row, nz):
    """ddim.py:196-203 / plms.py:206-216 with the table row {sqrt(1-a_t), 1/sqrt(a_t), sqrt(a_prev),
    sqrt(1-a_prev-sigma^2)} of include/upk.h; nz: sigma_t * temperature * randn (already scaled) or None."""
    c0, c1, c2, c3 = (row[i] for i in range(4))
    pred_x0 = (x - c0 * e) * c1
    x_prev = c2 * pred_x0 + c3 * e
    A_p = (x.abs() + c0.abs() * Ae) * c1.abs()
    A_x = c2.abs() * A_p + c3.abs() * Ae
    if nz is not None:
        x_prev = x_prev + nz
        A_x = A_x + nz.abs()
    return x_prev, pred_x0, A_x, A_p


def _guided(eps2, like, scale):
    """ddim.py:174-178 / plms.py:182-186: [unconditional ; conditional] -> e_u + scale (e_c - e_u)."""
    e2 = _d(eps2).reshape(2, *like.shape)
    e_u, e_c = e2[0], e2[1]
    s = float(scale)
    return e_u + s * (e_c - e_u), e_u.abs() + abs(s) * (e_c.abs() + e_u.abs())


def ddim_step(x, eps, coefs, noise=None, step=None):
    """upk_ddim_step_f32: one p_sample_ddim update (ddim.py:189-203)."""
    x, e = _d(x), _d(eps).reshape(x.shape)
    st, row = _row(coefs, step, 4)
    xp, p0, A_x, A_p = _ddim_update(x, e, e.abs(), row, _table_row(noise, st, x))
    return StepResult(xp, p0, xp, {"x": A_x, "pred_x0": A_p, "xin": A_x})


def ddim_step_cfg(x, eps2, coefs, noise=None, step=None, scale=1.0):
    """upk_ddim_step_cfg_f32: the same with classifier-free guidance folded in (ddim.py:173-178)."""
    x = _d(x)
    e, Ae = _guided(eps2, x, scale)
    st, row = _row(coefs, step, 4)
    xp, p0, A_x, A_p = _ddim_update(x, e, Ae, row, _table_row(noise, st, x))
    return StepResult(xp, p0, xp, {"x": A_x, "pred_x0": A_p, "xin": A_x})


def plms_step(x, eps, coefs, step, hist, cfg_scale=1.0, cfg=False):
    """upk_plms_step_f32: model evaluation k = step of p_sample_plms (plms.py:218-236; S + 1 evaluations for S steps).

    k = 0 is plms.py:219-222 up to the second model call: e0 is remembered, the predictor x~ = update(x, e0, index 0)
    goes to xin only.  k = 1 finishes that step: e' = (e0 + eps) / 2 (plms.py:223), x <- update(x, e', index 0); the
    reference appends e0, not eps, to old_eps (plms.py:236 returns e_t), so the ring is not written.  k >= 2 is DDIM
    index j = k - 1 of the loop with len(old_eps) = min(j, 3) (plms.py:224-232), then old_eps gets eps.  The ring of
    include/upk.h keeps e_j in slot j % 3."""
    x = _d(x)
    k = int(step)
    H = _d(hist).reshape(3, *x.shape).clone()
    A_h = torch.zeros_like(H)
    if cfg:
        e, Ae = _guided(eps, x, cfg_scale)
    else:
        e = _d(eps).reshape(x.shape)
        Ae = e.abs()
    j = max(k - 1, 0)
    old = [H[(j - i) % 3] for i in (1, 2, 3)]  # old_eps[-1], [-2], [-3]
    slot = None
    if k == 0:
        ep, Aep, slot = e, Ae, 0
    elif k == 1:
        ep, Aep = (H[0] + e) / 2, (H[0].abs() + Ae) / 2
    elif j == 1:
        ep, Aep, slot = (3 * e - old[0]) / 2, (3 * Ae + old[0].abs()) / 2, j % 3
    elif j == 2:
        ep = (23 * e - 16 * old[0] + 5 * old[1]) / 12
        Aep, slot = (23 * Ae + 16 * old[0].abs() + 5 * old[1].abs()) / 12, j % 3
    else:
        ep = (55 * e - 59 * old[0] + 37 * old[1] - 9 * old[2]) / 24
        Aep, slot = (55 * Ae + 59 * old[0].abs() + 37 * old[1].abs() + 9 * old[2].abs()) / 24, j % 3
    _, row = _row(coefs, j, 4)
    xp, p0, A_x, A_p = _ddim_update(x, ep, Aep, row, None)
    if slot is not None:
        H[slot], A_h[slot] = e, Ae
    zero = torch.zeros_like(x)
    if k == 0:  # neither x nor pred_x0 is committed
        return StepResult(x, None, xp, {"x": zero, "pred_x0": zero, "xin": A_x, "hist": A_h}, H, False, slot)
    return StepResult(xp, p0, xp, {"x": A_x, "pred_x0": A_p, "xin": A_x, "hist": A_h}, H, True, slot)


def ddpm_step(x, model_out, coefs, noise=None, noise2=None, x0=None, mask=None, step=None, flags=0):
    """upk_ddpm_step_f32: p_sample (ddpm.py:1157-1185) on p_mean_variance (1125-1154) with q_posterior's mean, then the
    masked blend img_orig * mask + (1 - mask) * img with img_orig = q_sample(x0, t) (ddpm.py:1282-1283).  Row of
    include/upk.h: {sqrt(1/a_t), sqrt(1/a_t - 1), posterior_mean_coef1, posterior_mean_coef2,
    nonzero(t) exp(0.5 log var), sqrt(a_t), sqrt(1 - a_t), 0}."""
    x, m = _d(x), _d(model_out).reshape(x.shape)
    st, r = _row(coefs, step, 8)
    if flags & UPK_DDPM_X0:  # parameterization "x0" (ddpm.py:1139-1140)
        xr, A_r = m, m.abs()
    else:  # predict_start_from_noise (ddpm.py:1137-1138)
        xr, A_r = r[0] * x - r[1] * m, r[0].abs() * x.abs() + r[1].abs() * m.abs()
    if flags & UPK_DDPM_CLIP:  # ddpm.py:1144-1145 (the magnitude keeps the unclamped value: it bounds the error)
        xr = xr.clamp(-1.0, 1.0)
    xp = r[2] * xr + r[3] * x
    A_x = r[2].abs() * A_r + r[3].abs() * x.abs()
    nz = _table_row(noise, st, x)
    if nz is not None:
        xp, A_x = xp + r[4] * nz, A_x + r[4].abs() * nz.abs()
    if mask is not None:
        mk, z0 = _d(mask).reshape(x.shape), _d(x0).reshape(x.shape)
        q, A_q = r[5] * z0, r[5].abs() * z0.abs()
        n2 = _table_row(noise2, st, x)
        if n2 is not None:
            q, A_q = q + r[6] * n2, A_q + r[6].abs() * n2.abs()
        xp = q * mk + (1.0 - mk) * xp
        A_x = A_q * mk.abs() + (1.0 + mk.abs()) * A_x
    return StepResult(xp, xr, xp, {"x": A_x, "pred_x0": A_r, "xin": A_x})


# ---------------------------------------------------------------------------------------------------------------------
# the input sets and modes the host test (bound admits the reference / rejects the mutants) and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = ("ddim", "ddim_cfg", "plms", "ddpm")
SHAPES = [(1, 4, 1, 1), (2, 4, 6, 5), (3, 3, 7, 5), (8, 4, 32, 32), (4, 3, 128, 96)]  # 1, 1, 2 (ragged), 128, 576 workgroups
ROWS = 8       # rows of the single-launch coefficient / noise tables (PLMS evaluations 0 ... 6 use rows 0 ... 5)
CFG_SCALE = 3.0


def make_inputs(kernel, shape, rows=ROWS):
    """Seeded fp32 CPU operands of one kernel at one shape.  eps, the history and the noises have O(1) spread, |x| and
    |model_out| pass 1 on most elements (the clamp bites, and not everywhere), the mask holds 0, 1 and values strictly
    inside (0, 1), and every coefficient / noise row is distinct."""
    g = torch.Generator().manual_seed(1000 * KERNELS.index(kernel) + int(np.prod(shape)) + shape[0])
    rn = lambda *s: torch.randn(*s, generator=g)
    n = int(np.prod(shape))
    inp = {"x": 2.0 * rn(*shape), "noise": rn(rows, n), "shape": tuple(shape), "n": n, "rows": rows}
    if kernel == "ddpm":
        inp["eps"] = 2.0 * rn(*shape)
        inp["coefs"] = torch.rand(rows, 8, generator=g) + 0.3
        inp["coefs"][:, 7] = 0.0
        inp["noise2"], inp["x0"] = rn(rows, n), rn(n)
        i = torch.arange(n)
        inp["mask"] = torch.where(i % 3 == 0, torch.zeros(n), torch.where(i % 3 == 1, torch.ones(n),
                                                                          0.1 + 0.8 * torch.rand(n, generator=g)))
    else:
        inp["eps"] = rn(2 if kernel != "ddim" else 1, *shape)  # [uncond ; cond]; the plain paths read the first half
        inp["coefs"] = torch.rand(rows, 4, generator=g) + 0.3
        inp["noise"] = 0.5 * inp["noise"]  # sigma_t * randn
        if kernel == "plms":
            inp["hist"] = rn(3, n)
    return inp


def modes(kernel, rows=ROWS):
    """The single-launch modes of one kernel: dicts {noise, pred, xin: present?; step: None (NULL) or the row} plus
    {flags, mask: None / "noise2" / "plain"} for DDPM and {cfg} for PLMS (there `step` is the evaluation index k)."""
    full = dict(noise=True, pred=True, xin=True)
    common = [dict(full, step=s) for s in (None, 0, rows // 2, rows - 1)]
    common += [dict(full, step=rows // 2, **{k: False}) for k in ("noise", "pred", "xin")]
    if kernel in ("ddim", "ddim_cfg"):
        return common
    if kernel == "ddpm":
        out = [dict(full, step=1 + (f + i) % (rows - 1), flags=f, mask=mk)
               for f in range(4) for i, mk in enumerate((None, "noise2", "plain"))]
        return out + [dict(m, flags=UPK_DDPM_CLIP, mask="noise2") for m in common]
    out = [dict(full, noise=False, step=k, cfg=c) for k in range(7) for c in (False, True)]
    return out + [dict(full, noise=False, step=4, cfg=True, **{k: False}) for k in ("pred", "xin")]


def operands(kernel, inp, mode):
    """The tensor operands of one launch in the given mode (None = NULL), as keyword arguments of the oracle."""
    kw = {"x": inp["x"], "coefs": inp["coefs"], "step": mode["step"]}
    if kernel == "plms":
        kw.update(eps=inp["eps"] if mode["cfg"] else inp["eps"][0], hist=inp["hist"], cfg=mode["cfg"], cfg_scale=CFG_SCALE)
        return kw
    kw["noise"] = inp["noise"] if mode["noise"] else None
    if kernel == "ddim":
        kw["eps"] = inp["eps"][0]
    elif kernel == "ddim_cfg":
        kw.update(eps2=inp["eps"], scale=CFG_SCALE)
    else:
        mk = mode["mask"]
        kw.update(model_out=inp["eps"], flags=mode["flags"], x0=inp["x0"] if mk else None,
                  mask=inp["mask"] if mk else None, noise2=inp["noise2"] if mk == "noise2" else None)
    return kw


STEP_FNS = {"ddim": ddim_step, "ddim_cfg": ddim_step_cfg, "plms": plms_step, "ddpm": ddpm_step}


def run(kernel, inp, mode):
    return STEP_FNS[kernel](**operands(kernel, inp, mode))


# ---------------------------------------------------------------------------------------------------------------------
# chains with a synthetic denoiser (no UNet): the cases, and the tolerance measured on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_SHAPES = [(8, 4, 32, 32), (3, 3, 7, 5)]
DDIM_CHAINS = [(50, 0.0), (50, 1.0), (10, 1.0)]  # (S, eta)
PLMS_CHAINS = [1, 2, 4, 5, 10, 50]               # S (must divide 1000: the uniform schedule, as in the reference)
CHAIN_SCALE = 3.0
# Largest deviation, relative to max |z|, between oracle.ddim's samplers run in fp32 and in fp64 on eps_fn below (both
# reading the fp16-rounded latent) over chain_cases(): 1.593e-03 (PLMS, S = 50, guided, 8x4x32x32), printed by
# `python -m oracle.steps`.  It is dominated by fp16 rounding flips of the stem input (2^-11 |x| times the Lipschitz
# constant of eps_fn, amplified by 1 / sqrt(a_t) in pred_x0), not by fp32 arithmetic.  The GPU chains assert four times
# that: the factor covers a second independent fp32 evaluation order.
CHAIN_MEASURED = 1.593e-3
CHAIN_TOL = 4.0 * CHAIN_MEASURED


def alphas_cumprod():
    from .schedule import ddpm_tables, linear_betas
    return ddpm_tables(linear_betas())["alphas_cumprod"]


def eps_fn(x, t, cond):
    """A smooth bounded denoiser (Lipschitz constant about 1.1) that reads the latent as the UNet does: rounded to
    fp16 (the stem input).  Evaluated in x's dtype."""
    xr = x.half().to(x.dtype)
    tt = t.to(x.dtype).reshape(-1, *([1] * (x.dim() - 1)))
    return 0.8 * torch.sin(1.3 * xr + 0.013 * tt) + 0.1 * torch.cos(0.7 * xr - 0.013 * tt) + cond.to(x.dtype)


def kernel_tables(S, eta):
    """What the samplers hand the kernels for an S-step uniform schedule: (descending timesteps [S], the
    upgpt_amd.schedule.ddim_coefficient_table rows in loop order [S, 4] fp32, fp32 sigmas in loop order [S])."""
    from upgpt_amd import schedule
    acp = torch.as_tensor(alphas_cumprod())
    ts = schedule.make_ddim_timesteps("uniform", S, 1000, verbose=False)
    sig, a, ap = schedule.make_ddim_sampling_parameters(acp, ts, eta, verbose=False)
    order = np.arange(S)[::-1].copy()
    coefs = schedule.ddim_coefficient_table(a, ap, sig, torch.sqrt(1.0 - a), order)
    return np.flip(ts).copy(), coefs, sig.float()[torch.as_tensor(order)]


def chain_inputs(shape, S):
    g = torch.Generator().manual_seed(77 + shape[0] + S)
    x_T = torch.randn(*shape, generator=g)
    cond, uncond = 0.1 * torch.randn(*shape, generator=g), 0.1 * torch.randn(*shape, generator=g)
    noise = torch.randn(S, *shape, generator=g)
    return x_T, cond, uncond, noise


def ddim_chain_oracle(shape, S, eta, guided, dtype):
    """oracle.ddim.ddim_sample on the synthetic denoiser, every step logged.  -> (x_0, [x per step], [pred_x0 per step])"""
    from .ddim import ddim_sample
    x_T, cond, uncond, noise = (t.to(dtype) for t in chain_inputs(shape, S))
    z, inter = ddim_sample(eps_fn, alphas_cumprod(), shape, S, eta, x_T, noise=noise if eta > 0 else None, cond=cond,
                           uncond=uncond if guided else None, guidance_scale=CHAIN_SCALE if guided else 1.0, log_every_t=1)
    return z, inter["x_inter"][1:], inter["pred_x0"][1:]


def plms_chain_oracle(shape, S, guided, dtype):
    """oracle.ddim.plms_sample likewise; guidance (plms.py:182-186) is folded into the eps_fn it is given."""
    from .ddim import plms_sample
    x_T, cond, uncond, _ = (t.to(dtype) for t in chain_inputs(shape, S))

    def fn(x, t, c):
        if not guided:
            return eps_fn(x, t, c)
        e_u = eps_fn(x, t, uncond)
        return e_u + CHAIN_SCALE * (eps_fn(x, t, c) - e_u)

    z, inter = plms_sample(fn, alphas_cumprod(), shape, S, x_T, cond=cond, log_every_t=1)
    return z, inter["x_inter"][1:], inter["pred_x0"][1:]


def chain_cases():
    for shape in CHAIN_SHAPES:
        for guided in (False, True):
            for S, eta in DDIM_CHAINS:
                yield ("ddim", shape, S, eta, guided)
            for S in PLMS_CHAINS:
                yield ("plms", shape, S, 0.0, guided)


def chain_oracle(case, dtype):
    kind, shape, S, eta, guided = case
    if kind == "ddim":
        return ddim_chain_oracle(shape, S, eta, guided, dtype)
    return plms_chain_oracle(shape, S, guided, dtype)


def chain_deviation(got, ref):
    """Largest deviation of the final latent and of every logged x / pred_x0, relative to max |z| of the fp64 run."""
    zmax = float(ref[0].abs().max())
    dev = float((_d(got[0]) - ref[0]).abs().max())
    for a, b in zip(list(got[1]) + list(got[2]), list(ref[1]) + list(ref[2])):
        dev = max(dev, float((_d(a) - b).abs().max()))
    return dev / zmax


def measure_chain_tolerance(verbose=False):
    """The reference against itself: fp32 vs fp64 oracle runs (both reading the fp16-rounded latent), all chain cases."""
    worst = 0.0
    for case in chain_cases():
        d = chain_deviation(chain_oracle(case, torch.float32), chain_oracle(case, torch.float64))
        if verbose:
            print("%-5s %-16s S=%-3d eta=%.0f guided=%d  %.3e" % (case[0], case[1], case[2], case[3], case[4], d))
        worst = max(worst, d)
    return worst


if __name__ == "__main__":
    print("largest fp32-vs-fp64 oracle deviation / max|z| over the chain cases: %.3e" % measure_chain_tolerance(True))
