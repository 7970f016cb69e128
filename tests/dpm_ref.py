"""fp64 numpy restatement of DPM-Solver++(2M) as this package runs it (include/upk.h upk_dpmpp_2m_step_f32,
upgpt_amd/schedule.py make_logsnr_timesteps / dpm_coefficient_table, upgpt_amd/dpm_solver.py): the step grid, the
coefficient table, ONE launch of the step kernel (guidance and the fp16 stem input included) and a whole chain.  Written
from Lu et al. 2022 (arXiv:2211.01095), algorithm 2, not from the code under test; the analytic Gaussian model at the end
(test_dpm_host.py) validates this restatement itself, since the modelled project has no DPM solver to compare with.

The solver.  With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), a step t -> p of size
h = lambda_p - lambda_t > 0 on the data prediction x0 = (x - sigma_t eps) / alpha_t is

    x_p = (sigma_p / sigma_t) x_t - alpha_p (exp(-h) - 1) D,    D = x0_t + (x0_t - x0_prev) / (2 r),   r = h_prev / h

(second order), or D = x0_t (first order: algebraically the DDIM eta = 0 update, since
sigma_p / sigma_t * alpha_t + alpha_p (1 - exp(-h)) = alpha_p ... see first_order_is_ddim below).

The bound of one launch, in the form oracle/steps.py uses: next to each output the reference carries its magnitude A —
the same expression with every coefficient and operand replaced by its absolute value and every subtraction by an
addition.  Every intermediate of an fp32 evaluation, in whatever association order, is bounded by A up to second order,
and each rounding adds at most 2^-24 relative to such an intermediate.  The longest path of this kernel: 3 roundings for
e_u + s (e_c - e_u), 3 for (x - c0 e) c1, 3 for p0 + w (p0 - x0_old), 3 for c2 x + c3 D: 12.  So a correct fp32 kernel
satisfies

    |got - ref64| <= BOUND * A  elementwise,   BOUND = 32 * 2^-24,

32 being more than double the count (second-order terms; FMA contraction only removes roundings).  The coefficient rows
are the SAME fp32 numbers on both sides (the reference widens the table the kernel reads), so the table's own rounding is
not part of the bound; test_dpm_host.py checks the table against fp64 separately.  xin is the fp16 rounding of the x the
kernel wrote: checked bit for bit against that x, and against the reference within BOUND * A + 2^-11 |ref| + 2^-25.
"""
import numpy as np

BOUND = 32.0 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ schedule
def linear_alphas_cumprod(T=1000, linear_start=0.00085, linear_end=0.012, fp32=True):
    """The configs' schedule (ddpm.py:125-146): betas = linspace(sqrt(start), sqrt(end), T)^2 in fp64; the model keeps
    the cumulative product in fp32 (fp32=True: widened back, as the samplers read it)."""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, T, dtype=np.float64) ** 2
    acp = np.cumprod(1.0 - betas)
    return acp.astype(np.float32).astype(np.float64) if fp32 else acp


def logsnr_nodes(acp, S):
    """S + 1 integer timesteps from 0 to T - 1, nearest to a uniform grid in lambda, strictly increasing."""
    acp = np.asarray(acp, dtype=np.float64)
    T = acp.shape[0]
    if S < 1:
        raise ValueError("S < 1")
    lam = 0.5 * np.log(acp / (1.0 - acp))
    node = []
    for k in range(S + 1):
        g = lam[0] + (lam[T - 1] - lam[0]) * k / S
        t = int(np.argmin(np.abs(lam - g)))  # the first minimiser
        if node:
            t = max(t, node[-1] + 1)
        node.append(t)
    if node[-1] > T - 1:
        raise ValueError("the nodes leave [0, T - 1]")
    return np.asarray(node, dtype=np.int64)


def uniform_timesteps(S, T=1000):
    """The reference's `uniform` DDIM grid (util.py:46-57)."""
    return np.arange(0, T, T // S) + 1


def tables(acp, timesteps):
    """(a_t, a_prev) per DDIM index (ascending t) for the chain over `timesteps`: the last target is acp[0]."""
    acp = np.asarray(acp, dtype=np.float64)
    ts = np.asarray(timesteps)
    return acp[ts], np.concatenate([acp[:1], acp[ts[:-1]]])


def coefficient_table(a_t, a_prev, order=2, lower_order_final=None):
    """fp64 [S, 8] rows in LOOP order (descending t): {sigma_t, 1/alpha_t, sigma_p/sigma_t, -alpha_p expm1(-h), w, 0, 0, 0}."""
    a_t, a_p = np.asarray(a_t, np.float64)[::-1], np.asarray(a_prev, np.float64)[::-1]
    S = a_t.shape[0]
    if lower_order_final is None:
        lower_order_final = S < 15
    rows = np.zeros((S, 8))
    h_prev = None
    for i in range(S):
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t[i]), np.sqrt(1 - a_t[i]), np.sqrt(a_p[i]), np.sqrt(1 - a_p[i])
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        first = i == 0 or order == 1 or (lower_order_final and i == S - 1)
        w = 0.0 if first else 1.0 / (2.0 * (h_prev / h))
        rows[i, :5] = sg_t, 1.0 / al_t, sg_p / sg_t, -al_p * np.expm1(-h), w
        h_prev = h
    return rows


# ---------------------------------------------------------------------------------------------------------- one launch
class Step:
    """Everything one launch may write, float64: x, p0 (= pred_x0 = the new x0_old), xin (x before its fp16 rounding),
    the magnitudes A["x"], A["p0"], and whether the row ran second-order."""

    def __init__(self, x, p0, A, second):
        self.x, self.p0, self.xin, self.A, self.second = x, p0, x, A, second


def step(x, eps, coefs, step=None, x0_old=None, first_row=0, cfg_scale=1.0, cfg=False):
    """x: [B, C, H, W]; eps: the same, or with cfg [2, B, C, H, W] = [uncond ; cond]; coefs: [rows, 8] (the fp32 table
    widened); step: the row (None: row 0); x0_old is looked at only when the row is second-order and not first_row."""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(eps, dtype=np.float64)
    if cfg:
        e = e.reshape(2, *x.shape)
        s = float(np.float32(cfg_scale))
        e, Ae = e[0] + s * (e[1] - e[0]), np.abs(e[0]) + abs(s) * (np.abs(e[1]) + np.abs(e[0]))
    else:
        e = e.reshape(x.shape)
        Ae = np.abs(e)
    st = 0 if step is None else int(step)
    c = np.asarray(coefs, dtype=np.float64).reshape(-1, 8)[st]
    p0 = (x - c[0] * e) * c[1]
    A_p = (np.abs(x) + abs(c[0]) * Ae) * abs(c[1])
    second = bool(c[4] != 0 and st != first_row)
    if second:
        old = np.asarray(x0_old, dtype=np.float64).reshape(x.shape)
        D = p0 + c[4] * (p0 - old)
        A_D = A_p + abs(c[4]) * (A_p + np.abs(old))
    else:
        D, A_D = p0, A_p
    xn = c[2] * x + c[3] * D
    A_x = abs(c[2]) * np.abs(x) + abs(c[3]) * A_D
    return Step(xn, p0, {"x": A_x, "p0": A_p}, second)


def within(got, ref, A, bound=BOUND):
    return np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref) <= bound * A


# --------------------------------------------------------------------------------------------------------------- chain
def chain(model, x_T, timesteps, table, start=0, blend=None):
    """The sampler's loop in fp64.  model(x, t, i) -> eps (or, guided, the already combined eps) for the integer timestep
    t of loop position i; timesteps: DESCENDING, one per row of `table` ([S, 8], any float dtype); the chain runs rows
    start .. S - 1 and its first row is first-order.  blend(x, t, i) -> x: the masked chains' q_sample blend in front of
    every evaluation.  Returns (x, [x after each step], [p0 of each step])."""
    x = np.asarray(x_T, dtype=np.float64)
    tab = np.asarray(table, dtype=np.float64)
    old, xs, ps = None, [], []
    for i in range(start, tab.shape[0]):
        t = int(timesteps[i])
        if blend is not None:
            x = blend(x, t, i)
        r = step(x, model(x, t, i), tab, i, old, first_row=start)
        x, old = r.x, r.p0
        xs.append(x)
        ps.append(r.p0)
    return x, xs, ps


def ddim_chain(model, x_T, acp, timesteps):
    """DDIM at eta = 0 (ddim.py:189-203) over ascending `timesteps`, fp64: the yardstick of the analytic test."""
    a_t, a_p = tables(acp, timesteps)
    x = np.asarray(x_T, dtype=np.float64)
    for j in range(len(timesteps) - 1, -1, -1):
        e = model(x, int(timesteps[j]), len(timesteps) - 1 - j)
        p0 = (x - np.sqrt(1 - a_t[j]) * e) / np.sqrt(a_t[j])
        x = np.sqrt(a_p[j]) * p0 + np.sqrt(1 - a_p[j]) * e
    return x


# ------------------------------------------------------------------------------------------------------ analytic model
def gaussian_eps(acp, s2):
    """Data x0 ~ N(0, s2): x_t ~ N(0, v_t), v = a s2 + 1 - a, and the exact noise prediction is
    E[eps | x_t] = sigma_t x_t / v_t."""
    def model(x, t, i):
        a = acp[t]
        return np.sqrt(1 - a) * x / (a * s2 + 1 - a)
    return model


def gaussian_exact(acp, s2, t_start, x_start):
    """The probability-flow ODE's solution from t_start down to the chain's last target acp[0]: x scales with sqrt(v)."""
    v = lambda a: a * s2 + 1 - a
    return x_start * np.sqrt(v(acp[0]) / v(acp[t_start]))


def gaussian_error(acp, s2, solver, grid, S, order=2):
    """Relative error of the final latent of `solver` ("2m" / "ddim") on `grid` ("logsnr" / "uniform") with S steps."""
    ts = logsnr_nodes(acp, S)[1:] if grid == "logsnr" else uniform_timesteps(S, acp.shape[0])
    model, x_T = gaussian_eps(acp, s2), np.asarray([1.0])
    if solver == "ddim":
        x = ddim_chain(model, x_T, acp, ts)
    else:
        x = chain(model, x_T, ts[::-1], coefficient_table(*tables(acp, ts), order=order))[0]
    exact = gaussian_exact(acp, s2, int(ts[-1]), x_T)
    return float(np.abs(x - exact)[0] / np.abs(exact)[0])
