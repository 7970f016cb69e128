"""fp64 numpy restatement of SDE-DPM-Solver++(2M) as this package runs it (include/upk.h upk_dpmpp_2m_sde_step_f32,
upgpt_amd/schedule.py dpm_sde_coefficient_table, upgpt_amd/dpm_sde.py): the update in the formula's form (which never
sees a coefficient row), the table, ONE launch of the step kernel (guidance, noise, mask, x_plain and the fp16 stem input
included), a chain over the table with given normals and keep rows, and the exact covariance recursion of the chain on a
Gaussian model.  Written from Lu et al. 2022 (arXiv:2211.01095; the sde-dpmsolver++ multistep form with the noise level
eta), not from the code under test; the schedule helpers are dpm_ref's.

The solver.  Points are numbered in loop order, lambda = log(alpha / sigma) ascends, a step s -> t has h = lambda_t -
lambda_s > 0 and m = (x - sigma_s e) / alpha_s:

    x_t = (sigma_t / sigma_s) exp(-eta h) x_s - alpha_t expm1(-(1 + eta) h) D + sigma_t sqrt(-expm1(-2 eta h)) z
    D = m_s (first order),  D = m_s + h / (2 h_prev) (m_s - m_{s-1}) (second order)

The bound of one launch, by dpm_ref's rule (magnitudes A: the same expression with absolute values and additions; each
rounding adds at most 2^-24 relative to an intermediate bounded by A).  The longest path is guided, second-order, with
noise and blend:
    3 roundings for e_u + s (e_c - e_u), 3 for (x - r0 e) r1, 3 for m + r4 (m - m_old), 3 for r2 x + r3 d, 1 for + noise,
    4 for mask * keep + (1 - mask) * xn  (the difference, two products, the sum):  17.
So a correct fp32 kernel satisfies |got - ref64| <= BOUND * A elementwise with BOUND = N * 2^-24, N = 40: more than double
the count (second-order terms; FMA contraction only removes roundings), fixed before any device run.  The coefficient rows
and the noise table are the SAME fp32 numbers on both sides.  xin is the fp16 rounding of the x the kernel wrote: checked
bit for bit against that x.
"""
import numpy as np

from dpm_ref import linear_alphas_cumprod, logsnr_nodes, tables, uniform_timesteps, within as _within  # noqa: F401

N_ROUNDINGS = 17
N = 40
BOUND = N * 2.0 ** -24


def within(got, ref, A, bound=BOUND):
    return _within(got, ref, A, bound)


# ------------------------------------------------------------------------------------------------------- formula form
def points(a_t, a_prev):
    """(alpha, sigma, lambda) of the S + 1 points of a chain in loop order from the DDIM tables (ascending index)."""
    a = np.concatenate([np.asarray(a_t, np.float64)[::-1], np.asarray(a_prev, np.float64)[:1]])
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    return al, sg, np.log(al / sg)


def formula_step(x, m, m_prev, al_s, sg_s, al_t, sg_t, h, h_prev, eta, z):
    """One step in the formula's form.  m_prev None: first order."""
    D = m if m_prev is None else m + h / (2.0 * h_prev) * (m - m_prev)
    return (sg_t / sg_s) * np.exp(-eta * h) * x - al_t * np.expm1(-(1.0 + eta) * h) * D + \
        sg_t * np.sqrt(-np.expm1(-2.0 * eta * h)) * z


def row_order(i, S, order, lower_order_final, start):
    if lower_order_final is None:
        lower_order_final = S < 15
    return 1 if (lower_order_final and i == S - 1) else min(order, i + 1 - start)


def formula_chain(model, x_T, a_t, a_prev, timesteps, eta, normals, order=2, lower_order_final=None, start=0):
    """The chain from the formulas alone.  model(x, t, i) -> eps; timesteps DESCENDING, one per loop position; normals[i]:
    the standard normals of loop position i.  Returns (x, [x after each step])."""
    al, sg, lam = points(a_t, a_prev)
    S = len(al) - 1
    x, m_prev, xs = np.asarray(x_T, np.float64), None, []
    for i in range(start, S):
        m = (x - sg[i] * model(x, int(timesteps[i]), i)) / al[i]
        second = row_order(i, S, order, lower_order_final, start) == 2
        h, h_prev = lam[i + 1] - lam[i], (lam[i] - lam[i - 1] if i > 0 else None)
        x = formula_step(x, m, m_prev if second else None, al[i], sg[i], al[i + 1], sg[i + 1], h, h_prev, eta,
                         np.asarray(normals[i], np.float64))
        m_prev = m
        xs.append(x)
    return x, xs


# -------------------------------------------------------------------------------------------------------------- table
def coefficient_table(a_t, a_prev, eta=1.0, order=2, lower_order_final=None, start=0):
    """fp64 [S - start, 8] rows in loop order: {sigma_s, 1/alpha_s, (sigma_t/sigma_s) exp(-eta h), -alpha_t expm1(-(1 + eta) h),
    w, sigma_t sqrt(-expm1(-2 eta h)), 0, 0}."""
    al, sg, lam = points(a_t, a_prev)
    S = len(al) - 1
    rows = np.zeros((S - start, 8))
    for i in range(start, S):
        h = lam[i + 1] - lam[i]
        w = h / (2.0 * (lam[i] - lam[i - 1])) if row_order(i, S, order, lower_order_final, start) == 2 else 0.0
        rows[i - start, :6] = (sg[i], 1.0 / al[i], sg[i + 1] / sg[i] * np.exp(-eta * h),
                               -al[i + 1] * np.expm1(-(1.0 + eta) * h), w, sg[i + 1] * np.sqrt(-np.expm1(-2.0 * eta * h)))
    return rows


# ---------------------------------------------------------------------------------------------------------- one launch
class Step:
    """Everything one launch may write, float64: x (after the blend), x_plain (before it), m (= pred_x0 = the new m_old), xin
    (x before its fp16 rounding), the magnitudes A["x"], A["x_plain"], A["m"], and what the row did."""

    def __init__(self, x, x_plain, m, A, second, blended):
        self.x, self.x_plain, self.m, self.xin, self.A, self.second, self.blended = x, x_plain, m, x, A, second, blended


def step(x, eps, coefs, step=None, m_old=None, noise=None, keep=None, mask=None, n_rows=0, cfg_scale=1.0, cfg=False):
    """x: [B, C, H, W]; eps: the same, or with cfg [2, B, C, H, W]; coefs: [rows, 8] (the fp32 table widened); step: the row
    (None: row 0); m_old is looked at only where the row's w is non-zero; noise: [rows, n] already scaled, or None; keep:
    [n_rows, n], mask: [n] (expanded to the latent), or None."""
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
    m = (x - c[0] * e) * c[1]
    A_m = (np.abs(x) + abs(c[0]) * Ae) * abs(c[1])
    second = bool(c[4] != 0)
    if second:
        old = np.asarray(m_old, dtype=np.float64).reshape(x.shape)
        d, A_d = m + c[4] * (m - old), A_m + abs(c[4]) * (A_m + np.abs(old))
    else:
        d, A_d = m, A_m
    xn = c[2] * x + c[3] * d
    A_x = abs(c[2]) * np.abs(x) + abs(c[3]) * A_d
    if noise is not None:
        nz = np.asarray(noise, dtype=np.float64).reshape(-1, x.size)[st].reshape(x.shape)
        xn, A_x = xn + nz, A_x + np.abs(nz)
    plain, A_plain = xn, A_x
    blended = mask is not None and st + 1 < n_rows
    if blended:
        mk = np.asarray(mask, dtype=np.float64).reshape(x.shape)
        kp = np.asarray(keep, dtype=np.float64).reshape(-1, x.size)[st + 1].reshape(x.shape)
        xn = mk * kp + (1.0 - mk) * xn
        A_x = np.abs(mk) * np.abs(kp) + (1.0 + np.abs(mk)) * A_x
    return Step(xn, plain, m, {"x": A_x, "x_plain": A_plain, "m": A_m}, second, blended)


# --------------------------------------------------------------------------------------------------------------- chain
def chain(model, x_T, timesteps, table, start=0, normals=None, temperature=1.0, keep=None, mask=None):
    """The sampler's loop in fp64 over `table` ([S - start, 8], any float dtype: row i - start is loop position i).
    model(x, t, i) -> eps (guided: already combined); timesteps DESCENDING, one per loop position; normals[i]: the standard
    normals of loop position i (scaled here by the row's r5 * temperature; for an fp32 table the product is rounded to fp32,
    as the sampler's noise scale is); keep[i] / mask: the blend in front of every evaluation (mask = 1 keeps).
    Returns (x, [unblended x after each step], [m of each step])."""
    x = np.asarray(x_T, dtype=np.float64)
    fp32 = np.asarray(table).dtype == np.float32
    tab = np.asarray(table, dtype=np.float64)
    S = start + tab.shape[0]
    mk = None if mask is None else np.broadcast_to(np.asarray(mask, np.float64), x.shape)
    old, xs, ms = None, [], []
    for i in range(start, S):
        if mk is not None:
            x = mk * np.asarray(keep[i], np.float64).reshape(x.shape) + (1.0 - mk) * x
        nz = None
        if tab[i - start, 5] != 0:
            scale = tab[i - start, 5] * temperature
            if fp32:
                scale = float(np.float32(np.float32(tab[i - start, 5]) * np.float32(temperature)))
            nz = (scale * np.asarray(normals[i], np.float64)).reshape(1, -1)
        r = step(x, model(x, int(timesteps[i]), i), tab[i - start], None, old, nz)
        x, old = r.x, r.m
        xs.append(x)
        ms.append(r.m)
    return x, xs, ms


# ------------------------------------------------------------------------------------------------------ Gaussian model
def gaussian_data(acp, s2):
    """Data x0 ~ N(0, s2): the exact data prediction is m(x, t) = g_t x, g = alpha s2 / (alpha^2 s2 + sigma^2)."""
    def g(t):
        a = acp[t]
        return np.sqrt(a) * s2 / (a * s2 + 1.0 - a)
    return g


def gaussian_variance_error(acp, s2, S, eta, order=2, lower_order_final=None):
    """|Var(x_final) / (alpha^2 s2 + sigma^2) - 1| of the chain on the logSNR grid, started from the exact marginal variance
    at its first point.  The chain is linear, so the covariance P of the state (x, m_old) is propagated exactly:
    P <- M P M^T, P[0, 0] += r5^2, M = [[kx + kd (1 + w) g, -kd w], [g, 0]]."""
    ts = logsnr_nodes(acp, S)[1:]
    tab = coefficient_table(*tables(acp, ts), eta=eta, order=order, lower_order_final=lower_order_final)
    g, desc = gaussian_data(acp, s2), ts[::-1]
    v = lambda a: a * s2 + 1.0 - a
    P = np.array([[v(acp[desc[0]]), 0.0], [0.0, 0.0]])
    for i in range(S):
        kx, kd, w, r5, gi = tab[i, 2], tab[i, 3], tab[i, 4], tab[i, 5], g(desc[i])
        M = np.array([[kx + kd * (1.0 + w) * gi, -kd * w], [gi, 0.0]])
        P = M @ P @ M.T
        P[0, 0] += r5 * r5
    return float(abs(P[0, 0] / v(acp[0]) - 1.0))


def ddim_variance_error(acp, s2, S, eta=1.0):
    """The same figure for DDIM (ddim.py:189-203) on the reference's uniform grid; one scalar of state."""
    ts = uniform_timesteps(S, acp.shape[0])
    a_t, a_p = tables(acp, ts)
    v = lambda a: a * s2 + 1.0 - a
    var = v(a_t[-1])
    for j in range(len(ts) - 1, -1, -1):
        sig = eta * np.sqrt((1.0 - a_p[j]) / (1.0 - a_t[j]) * (1.0 - a_t[j] / a_p[j]))
        ke = np.sqrt(1.0 - a_t[j]) / v(a_t[j])  # e = ke x
        kp = (1.0 - np.sqrt(1.0 - a_t[j]) * ke) / np.sqrt(a_t[j])  # pred_x0 = kp x
        c = np.sqrt(a_p[j]) * kp + np.sqrt(1.0 - a_p[j] - sig * sig) * ke
        var = c * c * var + sig * sig
    return float(abs(var / v(acp[0]) - 1.0))
