"""fp64 numpy restatement of UniPC as this package runs it (include/upk.h upk_unipc_step_f32, upgpt_amd/schedule.py
unipc_coefficient_table, upgpt_amd/unipc.py): the solver in the paper's own form (paper_chain), the coefficient table, ONE
launch of the step kernel (guidance and the fp16 stem input included), a chain over the table, and the error on the analytic
Gaussian model of tests/dpm_ref.py.  Written from Zhao et al. 2023 (arXiv:2302.04867), not from the code under test:
paper_chain never sees a coefficient row, and test_unipc_host.py holds the table-driven chain against it.

The solver (multistep, data prediction m = (x - sigma e) / alpha, lambda = log(alpha / sigma)).  Points k = 0 .. S along the
chain, lambda ascending.  For a step from point s to point t of size h = lambda_t - lambda_s with the history nodes
r_i = (lambda_{s-i} - lambda_s) / h < 0 and D_i = (m_{s-i} - m_s) / r_i, i = 1 .. p - 1:

    UniP-p:   x_t = (sigma_t / sigma_s) x_s - alpha_t expm1(-h) m_s - alpha_t B(h) sum_{i<p} rho_i D_i
    UniC-p:   x_t = (sigma_t / sigma_s) x_s - alpha_t expm1(-h) m_s - alpha_t B(h) (sum_{i<p} rho_i D_i + rho_p (m_t - m_s))

B(h) = expm1(-h) (bh2) or -h (bh1).  rho solves R rho = b, R[n][i] = r_i^n (r_p = 1 for the corrector's own node), b[n] =
(n + 1)! z phi_{n+2}(z) / B(h), z = -h, with phi_1(z) = expm1(z) / z, phi_{k+1}(z) = (phi_k(z) - 1 / k!) / z, n = 0 .. p - 1
(the recurrence below carries z phi_k: it starts from expm1(z) / z - 1 = z phi_2); the predictor takes the system
without its last row and column; rho = [0.5] for UniP-2 and UniC-1 (the paper's closed forms).  x_s of the corrector is the
last CORRECTED latent, m_t the model's prediction at the PREDICTED x_t — the evaluation the next step needs anyway.  The order
of the step k -> k+1 is min(order, k + 1 - start, S - k); the corrector at point k runs at the order of the predictor that led
there; the final latent is the last prediction.

The bound of one launch, by dpm_ref's rule: next to each output the reference carries its magnitude A (every coefficient
and operand replaced by its absolute value, every subtraction by an addition); each fp32 rounding adds at most 2^-24
relative to an intermediate bounded by A.  Roundings on the full path (guided, corrector order 3, predictor order 3):
e_u + s (e_c - e_u): 3;  (x - r0 e) r1: 3;  r2 x_corr: 1, + r3 h0: 2, + r4 (m - h0): 3, + r5 (h1 - h0): 3, + r6 (h2 - h0): 3
(the corrected latent: 12);  r7 xc: 1, + r8 m: 2, + r9 (h0 - m): 3, + r10 (h1 - m): 3 (the prediction: 9).  27 in all, so

    |got - ref64| <= BOUND * A  elementwise,   BOUND = 64 * 2^-24,

64 being the power of two above double the count (second-order terms; FMA contraction only removes roundings).  The rows
are the SAME fp32 numbers on both sides; test_unipc_host.py checks the table against fp64 separately.  xin is the fp16
rounding of the x the kernel wrote: bit for bit against that x, and against the reference within BOUND * A + 2^-11 |ref| +
2^-25.
"""
import math

import numpy as np

import dpm_ref as D

BOUND = 64.0 * 2.0 ** -24

linear_alphas_cumprod, logsnr_nodes, tables = D.linear_alphas_cumprod, D.logsnr_nodes, D.tables
gaussian_eps, gaussian_exact = D.gaussian_eps, D.gaussian_exact


# ---------------------------------------------------------------------------------------------------------- the paper
def _B(h, variant):
    if variant not in ("bh1", "bh2"):
        raise ValueError(variant)
    return math.expm1(-h) if variant == "bh2" else -h


def rho(nodes, h, variant):
    """R rho = b for the nodes r (fp64); see the module docstring."""
    n, z = len(nodes), -h
    phi, b = math.expm1(z) / z - 1.0, []
    for i in range(1, n + 1):
        b.append(phi * math.factorial(i) / _B(h, variant))
        phi = phi / z - 1.0 / math.factorial(i + 1)
    R = np.vander(np.asarray(nodes, dtype=np.float64), n, increasing=True).T
    return np.linalg.solve(R, np.asarray(b))


def _points(a_t, a_prev):
    """alpha, sigma, lambda of the points 0 .. S in loop order from the DDIM tables (ascending index)."""
    a = np.concatenate([np.asarray(a_t, np.float64)[::-1], np.asarray(a_prev, np.float64)[:1]])
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    return al, sg, np.log(al / sg)


def _order(k, order, S, start, lower_order_final):
    return min(order, k + 1 - start, S - k) if lower_order_final else min(order, k + 1 - start)


def paper_chain(model, x_T, a_t, a_prev, timesteps, order=2, variant="bh2", lower_order_final=True, corrector=True, start=0):
    """UniPC as the paper states it, no coefficient rows: model(x, t, i) -> eps; timesteps DESCENDING, one per point
    0 .. S - 1.  Returns (the final latent, [predicted latent after each evaluation], [m of each evaluation])."""
    al, sg, lam = _points(a_t, a_prev)
    S = len(al) - 1
    x = np.asarray(x_T, dtype=np.float64)
    ms, xs = {}, []
    x_corr = None
    for k in range(start, S):
        m = (x - sg[k] * model(x, int(timesteps[k]), k)) / al[k]
        ms[k] = m
        if corrector and k > start:
            s, p = k - 1, _order(k - 1, order, S, start, lower_order_final)
            h = lam[k] - lam[s]
            r = [(lam[s - i] - lam[s]) / h for i in range(1, p)]
            Ds = [(ms[s - i] - ms[s]) / r[i - 1] for i in range(1, p)]
            w = np.asarray([0.5]) if p == 1 else rho(r + [1.0], h, variant)
            res = sum(w[i] * Ds[i] for i in range(p - 1)) + w[-1] * (m - ms[s])
            xc = sg[k] / sg[s] * x_corr - al[k] * math.expm1(-h) * ms[s] - al[k] * _B(h, variant) * res
        else:
            xc = x
        p = _order(k, order, S, start, lower_order_final)
        h = lam[k + 1] - lam[k]
        r = [(lam[k - i] - lam[k]) / h for i in range(1, p)]
        Ds = [(ms[k - i] - m) / r[i - 1] for i in range(1, p)]
        w = [] if p == 1 else np.asarray([0.5]) if p == 2 else rho(r, h, variant)
        res = sum(w[i] * Ds[i] for i in range(p - 1)) if p > 1 else 0.0
        x = sg[k + 1] / sg[k] * xc - al[k + 1] * math.expm1(-h) * m - al[k + 1] * _B(h, variant) * res
        x_corr = xc
        xs.append(x)
    return x, xs, [ms[k] for k in range(start, S)]


# ----------------------------------------------------------------------------------------------------------- the table
def coefficient_table(a_t, a_prev, order=2, variant="bh2", lower_order_final=True, corrector=True, start=0):
    """fp64 [S - start, 12] rows in loop order: the paper's two updates with rho / r folded into one weight per difference."""
    if order not in (1, 2, 3):
        raise ValueError(order)
    al, sg, lam = _points(a_t, a_prev)
    S = len(al) - 1
    rows = np.zeros((S - start, 12))
    for k in range(start, S):
        row = rows[k - start]
        row[0], row[1] = sg[k], 1.0 / al[k]
        p = _order(k, order, S, start, lower_order_final)
        h = lam[k + 1] - lam[k]
        row[7], row[8] = sg[k + 1] / sg[k], -al[k + 1] * math.expm1(-h)
        r = [(lam[k - i] - lam[k]) / h for i in range(1, p)]
        w = [] if p == 1 else [0.5] if p == 2 else rho(r, h, variant)
        for i in range(p - 1):
            row[9 + i] = -al[k + 1] * _B(h, variant) * w[i] / r[i]
        if corrector and k > start:
            s, q = k - 1, _order(k - 1, order, S, start, lower_order_final)
            h = lam[k] - lam[s]
            r = [(lam[s - i] - lam[s]) / h for i in range(1, q)]
            w = [0.5] if q == 1 else rho(r + [1.0], h, variant)
            row[2], row[3], row[4], row[11] = sg[k] / sg[s], -al[k] * math.expm1(-h), -al[k] * _B(h, variant) * w[-1], 1.0
            for i in range(q - 1):
                row[5 + i] = -al[k] * _B(h, variant) * w[i] / r[i]
    return rows


# ---------------------------------------------------------------------------------------------------------- one launch
class Step:
    """Everything one launch may write, float64: x (the prediction; xin before its fp16 rounding), xc (the new x_corr), m
    (= pred_x0 = the ring slot written), the magnitudes A["x"], A["xc"], A["m"], and `reads`: which of x_corr, h0, h1, h2
    the row lets the kernel load."""

    def __init__(self, x, xc, m, A, reads):
        self.x, self.xc, self.m, self.xin, self.A, self.reads = x, xc, m, x, A, reads


def slots(step):
    """(slot of h0, of h1, of h2 = the slot m is written to) for evaluation `step`."""
    return (step - 1) % 3, (step - 2) % 3, step % 3


def step(x, eps, coefs, step=None, hist=None, x_corr=None, cfg_scale=1.0, cfg=False):
    """x: [B, C, H, W]; eps: the same, or with cfg [2, B, C, H, W] = [uncond ; cond]; coefs: [rows, 12] (the fp32 table
    widened); step: the row (None: row 0); hist: [3, ...] ring, x_corr: like x — looked at only where the row says so."""
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
    c = np.asarray(coefs, dtype=np.float64).reshape(-1, 12)[st]
    s0, s1, s2 = slots(st)
    H = None if hist is None else np.asarray(hist, dtype=np.float64).reshape(3, *x.shape)
    corr = c[11] != 0
    reads = {"x_corr": bool(corr), "h0": bool(corr or c[9] != 0), "h1": bool((corr and c[5] != 0) or c[10] != 0),
             "h2": bool(corr and c[6] != 0)}
    m = (x - c[0] * e) * c[1]
    A_m = (np.abs(x) + abs(c[0]) * Ae) * abs(c[1])
    if corr:
        xc0 = np.asarray(x_corr, dtype=np.float64).reshape(x.shape)
        h0 = H[s0]
        xc = c[2] * xc0 + c[3] * h0 + c[4] * (m - h0)
        A_c = abs(c[2]) * np.abs(xc0) + abs(c[3]) * np.abs(h0) + abs(c[4]) * (A_m + np.abs(h0))
        for w, s in ((c[5], s1), (c[6], s2)):
            if w != 0:
                xc = xc + w * (H[s] - h0)
                A_c = A_c + abs(w) * (np.abs(H[s]) + np.abs(h0))
    else:
        xc, A_c = x, np.abs(x)
    xn = c[7] * xc + c[8] * m
    A_x = abs(c[7]) * A_c + abs(c[8]) * A_m
    for w, s in ((c[9], s0), (c[10], s1)):
        if w != 0:
            xn = xn + w * (H[s] - m)
            A_x = A_x + abs(w) * (np.abs(H[s]) + A_m)
    return Step(xn, xc, m, {"x": A_x, "xc": A_c, "m": A_m}, reads)


def within(got, ref, A, bound=BOUND):
    return np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref) <= bound * A


# --------------------------------------------------------------------------------------------------------------- chain
def chain(model, x_T, timesteps, table):
    """The sampler's loop in fp64 over the rows of `table` ([T, 12], any float dtype; a table built with start= for a chain
    that begins inside the schedule).  model(x, t, i) -> eps (guided: the combined eps) for the integer timestep t of loop
    position i; timesteps: DESCENDING, one per row.  Returns (x, [x after each evaluation], [m of each evaluation])."""
    x = np.asarray(x_T, dtype=np.float64)
    tab = np.asarray(table, dtype=np.float64)
    hist, x_corr, xs, ms = np.full((3,) + x.shape, np.nan), np.full(x.shape, np.nan), [], []
    for i in range(tab.shape[0]):
        r = step(x, model(x, int(timesteps[i]), i), tab, i, hist, x_corr)
        hist[slots(i)[2]] = r.m
        x, x_corr = r.x, r.xc
        xs.append(x)
        ms.append(r.m)
    return x, xs, ms


# ------------------------------------------------------------------------------------------------------ analytic model
def gaussian_error(acp, s2, S, order=2, variant="bh2", corrector=True, lower_order_final=True, paper=False):
    """Relative error of UniPC's final latent on the logSNR grid with S steps, data x0 ~ N(0, s2) (dpm_ref.gaussian_eps);
    paper=True: through paper_chain instead of the table."""
    ts = logsnr_nodes(acp, S)[1:]
    a_t, a_p = tables(acp, ts)
    model, x_T = gaussian_eps(acp, s2), np.asarray([1.0])
    kw = dict(order=order, variant=variant, lower_order_final=lower_order_final, corrector=corrector)
    if paper:
        x = paper_chain(model, x_T, a_t, a_p, ts[::-1], **kw)[0]
    else:
        x = chain(model, x_T, ts[::-1], coefficient_table(a_t, a_p, **kw))[0]
    exact = gaussian_exact(acp, s2, int(ts[-1]), x_T)
    return float(np.abs(x - exact)[0] / np.abs(exact)[0])
