"""Host-side noise schedule tables (once per model / once per sample() call).

Numerics follow the reference exactly because the tables are tiny and precision-critical:
betas / alphas_cumprod in float64 numpy then stored fp32 (util.py:21-43, ddpm.py:125-146);
DDIM selection and sigmas per util.py:46-74.  The per-step scalars that the reference
re-materialises with torch.full every step (ddim.py:189-192) are folded here into ONE
device table of 4 fp32 coefficients per step for upk_ddim_step_f32 (8 per step for the DDPM
step, upk_ddpm_step_f32, and for the DPM-Solver++(2M)
step, upk_dpmpp_2m_step_f32, and its SDE form, upk_dpmpp_2m_sde_step_f32; 12 for the UniPC step, upk_unipc_step_f32).
"""
import numpy as np
import torch


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """Only "linear" — what bbox.yaml, the upscale config and every checkpoint of the path use (ddpm.py:85 default).  The
    reference's cosine / sqrt_linear / sqrt variants (util.py:29-40) serve no config on the path and are refused loudly."""
    if schedule != "linear":
        raise NotImplementedError("beta schedule %r is not on the UPGPT inference path (only 'linear' is)" % (schedule,))
    return (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2).numpy()


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    if ddim_discr_method == "uniform":
        stride = num_ddpm_timesteps // num_ddim_timesteps
        steps = np.arange(0, num_ddpm_timesteps, stride)
    elif ddim_discr_method == "quad":
        steps = (np.linspace(0, np.sqrt(num_ddpm_timesteps * .8), num_ddim_timesteps) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    steps = steps + 1  # the +1 gets the final alpha values right (util.py:56-57)
    if verbose:
        print("ddim timesteps:", steps)
    return steps


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    """alphacums: fp32 tensor (the model buffer).  Returns (sigmas f64 tensor, alphas fp32
    tensor, alphas_prev f64 ndarray) — the same types the reference hands back."""
    acp = torch.as_tensor(alphacums).detach().cpu().float()
    idx = torch.as_tensor(np.asarray(ddim_timesteps), dtype=torch.long)
    alphas = acp[idx]
    alphas_prev = np.asarray([float(acp[0])] + acp[idx[:-1]].tolist())
    ap = torch.from_numpy(alphas_prev)
    # fp32 reciprocal first, as torch's mixed ndarray/tensor dispatch does in the reference
    ratio = (1 - alphas).reciprocal().double() * (1 - ap)
    sigmas = eta * torch.sqrt(ratio * (1 - alphas.double() / ap))
    if verbose:
        print("ddim alphas:", alphas, "alphas_prev:", alphas_prev, "sigmas (eta %s):" % eta, sigmas)
    return sigmas, alphas, alphas_prev


def ddim_coefficient_table(alphas, alphas_prev, sigmas, sqrt_one_minus_alphas, order):
    """[len(order), 4] fp32: {sqrt(1-a_t), 1/sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2)}
    for DDIM indices `order` (loop order = descending index).  Scalars are rounded to
    fp32 first, like torch.full((b,1,1,1), value) does in ddim.py:189-192."""
    f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64)).float()
    a, ap, sg, sq = f32(alphas), f32(alphas_prev), f32(sigmas), f32(sqrt_one_minus_alphas)
    idx = torch.as_tensor(np.asarray(order), dtype=torch.long)
    a, ap, sg, sq = a[idx], ap[idx], sg[idx], sq[idx]
    return torch.stack([sq, 1.0 / a.sqrt(), ap.sqrt(), (1.0 - ap - sg ** 2).sqrt()], dim=1).contiguous()


def make_logsnr_timesteps(alphas_cumprod, S):
    """S + 1 integer timesteps `node`, ascending from 0 to T - 1, uniform in lambda = log(alpha / sigma) (half the logSNR)
    as far as integers allow — the grid DPM-Solver++ is derived on: node[k] is the first t nearest to
    lam[0] + (lam[T-1] - lam[0]) * k / S, then made strictly increasing in one ascending pass.  In the DDIM tables:
    ddim_timesteps = node[1:], alphas = acp[node[1:]], alphas_prev = acp[node[:-1]] (the last target is acp[0], as DDIM's)."""
    acp = np.asarray(torch.as_tensor(alphas_cumprod).detach().cpu().numpy(), dtype=np.float64)
    T, S = int(acp.shape[0]), int(S)
    if S < 1:
        raise ValueError("make_logsnr_timesteps: S = %d, need at least one step" % S)
    lam = 0.5 * np.log(acp / (1.0 - acp))
    g = lam[0] + (lam[T - 1] - lam[0]) * np.arange(S + 1, dtype=np.float64) / S
    node = np.abs(lam[None, :] - g[:, None]).argmin(axis=1).astype(np.int64)  # (argmin: the first minimiser)
    for k in range(1, S + 1):
        node[k] = max(node[k], node[k - 1] + 1)
    if node[0] < 0 or node[-1] > T - 1:
        raise ValueError("make_logsnr_timesteps: %d strictly increasing steps do not fit into %d timesteps" % (S, T))
    return node


def dpm_coefficient_table(alphas, alphas_prev, order=2, lower_order_final=None):
    """[S, 8] fp32 rows of upk_dpmpp_2m_step_f32 in LOOP order (descending DDIM index) from the DDIM tables `alphas` /
    `alphas_prev` (ascending index, as DDIMSampler keeps them).  Row i, step t -> p with alpha = sqrt(a), sigma = sqrt(1 - a),
    lambda = log(alpha / sigma), h_i = lambda_p - lambda_t > 0:
        {sigma_t, 1 / alpha_t, sigma_p / sigma_t, -alpha_p * expm1(-h_i), w_i, 0, 0, 0}
    w_i = h_i / (2 h_{i-1}) (= 1 / (2 r_i)) on a second-order row; 0 on a first-order one: row 0, every row with order = 1,
    and the last row with lower_order_final (default: S < 15, the usual rule for few steps).  Computed in fp64 and rounded
    once."""
    if order not in (1, 2):
        raise ValueError("dpm_coefficient_table: order %r (1 or 2)" % (order,))
    f64 = lambda v: np.asarray(torch.as_tensor(v).detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
    a_t, a_p = f64(alphas)[::-1], f64(alphas_prev)[::-1]
    S = int(a_t.shape[0])
    if lower_order_final is None:
        lower_order_final = S < 15
    al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1.0 - a_t), np.sqrt(a_p), np.sqrt(1.0 - a_p)
    h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
    if not (h > 0).all():
        raise ValueError("dpm_coefficient_table: the logSNR must rise along the chain")
    w = np.zeros(S)
    if order == 2:
        w[1:] = h[1:] / (2.0 * h[:-1])
        if lower_order_final:
            w[-1] = 0.0
    rows = np.zeros((S, 8))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = sg_t, 1.0 / al_t, sg_p / sg_t, -al_p * np.expm1(-h), w
    return torch.from_numpy(rows.astype(np.float32)).contiguous()


def dpm_sde_coefficient_table(alphas, alphas_prev, eta=1.0, order=2, lower_order_final=None, start=0):
    """[S - start, 8] fp32 rows of upk_dpmpp_2m_sde_step_f32 in LOOP order from the DDIM tables `alphas` / `alphas_prev`
    (ascending index).  Points k = 0 .. S as in unipc_coefficient_table; the chain starts at point `start` with no history.
    Row i - start is the step s -> t from point i to point i + 1, h = lambda_t - lambda_s > 0:
        {sigma_s, 1 / alpha_s, (sigma_t / sigma_s) exp(-eta h), -alpha_t expm1(-(1 + eta) h), w, sigma_t sqrt(-expm1(-2 eta h)), 0, 0}
    w = h_i / (2 h_{i-1}) on a second-order row, 0 on a first-order one: the order of row i is min(order, i + 1 - start), and
    the last row is first-order with lower_order_final (None: S < 15, DPMSolverSampler's rule).  Entry 5 is the row's noise
    scale, read by the host only (0 exactly when eta = 0).  eta = 0: dpm_coefficient_table's rows.  Computed in fp64 and
    rounded once."""
    if order not in (1, 2):
        raise ValueError("dpm_sde_coefficient_table: order %r (1 or 2)" % (order,))
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError("dpm_sde_coefficient_table: eta %r outside [0, 1]" % (eta,))
    f64 = lambda v: np.asarray(torch.as_tensor(v).detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
    a_t, a_p = f64(alphas)[::-1], f64(alphas_prev)[::-1]
    S, start = int(a_t.shape[0]), int(start)
    if not 0 <= start < S:
        raise ValueError("dpm_sde_coefficient_table: start %d outside the %d-step chain" % (start, S))
    if lower_order_final is None:
        lower_order_final = S < 15
    a = np.concatenate([a_t, a_p[-1:]])  # the S + 1 points
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    h = np.diff(np.log(al / sg))
    if not (h > 0).all():
        raise ValueError("dpm_sde_coefficient_table: the logSNR must rise along the chain")
    w = np.zeros(S)
    if order == 2:
        w[start + 1:] = h[start + 1:] / (2.0 * h[start:-1])
        if lower_order_final:
            w[-1] = 0.0
    rows = np.zeros((S, 8))
    rows[:, 0], rows[:, 1], rows[:, 4] = sg[:-1], 1.0 / al[:-1], w
    rows[:, 2] = sg[1:] / sg[:-1] * np.exp(-eta * h)
    rows[:, 3] = -al[1:] * np.expm1(-(1.0 + eta) * h)
    rows[:, 5] = sg[1:] * np.sqrt(-np.expm1(-2.0 * eta * h))
    return torch.from_numpy(rows[start:].astype(np.float32)).contiguous()


def _unipc_rho(r, h, variant):
    """The solution rho of UniPC's system R rho = b (Zhao et al. 2023, theorem 3.1) for the nodes r = [r_1 .. r_n]:
    R[i][j] = r_j^i, b[i] = (i + 1)! z phi_{i+2}(z) / B(h) with z = -h (the data prediction's sign), phi_1(z) = expm1(z) / z,
    phi_{k+1}(z) = (phi_k(z) - 1 / k!) / z, i = 0 .. n - 1; fp64."""
    n, hh = len(r), -h
    B = np.expm1(hh) if variant == "bh2" else hh
    phi, fact, b = np.expm1(hh) / hh - 1.0, 1.0, []
    for i in range(1, n + 1):
        b.append(phi * fact / B)
        fact *= i + 1
        phi = phi / hh - 1.0 / fact
    R = np.asarray([[rj ** i for rj in r] for i in range(n)], dtype=np.float64)
    return np.linalg.solve(R, np.asarray(b, dtype=np.float64))


def unipc_coefficient_table(alphas, alphas_prev, order=2, variant="bh2", lower_order_final=True, corrector=True, start=0):
    """[S - start, 12] fp32 rows of upk_unipc_step_f32 in LOOP order from the DDIM tables `alphas` / `alphas_prev` (ascending
    index).  The chain's points are numbered k = 0 .. S in loop order (point k < S is DDIM index S - 1 - k, point S the last
    target alphas_prev[0]), lambda = log(alpha / sigma) ascends; the chain starts at point `start` with no history.  Row
    k - start belongs to the model evaluation at point k (include/upk.h for the layout):
      predictor k -> k+1 of order p_k = min(order, k + 1 - start, S - k) (the last term with lower_order_final), on the nodes
        r_i = (lambda_{k-i} - lambda_k) / h_p, i = 1 .. p_k - 1: weights -alpha_{k+1} B(h_p) rho_i / r_i, rho from the system
        without its last row and column, [0.5] at order 2;
      corrector of k-1 -> k (none at point `start`, none with corrector=False) of order p_{k-1}, nodes r_i = (lambda_{k-1-i} -
        lambda_{k-1}) / h_c and r = 1 for m_k itself: weights -alpha_k B(h_c) rho_i / r_i, [0.5] at order 1.
    B(h) = expm1(-h) ("bh2") or -h ("bh1").  Computed in fp64 and rounded once."""
    if order not in (1, 2, 3):
        raise ValueError("unipc_coefficient_table: order %r (1, 2 or 3)" % (order,))
    if variant not in ("bh1", "bh2"):
        raise ValueError("unipc_coefficient_table: variant %r (bh1 or bh2)" % (variant,))
    f64 = lambda v: np.asarray(torch.as_tensor(v).detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
    a_t, a_p = f64(alphas)[::-1], f64(alphas_prev)[::-1]
    S, start = int(a_t.shape[0]), int(start)
    if not 0 <= start < S:
        raise ValueError("unipc_coefficient_table: start %d outside the %d-step chain" % (start, S))
    a = np.concatenate([a_t, a_p[-1:]])  # the S + 1 points
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    lam = np.log(al / sg)
    if not (np.diff(lam) > 0).all():
        raise ValueError("unipc_coefficient_table: the logSNR must rise along the chain")
    B = (lambda h: np.expm1(-h)) if variant == "bh2" else (lambda h: -h)
    p_of = lambda k: min(order, k + 1 - start, S - k if lower_order_final else order)
    rows = np.zeros((S - start, 12))
    for k in range(start, S):
        row, p = rows[k - start], p_of(k)
        row[0], row[1] = sg[k], 1.0 / al[k]
        h = lam[k + 1] - lam[k]
        row[7], row[8] = sg[k + 1] / sg[k], -al[k + 1] * np.expm1(-h)
        if p > 1:
            r = [(lam[k - i] - lam[k]) / h for i in range(1, p)]
            rho = np.asarray([0.5]) if p == 2 else _unipc_rho(r, h, variant)
            row[9:9 + p - 1] = -al[k + 1] * B(h) * rho / np.asarray(r)
        if corrector and k > start:
            q = p_of(k - 1)
            h = lam[k] - lam[k - 1]
            r = [(lam[k - 1 - i] - lam[k - 1]) / h for i in range(1, q)] + [1.0]
            rho = np.asarray([0.5]) if q == 1 else _unipc_rho(r, h, variant)
            row[2], row[3] = sg[k] / sg[k - 1], -al[k] * np.expm1(-h)
            row[4] = -al[k] * B(h) * rho[-1]
            row[5:5 + q - 1] = -al[k] * B(h) * rho[:-1] / np.asarray(r[:-1])
            row[11] = 1.0
    return torch.from_numpy(rows.astype(np.float32)).contiguous()


def ddpm_coefficient_table(model, t_order):
    """[len(t_order), 8] fp32 rows of upk_ddpm_step_f32 for the DDPM timesteps `t_order` (loop order), gathered from
    the model's fp32 schedule buffers and combined in fp32 as ddpm.py:1125-1187 does:
    {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2,
     nonzero(t) * (0.5 * posterior_log_variance_clipped).exp(), sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, 0}.
    The sampling temperature multiplies the noise (ddpm.py:1174), so it is folded into the noise table, not here."""
    t = torch.as_tensor(np.asarray(t_order), dtype=torch.long)
    buf = lambda name: getattr(model, name).detach().to("cpu", torch.float32)[t]
    nonzero = 1 - (t == 0).float()
    cols = [buf("sqrt_recip_alphas_cumprod"), buf("sqrt_recipm1_alphas_cumprod"), buf("posterior_mean_coef1"),
            buf("posterior_mean_coef2"), nonzero * (0.5 * buf("posterior_log_variance_clipped")).exp(),
            buf("sqrt_alphas_cumprod"), buf("sqrt_one_minus_alphas_cumprod"), torch.zeros(t.shape[0])]
    return torch.stack(cols, dim=1).contiguous()


def extract_into_tensor(a, t, x_shape):
    b = t.shape[0]
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))
