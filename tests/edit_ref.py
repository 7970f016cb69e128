"""fp64 restatement of ONE launch of upk_ddim_step_edit_f32 (include/upk.h), its inputs and modes, and the chain a sampler
builds from it — shared by tests/test_ddim_edit_host.py and tests/test_ddim_edit_gpu.py.  Built on oracle/steps.py (the
update, the guidance combination, the seeded inputs and the bound); nothing here is read by the package.

Written from the reference's loop, ldm/models/diffusion/ddim.py:140-163: a masked step is
    img = q_sample(x0, ts) * mask + (1 - mask) * img        (144-147, BEFORE the model evaluation)
    img, pred_x0 = p_sample_ddim(img, ...)                  (150-157)
and `img` as p_sample_ddim returned it — unblended — is what is logged and, after the last step, returned.  The kernel
applies the blend of step r + 1 at the end of step r (row r + 1 of `keep`) and leaves the last row's result alone.

The bound.  oracle/steps.py derives |got - ref64| <= 32 * 2^-24 * A from the longest fp32 path of the four step kernels
(17 roundings, PLMS with guidance at order 4), A being the expression with every operand replaced by its magnitude.
This kernel's longest path is guidance (3) + update (6) + noise (1) + the blend m * k + (1 - m) * x_prev: one rounding
each for 1 - m, the two products and their sum (4): 14 roundings, inside the same constant.  The blend adds two products,
so A grows the way it does for the DDPM blend there:  A_x = |m| |k| + (1 + |m|) A_xprev  (|1 - m| <= 1 + |m|).  x_plain and
pred_x0 keep the magnitudes of the plain update."""
import numpy as np
import torch

from oracle import steps as st

SCALE = st.CFG_SCALE
ROWS = st.ROWS


class EditResult:
    """x (what goes to x and, before its fp16 rounding, to xin), x_plain, pred_x0: float64 CPU; A: name -> magnitude."""

    def __init__(self, x, x_plain, pred_x0, A):
        self.x, self.xin, self.x_plain, self.pred_x0, self.A = x, x, x_plain, pred_x0, A


def ddim_step_edit(x, eps, coefs, noise=None, keep=None, mask=None, n_rows=0, step=None, scale=1.0, cfg=False):
    """upk_ddim_step_edit_f32 on the operands of its C entry point (None = NULL)."""
    x = st._d(x)
    if cfg:
        e, Ae = st._guided(eps, x, scale)
    else:
        e = st._d(eps).reshape(x.shape)
        Ae = e.abs()
    s, row = st._row(coefs, step, 4)
    xp, p0, A_x, A_p = st._ddim_update(x, e, Ae, row, st._table_row(noise, s, x))
    xo, A_o = xp, A_x
    if mask is not None and s + 1 < int(n_rows):
        mk, kp = st._d(mask).reshape(x.shape), st._table_row(keep, s + 1, x)
        xo = mk * kp + (1.0 - mk) * xp
        A_o = mk.abs() * kp.abs() + (1.0 + mk.abs()) * A_x
    return EditResult(xo, xp, p0, {"x": A_o, "xin": A_o, "x_plain": A_x, "pred_x0": A_p})


def make_inputs(shape, rows=ROWS):
    """Seeded fp32 CPU operands at one shape: oracle/steps.py's guided-DDIM set plus a keep table with distinct rows and
    a mask holding 0, 1 and values strictly inside (0, 1)."""
    inp = st.make_inputs("ddim_cfg", shape, rows)
    n = inp["n"]
    g = torch.Generator().manual_seed(4242 + n + shape[0])
    inp["keep"] = 1.5 * torch.randn(rows, n, generator=g)
    i = torch.arange(n)
    inp["mask"] = torch.where(i % 3 == 0, torch.zeros(n), torch.where(i % 3 == 1, torch.ones(n),
                                                                      0.1 + 0.8 * torch.rand(n, generator=g)))
    return inp


def modes(rows=ROWS):
    """Every combination of cfg, noise, mask, x_plain and last row or not, with pred_x0 / xin / step present; then the
    NULL cases of pred_x0, xin and step on the fullest mode.  `step` is the row; rows - 1 is the last one."""
    out = []
    for cfg in (False, True):
        for noise in (False, True):
            for mask in (False, True):
                for plain in (False, True):
                    for step in (rows // 2, rows - 1):
                        out.append(dict(cfg=cfg, noise=noise, mask=mask, plain=plain, step=step, pred=True, xin=True))
    full = dict(cfg=True, noise=True, mask=True, plain=True, step=rows // 2, pred=True, xin=True)
    out += [dict(full, **{k: False}) for k in ("pred", "xin")]
    out += [dict(full, step=None), dict(full, step=None, cfg=False), dict(full, step=0)]
    return out


def operands(inp, mode):
    """Keyword arguments of ddim_step_edit for one mode."""
    return dict(x=inp["x"], eps=inp["eps"] if mode["cfg"] else inp["eps"][0], coefs=inp["coefs"],
                noise=inp["noise"] if mode["noise"] else None, keep=inp["keep"] if mode["mask"] else None,
                mask=inp["mask"] if mode["mask"] else None, n_rows=inp["rows"], step=mode["step"], scale=SCALE,
                cfg=mode["cfg"])


# ---------------------------------------------------------------------------------------------------------------------
# chains: what DDIMSampler._fast_sampling builds from the kernel, restated in fp64
# ---------------------------------------------------------------------------------------------------------------------
def q_sample_fn(acp, noises):
    """q_sample(x0, t) = sqrt(a_t) x0 + sqrt(1 - a_t) noise (ddpm.py:271-274) drawing its noise from `noises` in call
    order, as the reference's draws one randn per call."""
    feed = iter(noises)
    a = torch.as_tensor(np.asarray(acp, dtype=np.float64))

    def q(x0, t):
        at = a[t.long()].reshape(-1, 1, 1, 1)
        return (at.sqrt() * x0 + (1.0 - at).sqrt() * next(feed)).to(x0.dtype)
    return q


def edit_chain(eps_fn, S, eta, x_T, cond, uncond=None, scale=1.0, noise=None, mask=None, x0=None, q_sample=None,
               t_steps=None):
    """The sampler's side of a chain over the last `t_steps` (default S) loop positions, all in fp64: the keep rows are
    filled in loop order, the first latent is blended here, and every step is ONE ddim_step_edit at the row the device
    counter would hold.  -> (x_0, [x_plain or x per step], [pred_x0 per step])"""
    ts, coefs, sig = st.kernel_tables(S, eta)
    coefs = coefs.double()
    T = S if t_steps is None else int(t_steps)
    k = S - T
    shape, b = tuple(x_T.shape), x_T.shape[0]
    n = x_T.numel()
    keep = None
    if mask is not None:
        keep = torch.zeros(S, n, dtype=torch.float64)
        for r in range(k, S):
            keep[r] = q_sample(x0, torch.full((b,), int(ts[r]), dtype=torch.long)).reshape(-1)
        emask = mask.double().expand(shape).reshape(-1)
    nz = None
    if noise is not None and eta > 0:  # rows k ... S - 1 hold sigma_t * randn of local steps 0 ... T - 1
        nz = torch.zeros(S, n, dtype=torch.float64)
        nz[k:] = sig.double()[k:, None] * noise.double().reshape(T, n)
    x = x_T.double()
    if mask is not None:
        x = keep[k].view(shape) * mask.double() + (1.0 - mask.double()) * x
    xs, preds = [], []
    for r in range(k, S):
        t = torch.full((b,), int(ts[r]), dtype=torch.long)
        if uncond is None:
            eps = eps_fn(x, t, cond)
        else:
            eps = torch.stack([eps_fn(x, t, uncond), eps_fn(x, t, cond)])
        res = ddim_step_edit(x, eps, coefs, nz, keep, emask if mask is not None else None, S, r, scale,
                             uncond is not None)
        x = res.x
        xs.append(res.x_plain)
        preds.append(res.pred_x0)
    return x, xs, preds
