"""fp64 numpy restatement of q_sample (ddpm.py:271-274) and of the loss of p_losses (ddpm.py:1101-1121) — the reference
tests/test_loss_host.py and tests/test_loss_gpu.py share.  Everything is exact arithmetic on the given inputs up to fp64
rounding; nothing here imitates the order or the precision of the code under test."""
import numpy as np

F64 = np.float64


def q_sample(x_start, noise, t, sqrt_ac, sqrt_1m_ac):
    """[B, C, H, W] fp64: a[t_b] * x_start + s[t_b] * noise."""
    t = np.asarray(t, dtype=np.int64)
    a = np.asarray(sqrt_ac, dtype=F64)[t].reshape(-1, 1, 1, 1)
    s = np.asarray(sqrt_1m_ac, dtype=F64)[t].reshape(-1, 1, 1, 1)
    return a * np.asarray(x_start, dtype=F64) + s * np.asarray(noise, dtype=F64)


def get_loss(pred, target, loss_type="l2", mean=True):
    d = np.asarray(target, dtype=F64) - np.asarray(pred, dtype=F64)
    e = np.abs(d) if loss_type == "l1" else d * d
    return e.mean() if mean else e


def p_losses(model_out, target, t, logvar, lvlb_weights, loss_w=None, loss_type="l2", l_simple_weight=1.0,
             original_elbo_weight=0.0):
    """dict of fp64 values: simple [B], plain [B], loss_simple, loss_gamma, loss_vlb, loss, and gamma_mag / loss_mag, the
    sums of the magnitudes of the terms of loss_gamma / loss (what an absolute tolerance on them scales with)."""
    e = get_loss(model_out, target, loss_type, mean=False)
    B = e.shape[0]
    we = e if loss_w is None else np.asarray(loss_w, dtype=F64) * e
    simple = we.reshape(B, -1).mean(1)
    plain = e.reshape(B, -1).mean(1)
    t = np.asarray(t, dtype=np.int64)
    lv = np.asarray(logvar, dtype=F64)[t]
    lw = np.asarray(lvlb_weights, dtype=F64)[t]
    gamma = (simple / np.exp(lv) + lv).mean()
    gamma_mag = (np.abs(simple / np.exp(lv)) + np.abs(lv)).mean()
    vlb = (lw * plain).mean()
    lsw, oew = F64(l_simple_weight), F64(original_elbo_weight)
    return {"simple": simple, "plain": plain, "loss_simple": simple.mean(), "loss_gamma": gamma, "loss_vlb": vlb,
            "loss": lsw * gamma + oew * vlb, "gamma_mag": gamma_mag,
            "loss_mag": abs(lsw) * gamma_mag + abs(oew) * np.abs(lw * plain).mean()}


def fixture_inputs(seed):
    """(x_start, noise, loss_w [B, 1, 32, 24], cond) of tests/golden/loss.npz as torch CPU tensors, rebuilt from the recipe
    the way tests/golden/make_loss_golden.py builds them (B = 2, latent 4 x 32 x 24, 87 context tokens)."""
    import torch
    from upgpt_amd import synth
    inp = synth.synth_inputs(2, (32, 24), 4, 87, 768, seed=int(seed), steps=1)
    loss_w = torch.ones(2, 1, 32, 24)
    loss_w[:, :, 0:8] = 2.0
    loss_w[:, :, 20:32] = 0.5
    cond = {"c_crossattn": inp["c_crossattn"], "c_concat": [inp["c_concat"]]}
    return 0.18215 * 4.0 * inp["x_T"], inp["noise"][0], loss_w, cond
