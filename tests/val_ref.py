"""fp64 numpy restatement of the keyed loss evaluation (include/upk.h upk_q_sample_keyed_f32, evaluate.validation_means),
built on tests/rng_ref.py (the Philox words and normals) and tests/loss_ref.py (q_sample).  Nothing here imports the code
under test."""
import numpy as np

import loss_ref
import rng_ref

STREAM_TIMESTEP, STREAM_LOSS_NOISE = 4, 5


def timesteps(keys, n_t, draw=0):
    """int64 [B]: (w0 * n_t) >> 32 with w0 = word 0 of the Philox call (0, 0, STREAM_TIMESTEP, draw) of every key."""
    w0 = rng_ref.words(keys, 4, 0, 1, STREAM_TIMESTEP, draw)[0, :, 0].astype(np.uint64)
    return ((w0 * np.uint64(n_t)) >> np.uint64(32)).astype(np.int64)


def noise(keys, n, draw=0):
    """float64 [B, n]: the normals of counter (e >> 2, 0, STREAM_LOSS_NOISE, draw)."""
    return rng_ref.normals(keys, n, 0, 1, STREAM_LOSS_NOISE, draw)[0]


def q_sample_keyed(keys, draw, x_start, sqrt_ac, sqrt_1m_ac, t=None):
    """(t [B], noise [B, C, H, W], x_noisy [B, C, H, W]) in fp64 for x_start [B, C, H, W]."""
    x_start = np.asarray(x_start, dtype=np.float64)
    t = timesteps(keys, len(sqrt_ac), draw) if t is None else np.asarray(t, dtype=np.int64)
    nz = noise(keys, int(np.prod(x_start.shape[1:])), draw).reshape(x_start.shape)
    return t, nz, loss_ref.q_sample(x_start, nz, t, sqrt_ac, sqrt_1m_ac)


def shard(n_batches, rank, world):
    return [j for j in range(n_batches) if j % world == rank]


def epoch_means(table, lvlb, logvar, l_simple_weight=1.0, original_elbo_weight=0.0, prefix="val"):
    """{key: fp64} of a per-sample table [N, 6] (t, simple, plain, t_ema, simple_ema, plain_ema): the means over the
    samples, summed with numpy (another order than the code under test: compare with a tolerance of a few ulp)."""
    table = np.asarray(table, dtype=np.float64)
    lvlb, logvar = np.asarray(lvlb, dtype=np.float64), np.asarray(logvar, dtype=np.float64)
    out = {}
    for suffix, off in (("", 0), ("_ema", 3)):
        t = table[:, off].astype(np.int64)
        simple, plain = table[:, off + 1], table[:, off + 2]
        gamma = (simple / np.exp(logvar[t]) + logvar[t]).mean()
        vlb = (lvlb[t] * plain).mean()
        out[prefix + "/loss_simple" + suffix] = simple.mean()
        out[prefix + "/loss_vlb" + suffix] = vlb
        out[prefix + "/loss" + suffix] = l_simple_weight * gamma + original_elbo_weight * vlb
    return out
