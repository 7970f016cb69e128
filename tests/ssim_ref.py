"""SSIM / MS-SSIM as scripts/eval_metrics.py:110-111 computes them (pytorch_msssim.ssim / ms_ssim, data_range=1,
size_average=False), restated in torch on the CPU in a chosen dtype.  Imports nothing from upgpt_amd.

Inputs are uint8 [N, H, W, 3]; X = u / 255 per channel.  Window g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), 11 taps, sum 1,
separable along H then W, valid; C1 = 0.01^2, C2 = 0.03^2; cs_map = (2 s12 + C2) / (s11 + s22 + C2), ssim_map =
(2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map; per-channel means; SSIM = channel mean at level 0; MS-SSIM = channel
mean of prod_{l<4} relu(cs[l])^w[l] * relu(ssim[4])^w[4] over a pyramid of avg_pool2d(2, 2, padding = size % 2,
count_include_pad=True).

The keyword arguments of `levels` exist only to build WRONG variants for the test that the tolerance discriminates.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype, taps=11, sigma=1.5):
    c = torch.arange(taps, dtype=dtype) - taps // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blur(x, g, same=False):
    """x [N, 3, H, W]: the window along H, then along W; valid, or zero-padded to the same size."""
    t = g.numel()
    if same:
        x = F.pad(x, (t // 2, t // 2, t // 2, t // 2))
    h, w = x.shape[2] - t + 1, x.shape[3] - t + 1
    y = sum(g[k] * x[:, :, k:k + h, :] for k in range(t))
    return sum(g[k] * y[:, :, :, k:k + w] for k in range(t))


def pool(x, pad=True):
    """avg_pool2d(x, 2, 2, padding=(H % 2, W % 2), count_include_pad=True) written out: a zero row / column in FRONT of
    an odd axis, then 2 x 2 block means with the divisor 4.  pad=False (a wrong variant) drops the last row / column of
    an odd axis instead."""
    h, w = x.shape[2], x.shape[3]
    if pad:
        x = F.pad(x, (w % 2, 0, h % 2, 0))
    else:
        x = x[:, :, :h - h % 2, :w - w % 2]
    n, c, h, w = x.shape
    return x.reshape(n, c, h // 2, 2, w // 2, 2).sum((3, 5)) / 4


def levels(a, b, nlevels, dtype=torch.float64, taps=11, sigma=1.5, same=False, pool_pad=True):
    """[N, nlevels, 3, 2] of `dtype`: (ssim_c, cs_c) per level and channel."""
    x = torch.as_tensor(a).permute(0, 3, 1, 2).to(dtype) / 255
    y = torch.as_tensor(b).permute(0, 3, 1, 2).to(dtype) / 255
    g = window(dtype, taps, sigma)
    out = []
    for l in range(nlevels):
        mu1, mu2 = blur(x, g, same), blur(y, g, same)
        s11 = blur(x * x, g, same) - mu1 * mu1
        s22 = blur(y * y, g, same) - mu2 * mu2
        s12 = blur(x * y, g, same) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        out.append(torch.stack([ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)], -1))
        if l + 1 < nlevels:
            x, y = pool(x, pool_pad), pool(y, pool_pad)
    return torch.stack(out, 1)


def ssim_of(lv):
    return lv[:, 0, :, 0].mean(1)


def ms_ssim_of(lv):
    assert lv.shape[1] == 5
    vals = torch.relu(torch.cat([lv[:, :-1, :, 1], lv[:, -1:, :, 0]], 1))
    wt = torch.tensor(MS_WEIGHTS, dtype=lv.dtype).view(1, 5, 1)
    return (vals ** wt).prod(1).mean(1)


def metrics(a, b, nlevels, dtype=torch.float64, **variant):
    """(raw [N, L, 3, 2], SSIM [N], MS-SSIM [N] or None when nlevels < 5), all of `dtype`."""
    lv = levels(a, b, nlevels, dtype, **variant)
    return lv, ssim_of(lv), (ms_ssim_of(lv) if nlevels == 5 else None)


# ---- the inputs and cases of the GPU test (tests/test_metrics_gpu.py), shared with the host test that shows the
# tolerance discriminates
SHAPES = [(11, 11, 1), (12, 27, 1), (23, 37, 1), (64, 48, 1), (176, 161, 5), (256, 176, 5)]
KINDS = ["noise", "smooth", "flat", "same"]


def make_pair(kind, n, h, w, seed=0):
    """Two uint8 [n, h, w, 3] arrays."""
    rng = np.random.RandomState(seed + 1000 * h + w)
    if kind == "noise":  # independent bytes: cs goes negative
        return rng.randint(0, 256, (n, h, w, 3), dtype=np.uint8), rng.randint(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind in ("smooth", "same"):  # a sinusoid, and the same plus Gaussian noise of 12 grey levels
        yy, xx = np.mgrid[0:h, 0:w]
        ph = rng.uniform(0, 2 * math.pi, (n, 1, 1, 3))
        base = 128 + 90 * np.sin(yy[None, :, :, None] / 7.0 + ph) * np.cos(xx[None, :, :, None] / 5.0 + 0.5 * ph)
        a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
        if kind == "same":
            return a, a.copy()
        return a, np.clip(np.rint(base + 12 * rng.standard_normal((n, h, w, 3))), 0, 255).astype(np.uint8)
    assert kind == "flat"  # 255 against 254 on half the picture, plus a 3 x 3 black corner: sigma^2 is pure cancellation
    a = np.full((n, h, w, 3), 255, dtype=np.uint8)
    b = a.copy()
    b[:, :, w // 2:] = 254
    a[:, :3, :3] = 0
    return a, b


def tolerance(a, b, nlevels):
    """(fp64 results, bounds): per quantity (raw, SSIM, MS-SSIM) the bound 4 * e32 + 5e-6 with e32 = max |fp32
    restatement - fp64 restatement|.  4: the same arithmetic class in another summation order; 5e-6: 1 / 20 of the
    fourth decimal papers report (`same` has e32 = 0)."""
    r64 = metrics(a, b, nlevels, torch.float64)
    r32 = metrics(a, b, nlevels, torch.float32)
    e32 = [None if v64 is None else float((v32.double() - v64).abs().max()) for v64, v32 in zip(r64, r32)]
    return r64, e32, [None if e is None else 4 * e + 5e-6 for e in e32]
