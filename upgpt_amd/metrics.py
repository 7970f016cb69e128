"""SSIM and MS-SSIM of uint8 picture pairs on the device: what scripts/eval_metrics.py:110-111 gets from
pytorch_msssim.ssim / ms_ssim (data_range=1, size_average=False), per image.

The pixel work (11-tap Gaussian moments, the two rational maps, their per-channel means, the 2 x 2 pooling pyramid) is
upk_ssim_u8 (include/upk.h, csrc/metrics.hip): 2 * levels launches per batch, whatever its size.  What is left acts on
6 * levels numbers per image and is written here: the relu, the level weights, the product and the channel mean.
The algorithm is stated in include/upk.h and DESIGN.md 17.

lpips / lpips_layers: the LPIPS (VGG16) column of the same script (its line 112) through an upgpt_amd.lpips.LPIPS
instance that holds the user's weights.

fid_features / FidStats / fid_stats / fid_from_stats: the first line of that script's metrics.txt, pytorch_fid's FID (its line
102): InceptionV3 features through an upgpt_amd.fid.FIDInception that holds the user's weights, the statistics and the
Frechet distance on the host in fp64 numpy.
"""
import numpy as np
import torch

from . import _lib
from ._check import require

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WINDOW = 11          # taps of the Gaussian window: the smallest side a level may have
MS_MIN_SIDE = 160    # ms_ssim needs min(H, W) > 160 = (WINDOW - 1) * 2^4
LPIPS_MIN_SIDE = 16  # lpips needs min(H, W) >= 16: the fifth VGG tap must have a pixel

_WS = {}  # (device index, lane, H, W, levels) -> uint8 workspace tensor, large enough for the largest batch seen


def level_sizes(h, w, levels):
    """[(h, w)] of every level: avg_pool2d(2, 2, padding = size % 2) takes s to (s + 1) // 2."""
    out = []
    for _ in range(levels):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _workspace(ctx, n, h, w, levels):
    """The workspace of a shape, kept per (device, lane, H, W, levels) as the plans are and grown when a larger batch
    comes: one entry per picture size, whatever batch sizes (a directory's tail batches) are seen.  A replaced tensor
    goes back to the caching allocator, which keeps it for the launches already queued on the lane's stream."""
    key = (ctx.device.index, _lib.current_lane(), h, w, levels)
    nbytes = ctx.ssim_ws_bytes(n, h, w, levels)
    require(nbytes > 0, "upk_ssim_ws_bytes refused (%d, %d, %d, %d)" % (n, h, w, levels), RuntimeError)
    with _lib.PLAN_LOCK:
        ws = _WS.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    return ws


def _check_pictures(name, a, b):
    require(torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda,
            "%s needs device tensors: there is no CPU fallback for the HIP path" % name, RuntimeError)
    require(a.dtype == torch.uint8 and b.dtype == torch.uint8, "%s: pictures must be uint8" % name, TypeError)
    require(a.dim() == 4 and a.shape[3] == 3 and a.shape == b.shape,
            "%s: pictures must be two [N, H, W, 3] tensors of one shape, got %s and %s" % (name, tuple(a.shape), tuple(b.shape)),
            ValueError)
    require(a.device == b.device, "%s: both pictures must be on one device" % name, ValueError)
    n, h, w = a.shape[0], a.shape[1], a.shape[2]
    require(n >= 1, "%s: empty batch" % name, ValueError)
    for t in (a, b):
        require(t.stride(3) == 1 and t.stride(2) == 3, "%s: pixels must be dense inside a row" % name, ValueError)
        require(t.stride(1) >= 3 * w, "%s: row pitch %d below 3 * W" % (name, t.stride(1)), ValueError)
        require(n == 1 or t.stride(0) >= (h - 1) * t.stride(1) + 3 * w, "%s: samples overlap (sample stride %d)" % (
            name, t.stride(0)), ValueError)
    return n, h, w


def _check_picture(name, a):
    """One set of pictures, as _check_pictures checks each side of a pair."""
    require(torch.is_tensor(a) and a.is_cuda, "%s needs device tensors: there is no CPU fallback for the HIP path" % name, RuntimeError)
    require(a.dtype == torch.uint8, "%s: pictures must be uint8" % name, TypeError)
    require(a.dim() == 4 and a.shape[3] == 3, "%s: pictures must be [N, H, W, 3], got %s" % (name, tuple(a.shape)), ValueError)
    n, h, w = a.shape[0], a.shape[1], a.shape[2]
    require(n >= 1 and h >= 1 and w >= 1, "%s: empty batch" % name, ValueError)
    require(a.stride(3) == 1 and a.stride(2) == 3, "%s: pixels must be dense inside a row" % name, ValueError)
    require(a.stride(1) >= 3 * w, "%s: row pitch %d below 3 * W" % (name, a.stride(1)), ValueError)
    require(n == 1 or a.stride(0) >= (h - 1) * a.stride(1) + 3 * w, "%s: samples overlap (sample stride %d)" % (name, a.stride(0)),
            ValueError)
    return n, h, w


def ssim_levels(a, b, levels):
    """[N, levels, 3, 2] fp32 on the pictures' device: (ssim_c, cs_c), the means of the SSIM map and of the
    contrast-structure map per level and channel.  a, b: uint8 device tensors [N, H, W, 3], pixels dense inside a row, any
    row pitch / sample stride (a window of a strip is compared in place).  One upk_ssim_u8 call on the current stream;
    no synchronisation.  Host tensors raise: no CPU fallback."""
    n, h, w = _check_pictures("ssim_levels", a, b)
    levels = int(levels)
    require(1 <= levels <= len(MS_WEIGHTS), "ssim_levels: levels must be 1 .. %d, got %d" % (len(MS_WEIGHTS), levels), ValueError)
    hl, wl = level_sizes(h, w, levels)[-1]
    require(min(hl, wl) >= WINDOW, "ssim_levels: level %d of a %d x %d picture is %d x %d, smaller than the %d-tap window" % (
        levels - 1, h, w, hl, wl, WINDOW), ValueError)
    ctx = _lib.get_context(a.device)
    ws = _workspace(ctx, n, h, w, levels)
    out = torch.empty((n, levels, 3, 2), dtype=torch.float32, device=a.device)
    ctx.ssim_u8(a, a.stride(1), a.stride(0), b, b.stride(1), b.stride(0), n, h, w, levels, out, ws, ws.numel())
    return out


def ssim_from_levels(lv):
    """[N] fp64: the channel mean of ssim_c at level 0 (no relu)."""
    return lv[:, 0, :, 0].double().mean(1)


def ms_ssim_from_levels(lv):
    """[N] fp64 of a 5-level result: per channel prod_{l<4} relu(cs_c[l])^w[l] * relu(ssim_c[4])^w[4], then the channel
    mean."""
    require(lv.shape[1] == len(MS_WEIGHTS), "ms_ssim needs %d levels, got %d" % (len(MS_WEIGHTS), lv.shape[1]), ValueError)
    lv = lv.double()
    vals = torch.cat([lv[:, :-1, :, 1], lv[:, -1:, :, 0]], 1).clamp_min(0)  # [N, 5, 3]
    wt = torch.tensor(MS_WEIGHTS, dtype=torch.float64, device=lv.device).view(1, -1, 1)
    return (vals ** wt).prod(1).mean(1)


def ssim(a, b):
    """[N] fp32 device tensor: pytorch_msssim.ssim(X, Y, data_range=1, size_average=False) of the pictures / 255."""
    return ssim_from_levels(ssim_levels(a, b, 1)).float()


def ms_ssim(a, b):
    """[N] fp32 device tensor: pytorch_msssim.ms_ssim(X, Y, data_range=1, size_average=False) of the pictures / 255."""
    _check_pictures("ms_ssim", a, b)
    require(min(a.shape[1], a.shape[2]) > MS_MIN_SIDE, "ms_ssim: the smaller side must be larger than %d, got %d x %d" % (
        MS_MIN_SIDE, a.shape[1], a.shape[2]), ValueError)
    return ms_ssim_from_levels(ssim_levels(a, b, len(MS_WEIGHTS))).float()


def lpips_layers(a, b, net):
    """[N, 5] fp32 on the pictures' device: the five tap distances d_l of lpips.LPIPS(net='vgg')(a / 255, b / 255), what
    scripts/eval_metrics.py:112 computes (ToTensor output, normalize=False).  a, b as for ssim_levels; net: an
    upgpt_amd.lpips.LPIPS on the same device.  Host tensors raise: no CPU fallback."""
    from .lpips import LPIPS
    require(isinstance(net, LPIPS), "lpips needs an upgpt_amd.lpips.LPIPS instance (the weights are the user's)", TypeError)
    _check_pictures("lpips", a, b)
    return net.pairs_u8(a, b)


def lpips_from_layers(lv):
    """[N] fp64: the sum of the five tap values."""
    return lv.double().sum(1)


def lpips(a, b, net):
    """[N] fp32 device tensor: lpips.LPIPS(net='vgg')(a / 255, b / 255) per pair (summed in fp64, rounded once)."""
    return lpips_from_layers(lpips_layers(a, b, net)).float()


def fid_features(x, net):
    """[N, 2048] fp32 on the pictures' device: pytorch_fid's InceptionV3 pool3 features of x / 255 (resized to 299 x 299, 2 x -
    1).  x: uint8 device tensor [N, H, W, 3] as for ssim_levels; net: an upgpt_amd.fid.FIDInception on the same device.  Host
    tensors raise: no CPU fallback."""
    from .fid import FIDInception
    require(isinstance(net, FIDInception), "fid_features needs an upgpt_amd.fid.FIDInception instance (the weights are the user's)",
            TypeError)
    _check_picture("fid_features", x)
    return net.features_u8(x)


class FidStats:
    """The statistics of a set, accumulated batch by batch in fp64 as the sum and the sum of outer products: no [N, 2048]
    array of a whole set is kept.  stats() -> (mu, sigma) with sigma = np.cov(rowvar=False) (divisor N - 1); NaN-filled for
    fewer than two pictures.

    Rows are folded in blocks of exactly CHUNK pictures in arrival order (at most CHUNK - 1 wait in a buffer; stats() folds
    the tail without consuming it), so the arithmetic, and with it every bit of the result, depends on the ORDER of the
    pictures only, never on how they were cut into batches.  That matters: for N < D the Frechet distance amplifies a
    last-bit difference of sigma by many orders of magnitude."""
    CHUNK = 64

    def __init__(self, dims=2048):
        self.n, self.s, self.ss = 0, np.zeros(dims, dtype=np.float64), np.zeros((dims, dims), dtype=np.float64)
        self._pend = np.zeros((0, dims), dtype=np.float64)

    @staticmethod
    def _fold(n, s, ss, rows):
        return n + rows.shape[0], s + rows.sum(0), ss + rows.T @ rows

    def add(self, feat):
        f = np.asarray(feat.detach().cpu() if torch.is_tensor(feat) else feat, dtype=np.float64)
        require(f.ndim == 2 and f.shape[1] == self.s.shape[0], "FidStats.add: features must be [n, %d], got %s" % (
            self.s.shape[0], f.shape), ValueError)
        pend = np.concatenate([self._pend, f], 0)
        while pend.shape[0] >= self.CHUNK:
            self.n, self.s, self.ss = self._fold(self.n, self.s, self.ss, np.ascontiguousarray(pend[:self.CHUNK]))
            pend = pend[self.CHUNK:]
        self._pend = np.ascontiguousarray(pend)
        return self

    @property
    def count(self):
        return self.n + self._pend.shape[0]

    def stats(self):
        n, s, ss = self.n, self.s, self.ss
        if self._pend.shape[0]:
            n, s, ss = self._fold(n, s, ss, self._pend)
        if n < 2:
            return np.full_like(self.s, np.nan), np.full_like(self.ss, np.nan)
        mu = s / n
        return mu, (ss - n * np.outer(mu, mu)) / (n - 1)


def fid_stats(feat):
    """(mu, sigma) of features [N, D] (host or device, any float type), fp64 numpy: mu = mean(feat, 0), sigma = np.cov(feat,
    rowvar=False); NaN-filled for N < 2.  Computed as FidStats computes them, so the batch-wise accumulation of the same
    rows in the same order gives the same bits."""
    f = np.asarray(feat.detach().cpu() if torch.is_tensor(feat) else feat, dtype=np.float64)
    require(f.ndim == 2, "fid_stats: features must be [N, D], got %s" % (f.shape,), ValueError)
    return FidStats(f.shape[1]).add(f).stats()


def fid_from_stats(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr(sqrtm(sigma1 sigma2)), host fp64.  The trace of the principal square
    root is the sum of the square roots of the eigenvalues of sigma1 sigma2 (np.linalg.eigvals, complex square root, real
    part kept): the quantity pytorch_fid takes from scipy.linalg.sqrtm, without scipy.  NaN statistics (a set
    of fewer than two pictures) give NaN."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    require(mu1.shape == mu2.shape and s1.shape == s2.shape == (mu1.shape[0], mu1.shape[0]),
            "fid_from_stats: mean vectors and covariances of different shapes", ValueError)
    if not (np.isfinite(mu1).all() and np.isfinite(mu2).all() and np.isfinite(s1).all() and np.isfinite(s2).all()):
        return float("nan")
    d = mu1 - mu2
    tr_sqrt = np.sqrt(np.linalg.eigvals(s1 @ s2).astype(np.complex128)).real.sum()
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * tr_sqrt)
