"""numpy restatement of the low-resolution conditioning transform (app.py:93-97, deepfashion_inshop.py:427-431):
T.Pad(edge) -> T.Resize(BILINEAR) on a PIL picture -> T.ToTensor() -> x * 2 - 1.

T.Resize on a PIL picture is Pillow's two-pass integer resampling: per axis a table of 22-bit fixed-point weights built
in double, the horizontal pass first with its result rounded to uint8, then the vertical pass on those bytes; a pass
whose size does not change is skipped.  tests/test_resize_host.py pins this file to PIL.Image.resize byte for byte.
The fp32 finishing is ToTensor's u / 255 (one fp32 division) followed by * 2 (exact) and - 1 (one rounding), in
np.float32 operations."""
import numpy as np

PRECISION_BITS = 22


def coeffs(in_size, out_size):
    """(bounds int32 [out, 2] = (xmin, n), k int32 [out, ksize], ksize) of the triangle filter, every step in double."""
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx] = (xmin, n)
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(v * float(1 << PRECISION_BITS) + 0.5)
    return bounds, k, ksize


def one_pass(img, bounds, k, axis):
    """img uint8 [H, W, C]; resamples `axis` (0 rows, 1 columns) with int32 accumulators."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(int(n)):
            acc += src[lo + t] * int(k[i, t])
        assert int(acc.max()) < 2 ** 31
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pad_edge(img, pad):
    """T.Pad((pad_x, pad_y), padding_mode='edge') on [H, W, C] by index clamping."""
    px, py = pad
    h, w = img.shape[:2]
    ys = np.clip(np.arange(h + 2 * py) - py, 0, h - 1)
    xs = np.clip(np.arange(w + 2 * px) - px, 0, w - 1)
    return img[ys][:, xs]


def resize(img, size, pad=(0, 0)):
    """uint8 [H, W, C] -> uint8 [oh, ow, C]: edge pad, horizontal pass (to bytes), vertical pass."""
    oh, ow = size
    x = pad_edge(np.asarray(img, dtype=np.uint8), pad)
    if x.shape[1] != ow:
        b, k, _ = coeffs(x.shape[1], ow)
        x = one_pass(x, b, k, 1)
    if x.shape[0] != oh:
        b, k, _ = coeffs(x.shape[0], oh)
        x = one_pass(x, b, k, 0)
    return np.ascontiguousarray(x)


def to_lr(u8):
    """ToTensor then x * 2. - 1. on uint8 [..., H, W, 3] -> fp32 of the same layout: fl(fl(u / 255) * 2 - 1)."""
    t = u8.astype(np.float32) / np.float32(255.0)
    return t * np.float32(2.0) - np.float32(1.0)


def lr_transform(pictures, size, pad=(0, 0)):
    """uint8 [B, H, W, 3] -> (lr fp32 [B, 3, oh, ow], lr_image fp32 [B, oh, ow, 3], the bytes [B, oh, ow, 3])."""
    u8 = np.stack([resize(p, size, pad) for p in np.asarray(pictures)])
    hwc = to_lr(u8)
    return np.ascontiguousarray(hwc.transpose(0, 3, 1, 2)), hwc, u8
