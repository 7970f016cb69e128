"""The step between the two models: a generated low-resolution picture -> the `lr` concat conditioning of the upscale
model.  The reference does it on the host with torchvision on a PIL picture (app.py:93-97 with p = 4,
deepfashion_inshop.py:427-431 with p = 8):

    T.Pad((p, 0), padding_mode='edge') -> T.Resize(size, BILINEAR) -> T.ToTensor() -> x * 2. - 1.

Here the whole chain is one upk_resize_bilinear_u8 launch (include/upk.h) on uint8 device pictures, the
very bytes upk_image_finish_u8 writes.  T.Resize on a PIL picture is Pillow's two-pass fixed-point resampling; the
coefficient tables are built here in double, exactly as Pillow builds them, and the kernel's integer passes reproduce
its bytes bit for bit.  No CPU fallback: without a GPU these functions raise."""
import math

import numpy as np
import torch

from . import _lib
from ._check import require

PRECISION_BITS = 22  # Pillow's 8-bit-per-channel coefficient scale
_tables = {}  # (device index, in, out) -> (bounds, k, ksize) on the device


def resample_coeffs(in_size, out_size):
    """The triangle-filter table of one axis: (bounds int32 [out, 2] = (xmin, n), k int32 [out, ksize], ksize) as host
    arrays, or None for in_size == out_size (the pass is skipped).  Every step in double, in this order: scale = in /
    out, fs = max(scale, 1), support = fs; per output xx: center = (xx + 0.5) scale, xmin = max(int(center - support +
    0.5), 0), xmax = min(int(center + support + 0.5), in), w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fs|), divided
    by their sum (accumulated left to right), k[x] = int(w[x] * 2^22 + 0.5)."""
    in_size, out_size = int(in_size), int(out_size)
    require(in_size >= 1 and out_size >= 1, "resample_coeffs: sizes must be positive, got %d -> %d" % (in_size, out_size),
            ValueError)
    if in_size == out_size:
        return None
    scale = in_size / out_size
    fs = scale if scale > 1.0 else 1.0
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[xx] = (xmin, xmax - xmin)
        k[xx, :len(w)] = [int(v * one + 0.5) for v in w]
    return bounds, k, ksize


def validate_table(table, in_size, out_size):
    """What the kernel relies on (include/upk.h): xmin >= 0, 1 <= n <= ksize, xmin + n <= in_size; the weights are
    non-negative and sum to 2^22 within n, so that an accumulator stays below 2^31."""
    bounds, k, ksize = table
    require(bounds.shape == (out_size, 2) and k.shape == (out_size, ksize) and ksize >= 1, "resample table of the wrong shape",
            ValueError)
    lo, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    require(bool((lo >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (lo + n <= in_size).all()),
            "resample table leaves the %d-sample axis" % in_size, ValueError)
    require(bool((k >= 0).all() and (np.abs(k.sum(1, dtype=np.int64) - (1 << PRECISION_BITS)) <= n).all()),
            "resample weights do not sum to 2^22", ValueError)


def device_coeffs(device, in_size, out_size):
    """resample_coeffs on `device` (validated, uploaded once per (device, in, out)); None for a skipped pass.
    The first use of a size pair builds the table on the host and uploads it from pageable memory, which a stream that
    is being captured into a graph does not allow: call this (or resize_u8 / lr_transform once) for the sizes in use
    BEFORE a capture begins; afterwards the calls only launch.  The cache keeps one entry of a few KB per size pair for
    the life of the process and is never evicted: the callers here use one or two pairs per model."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(in_size), int(out_size))
    if key not in _tables:
        t = resample_coeffs(in_size, out_size)
        if t is not None:
            validate_table(t, int(in_size), int(out_size))
            with _lib.host_io():
                t = (torch.from_numpy(t[0]).to(device), torch.from_numpy(t[1]).to(device), t[2])
        _tables[key] = t
    return _tables[key]


def _size(size):
    size = [int(v) for v in (size if np.ndim(size) else [size, size])]
    require(len(size) == 2 and size[0] >= 1 and size[1] >= 1, "size must be [h, w] with positive entries, got %r" % (size,),
            ValueError)
    return size


def _pictures(pictures):
    """uint8 [B, H, W, 3] on the device, pixels dense inside a row (any row pitch / sample stride)."""
    if isinstance(pictures, np.ndarray):
        pictures = torch.from_numpy(np.ascontiguousarray(pictures))
    require(torch.is_tensor(pictures), "pictures must be a uint8 [B, H, W, 3] tensor or array, got %s" % type(pictures).__name__,
            TypeError)
    require(pictures.dtype == torch.uint8, "pictures must be uint8, got %s" % pictures.dtype, TypeError)
    require(pictures.dim() == 4, "pictures must be [B, H, W, 3], got %s" % (tuple(pictures.shape),), ValueError)
    require(pictures.shape[3] == 3, "3-channel pictures only, got %s" % (tuple(pictures.shape),), ValueError)
    require(min(pictures.shape[:3]) >= 1, "pictures must not be empty, got %s" % (tuple(pictures.shape),), ValueError)
    if not pictures.is_cuda:
        require(torch.cuda.is_available(), "the resize runs on the MI355X (upk_resize_bilinear_u8): no GPU is visible and "
                "there is no CPU fallback for the HIP path", RuntimeError)
        with _lib.host_io():
            pictures = pictures.contiguous().cuda()
    if pictures.stride(3) != 1 or pictures.stride(2) != 3 or pictures.stride(1) < 0 or pictures.stride(0) < 0:
        pictures = pictures.contiguous()
    return pictures


def _launch(pictures, size, pad, want_u8, want_f32, out_u8=None):
    oh, ow = _size(size)
    require(len(pad) == 2, "pad must be (pad_x, pad_y), got %r" % (pad,), ValueError)
    px, py = int(pad[0]), int(pad[1])
    require(px >= 0 and py >= 0, "pad must not be negative, got %r" % (pad,), ValueError)
    src = _pictures(pictures)
    b, h, w = (int(v) for v in src.shape[:3])
    dev = src.device
    xtab = device_coeffs(dev, w + 2 * px, ow)
    ytab = device_coeffs(dev, h + 2 * py, oh)
    u8 = torch.empty((b, oh, ow, 3), dtype=torch.uint8, device=dev) if want_u8 else out_u8
    if u8 is not None:
        require(torch.is_tensor(u8) and u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (b, oh, ow, 3) and
                u8.stride(3) == 1 and u8.stride(2) == 3, "out_u8 must be a uint8 device tensor [%d, %d, %d, 3] with dense "
                "pixels inside a row" % (b, oh, ow), ValueError)
    nchw = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=dev) if want_f32 else None
    nhwc = torch.empty((b, oh, ow, 3), dtype=torch.float32, device=dev) if want_f32 else None
    _lib.get_context(dev).resize_bilinear(src, b, h, w, src.stride(1), src.stride(0), px, py, oh, ow, xtab, ytab,
                                          u8, 0 if u8 is None else u8.stride(1), 0 if u8 is None else u8.stride(0),
                                          nchw, nhwc)
    return u8, nchw, nhwc


def resize_u8(pictures, size, pad=(0, 0)):
    """T.Pad(pad, padding_mode='edge') then T.Resize(size, BILINEAR) on PIL pictures, on the device: uint8 [B, H, W, 3]
    (a device tensor, read in place whatever its row pitch and sample stride; a host tensor or array is uploaded) ->
    uint8 device tensor [B, oh, ow, 3], byte for byte Pillow's.  size = [oh, ow]; pad = (pad_x, pad_y), torchvision's
    2-tuple order.  One launch on the current stream."""
    return _launch(pictures, size, pad, True, False)[0]


def lr_transform(pictures, size, pad=(0, 0), out_u8=None):
    """The reference's lr_transform: (lr [B, 3, oh, ow] fp32, lr_image [B, oh, ow, 3] fp32) on the device, the `lr` and
    `lr_image` entries of DeepFashionSuperResSampling / DeepFashionSuperRes, both written by the same launch:
    ToTensor and x * 2. - 1. of the resized bytes, t = fl(fl(u / 255) * 2 - 1).  With `size` equal to the padded size
    both passes are skipped and lr_image is the reference's image_transform (ToTensor, x * 2 - 1, HWC).
    out_u8: optionally a uint8 device tensor [B, oh, ow, 3] (any row pitch / sample stride) that receives the resized
    bytes from the same launch."""
    _, nchw, nhwc = _launch(pictures, size, pad, False, True, out_u8)
    return nchw, nhwc
