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


# ---- pose interpolation: the conditioning of a frame sequence and the demo's pose folders

def check_alphas(alphas):
    """`alphas` as a float64 array [n]; ValueError for an empty sequence, a NaN or a value outside [0, 1] (outside it the
    reference's negative slice bounds wrap around, which is not worth reproducing)."""
    try:
        a = np.array(alphas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("alphas must be a sequence of floats, got %r" % (alphas,))
    require(a.size >= 1, "alphas must not be empty", ValueError)
    require(not np.isnan(a).any(), "alphas holds a NaN", ValueError)
    require(bool((a >= 0.0).all() and (a <= 1.0).all()), lambda: "alphas must lie in [0, 1], got %s" % (a.tolist(),), ValueError)
    return a


def _pose_f32(t, name, tail_dims):
    """fp32 tensor whose leading axes are all 1 and whose last `tail_dims` axes are the payload, dense; never a view the
    caller's tensor could be written through."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t))
    require(torch.is_tensor(t), "%s must be an fp32 tensor or array, got %s" % (name, type(t).__name__), TypeError)
    require(t.dtype == torch.float32, "%s must be fp32, got %s" % (name, t.dtype), TypeError)
    require(t.dim() >= tail_dims and t.numel() >= 1 and all(int(s) == 1 for s in t.shape[:t.dim() - tail_dims]),
            "%s must be %s with leading axes of 1, got %s" % (name, "[1, h, w]" if tail_dims == 2 else "[1, d]", tuple(t.shape)),
            ValueError)
    return t.reshape(t.shape[t.dim() - tail_dims:]).contiguous()


def interp_pose(src_mask, dst_mask, src_smpl, dst_smpl, alphas, return_boxes=False):
    """The conditioning of the n = len(alphas) frames of a pose interpolation, the loop of app.py:298-300, in ONE
    upk_pose_interp_f32 launch on the current stream: {'smpl': fp32 [n, 1, d], 'person_mask': fp32 [n, 1, h, w]} on the
    device, frame i being alphas[i] of the source and 1 - alphas[i] of the destination — bit for bit torch's
    `alpha * smpl_src + (1 - alpha) * smpl_dst` and inference.interp_mask(src_mask, dst_mask, alpha) with a numpy float64
    alpha (include/upk.h states the arithmetic and the occupancy precondition on the masks).
    src_mask, dst_mask: fp32 [1, h, w] of one size; src_smpl, dst_smpl: fp32 [1, d]; host tensors / arrays are uploaded,
    device tensors are read in place, none is modified.  alphas: any float sequence, taken as float64 and uploaded once;
    ValueError for an empty one, a NaN or a value outside [0, 1].
    A HOST mask without foreground (no element other than -1 and 0) raises ValueError before anything is uploaded, where
    the reference raises IndexError; a DEVICE mask is not looked at (that would synchronise): the kernel then gives every
    frame an all-background mask and boxes of -1.
    return_boxes=True adds 'boxes': int32 [n + 2, 4] = (r0, r1, c0, c1) on the device, rows 0 and 1 the source's and the
    destination's box, row 2 + i frame i's.  No CPU fallback: without a GPU this raises."""
    a = check_alphas(alphas)
    sm, dm = _pose_f32(src_mask, "src_mask", 2), _pose_f32(dst_mask, "dst_mask", 2)
    ss, ds = _pose_f32(src_smpl, "src_smpl", 1), _pose_f32(dst_smpl, "dst_smpl", 1)
    require(sm.shape == dm.shape, "src_mask %s and dst_mask %s differ in size" % (tuple(sm.shape), tuple(dm.shape)), ValueError)
    require(ss.shape == ds.shape, "src_smpl %s and dst_smpl %s differ in size" % (tuple(ss.shape), tuple(ds.shape)), ValueError)
    for name, m in (("src_mask", sm), ("dst_mask", dm)):
        if not m.is_cuda:
            require(bool(((m != -1.0) & (m != 0.0)).any()), "%s has no foreground: its bounding box is undefined" % name, ValueError)
    dev = next((t.device for t in (sm, dm, ss, ds) if t.is_cuda), None)
    if dev is None:
        require(torch.cuda.is_available(), "the frames are built on the MI355X (upk_pose_interp_f32): no GPU is visible and "
                "there is no CPU fallback for the HIP path", RuntimeError)
        dev = torch.device("cuda", torch.cuda.current_device())
    with _lib.host_io():
        sm, dm, ss, ds = (t.to(dev) for t in (sm, dm, ss, ds))
        at = torch.from_numpy(a).to(dev)
    n, (h, w), d = int(a.size), (int(v) for v in sm.shape), int(ss.shape[0])
    mask = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
    smpl = torch.empty((n, 1, d), dtype=torch.float32, device=dev)
    boxes = torch.empty((n + 2, 4), dtype=torch.int32, device=dev) if return_boxes else None
    with torch.cuda.device(dev):
        _lib.get_context(dev).pose_interp(sm, dm, h, w, ss, ds, d, at, n, mask, smpl, boxes)
    out = {'smpl': smpl, 'person_mask': mask}
    if return_boxes:
        out['boxes'] = boxes
    return out


def read_pose_folder(folder):
    """The host part of load_pose: (smpl fp32 array [1, 85] = pose | betas | camera, picture uint8 [H, W, 3], mask uint8
    [H, W], the palette indices of the mode-P PNG) of a pose folder of the demo.  A folder without exactly one .p, one
    .jpg and one .png, a pickle of another structure or an unreadable picture raises ValueError."""
    import pickle
    from pathlib import Path

    from PIL import Image
    folder = Path(folder)
    require(folder.is_dir(), "load_pose: %s is not a directory" % folder, ValueError)
    files = {}
    for ext in (".p", ".jpg", ".png"):
        found = sorted(f for f in folder.iterdir() if f.is_file() and f.suffix == ext)
        require(len(found) == 1, "load_pose: %s holds %d %s files, expected exactly one" % (folder, len(found), ext), ValueError)
        files[ext] = found[0]
    try:
        with open(str(files[".p"]), "rb") as f:
            first = pickle.load(f)[0]
        pose, betas = np.asarray(first['pred_body_pose']), np.asarray(first['pred_betas'])
        smpl = np.concatenate((pose, betas, np.expand_dims(np.asarray(first['pred_camera']), 0)), axis=1)
    except Exception as e:
        raise ValueError("load_pose: %s is not a list whose first entry holds pred_body_pose (1, 72), pred_betas (1, 10) "
                         "and pred_camera (3,): %s" % (files[".p"], e))
    require(smpl.ndim == 2 and smpl.shape[0] == 1, "load_pose: %s gives an SMPL vector of shape %s" % (files[".p"], smpl.shape),
            ValueError)
    try:
        with Image.open(str(files[".jpg"])) as im:
            picture = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(str(files[".png"])) as im:
            mask = np.asarray(im, dtype=np.uint8)  # (mode P: the palette indices, what ToTensor reads)
    except Exception as e:
        raise ValueError("load_pose: cannot read the pictures of %s: %s" % (folder, e))
    require(mask.ndim == 2, "load_pose: %s is not a one-channel picture" % files[".png"], ValueError)
    return np.ascontiguousarray(smpl, dtype=np.float32), picture, mask


def load_pose(folder, mask_size=(32, 24), crop=(256, 192)):
    """The demo's load_smpl (app.py:115-143) of a pose folder (one .p, one .jpg, one .png):
    'smpl'         fp32 [1, 85] host tensor: pred_body_pose | pred_betas | pred_camera of the pickle's first entry
    'smpl_image'   uint8 [crop_h, crop_w, 3] host tensor: T.CenterCrop(crop) of the picture (the reference keeps the PIL
                   picture; a picture smaller than the crop raises ValueError instead of being zero-padded)
    'person_mask'  fp32 [1, h, w] on the device, mask_size = [h, w]: Pillow's NEAREST resize of the mode-P mask, ToTensor,
                   x * 2 - 1, values {-1, -0.99215686} — the loader's input_mask_type='mask' path (data.person_mask:
                   the same index tables, the same look-up table, one upk_cond_gather_u8 launch).
    The pickle is read with pickle and numpy only.  The dict goes into InferenceModel.create_batch / interpolate as it is."""
    from . import data
    from .evaluate import center_crop_window
    smpl, picture, mask = read_pose_folder(folder)
    top, left, ch, cw = center_crop_window(picture.shape[0], picture.shape[1], list(crop))
    person_mask = data.person_mask(mask[None], mask_size, 'mask')[0]
    return {'smpl': torch.from_numpy(smpl), 'smpl_image': torch.from_numpy(np.array(picture[top:top + ch, left:left + cw])),
            'person_mask': person_mask}
