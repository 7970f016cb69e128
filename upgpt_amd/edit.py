"""Region-locked editing: change one garment of a given photo and nothing else.

The sampling side was here already: AutoencoderKL.encode, the masked chain of the samplers (sample(mask=, x0=)),
upk_image_finish_u8.  This module adds the two per-pixel passes around it, one launch each (include/upk.h):

  region_mask   a human-parsing label map and a region name -> the dilated picture-resolution edit mask, the
                latent-resolution keep-mask the sampler takes and the number of edited cells (upk_region_mask_u8)
  composite     the generated picture blended into the original under the feathered mask, on the bytes
                (upk_composite_u8): every pixel farther than dilate + feather from the region is the input's, byte for byte

InferenceModel.edit_region (inference.py) strings them together.  No CPU fallback: without a GPU these functions raise."""
import numpy as np
import torch

from . import _lib
from ._check import require
from .styles import get_segmenter

MAX_DILATE = 32   # upk_region_mask_u8
MAX_FEATHER = 16  # upk_composite_u8
FACTORS = (1, 2, 4, 8, 16)
LABEL_PREFIX = "label:"


def region_labels(region, segmenter='lip'):
    """The label ids a region stands for, as a sorted tuple.  region: a name or an iterable of names; a name that is a
    group of the segmenter (styles.Segmenter.groups: 'top', 'bottom', 'hair', ...) expands to the group's labels,
    anything else must be a label name; 'label:top' forces the single label where a group has the same name (LIP's
    `top` group is top, dress, jumpsuits and scarf).  Unknown or empty: ValueError naming the valid groups and labels."""
    seg = get_segmenter(segmenter)
    names = [region] if isinstance(region, str) else list(region) if isinstance(region, (list, tuple, set, frozenset)) else None
    valid = lambda: "groups: %s; labels: %s (prefix %r forces a label)" % (", ".join(seg.names), ", ".join(seg.label_names), LABEL_PREFIX)
    require(names is not None and all(isinstance(n, str) for n in names),
            lambda: "region must be a name or a list of names, got %r (%s)" % (region, valid()), ValueError)
    require(len(names) > 0, lambda: "region is empty (%s)" % valid(), ValueError)
    ids = set()
    for name in names:
        if name.startswith(LABEL_PREFIX):
            label = name[len(LABEL_PREFIX):]
            require(label in seg.label2id, lambda: "unknown label %r in region %r (%s)" % (label, name, valid()), ValueError)
            ids.add(seg.label2id[label])
        elif name in seg.group_ids:
            ids.update(seg.group_ids[name])
        else:
            require(name in seg.label2id, lambda: "unknown region %r (%s)" % (name, valid()), ValueError)
            ids.add(seg.label2id[name])
    return tuple(sorted(ids))


def _u8(name, t, shape_text, dims):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t) if t.flags.writeable else np.array(t))  # (PIL's arrays are read-only)
    require(torch.is_tensor(t), lambda: "%s must be a uint8 tensor or array, got %s" % (name, type(t).__name__), TypeError)
    require(t.dtype == torch.uint8, lambda: "%s must be uint8, got %s" % (name, t.dtype), TypeError)
    require(t.dim() == dims, lambda: "%s must be %s, got %s" % (name, shape_text, tuple(t.shape)), ValueError)
    require(min(t.shape) >= 1, lambda: "%s must not be empty, got %s" % (name, tuple(t.shape)), ValueError)
    return t


def _on_device(tensors, what):
    """Host tensors are uploaded (under host_io) to the device of the first device tensor, else the current one."""
    if not all(t.is_cuda for t in tensors):
        require(torch.cuda.is_available(), "%s: no GPU is visible and there is no CPU fallback for the HIP path" % what, RuntimeError)
    dev = next((t.device for t in tensors if t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    with _lib.host_io():
        tensors = [t if t.is_cuda else t.contiguous().to(dev) for t in tensors]
    require(all(t.device == dev for t in tensors), "the inputs are on different devices", ValueError)
    return tensors


def _rows(t, px):
    """A [B, H, W(, 3)] uint8 device tensor the kernels read in place: px bytes per pixel, dense inside a row."""
    ok = t.stride(2) == px and t.stride(1) >= px * t.shape[2] and t.stride(0) >= 0 and (px == 1 or t.stride(3) == 1)
    return t if ok else t.contiguous()


def region_mask(segm, region, segmenter='lip', dilate=8, factor=8):
    """The edit mask of a region: label maps uint8 [B, H, W] (a device tensor is read in place whatever its row pitch and
    sample stride; a host tensor / array is uploaded) -> (mask_u8 uint8 [B, H, W]: 255 where a pixel lies within `dilate`
    (Chebyshev) of a pixel of the region, else 0; keep fp32 [B, 1, H / factor, W / factor]: 0.0 for a latent cell whose
    factor x factor block holds a mask pixel, else 1.0, the samplers' `mask=`; cells int32 [B]: the edited cells), all on
    the device.  region / segmenter: see region_labels.  One launch on the current stream, no synchronisation, nothing
    crosses to the host."""
    labels = region_labels(region, segmenter)
    segm = _u8("segm", segm, "[B, H, W]", 3)
    b, h, w = (int(v) for v in segm.shape)
    dilate, factor = int(dilate), int(factor)
    require(0 <= dilate <= MAX_DILATE, lambda: "dilate must be 0 .. %d, got %d" % (MAX_DILATE, dilate), ValueError)
    require(factor in FACTORS, lambda: "factor must be one of %s, got %d" % (FACTORS, factor), ValueError)
    require(h % factor == 0 and w % factor == 0, lambda: "a %d x %d map is not a multiple of factor %d" % (h, w, factor), ValueError)
    segm = _rows(_on_device([segm], "the edit mask is made on the MI355X (upk_region_mask_u8)")[0], 1)
    dev = segm.device
    mask = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    keep = torch.empty((b, 1, h // factor, w // factor), dtype=torch.float32, device=dev)
    cells = torch.empty((b,), dtype=torch.int32, device=dev)
    _lib.get_context(dev).region_mask(segm, segm.stride(1), segm.stride(0), b, h, w, labels, dilate, factor, mask, mask.stride(1),
                                      mask.stride(0), keep, cells)
    return mask, keep, cells


def composite(orig, gen, mask_u8, feather=4, return_alpha=False):
    """The generated pictures blended into the originals: orig, gen uint8 [B, H, W, 3] and mask_u8 uint8 [B, H, W] (device
    tensors are read in place, host tensors / arrays are uploaded) -> uint8 [B, H, W, 3] on the device, with
    return_alpha=True (out, alpha uint8 [B, H, W]).  alpha is the (2 feather + 1)^2 box mean of the mask (edges
    replicated) scaled to 0 .. 255; out = (alpha gen + (255 - alpha) orig + 127) / 255 in integers: alpha 0 returns the
    original byte, alpha 255 the generated one.  One launch on the current stream."""
    orig, gen = _u8("orig", orig, "[B, H, W, 3]", 4), _u8("gen", gen, "[B, H, W, 3]", 4)
    mask_u8 = _u8("mask_u8", mask_u8, "[B, H, W]", 3)
    require(orig.shape[3] == 3, lambda: "3-channel pictures only, got %s" % (tuple(orig.shape),), ValueError)
    require(gen.shape == orig.shape and tuple(mask_u8.shape) == tuple(orig.shape[:3]), lambda: "orig %s, gen %s and mask_u8 %s do not match" % (
        tuple(orig.shape), tuple(gen.shape), tuple(mask_u8.shape)), ValueError)
    feather = int(feather)
    require(0 <= feather <= MAX_FEATHER, lambda: "feather must be 0 .. %d, got %d" % (MAX_FEATHER, feather), ValueError)
    orig, gen, mask_u8 = _on_device([orig, gen, mask_u8], "the composite is made on the MI355X (upk_composite_u8)")
    orig, gen, mask_u8 = _rows(orig, 3), _rows(gen, 3), _rows(mask_u8, 1)
    b, h, w = (int(v) for v in mask_u8.shape)
    dev = orig.device
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
    alpha = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if return_alpha else None
    _lib.get_context(dev).composite(orig, orig.stride(1), orig.stride(0), gen, gen.stride(1), gen.stride(0), mask_u8,
                                    mask_u8.stride(1), mask_u8.stride(0), b, h, w, feather, out, out.stride(1), out.stride(0),
                                    alpha, 0 if alpha is None else alpha.stride(1), 0 if alpha is None else alpha.stride(0))
    return (out, alpha) if return_alpha else out
