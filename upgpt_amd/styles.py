"""The style crops of a source picture: batch['styles'], the [9, 3, 224, 224] input of mix_style and
FrozenClipImageEmbedder2.  The reference cuts them on the host (ldm/data/segm_utils.py: Segmenter.forward over a
human-parsing label map, one Pillow / torchvision round per group), stores them as <style>.jpg and reads those files
back through clip_transform (deepfashion_inshop.py:128-133, 208-216).

Here the chain label map -> boxes -> coefficients -> cut, pad, resize, centre crop, CLIP normalisation is two launches
on the device (upk_segm_boxes_u8, upk_style_crops_u8; include/upk.h) with no device-to-host copy in it:
the second launch reads every group's box from device memory, so the pair can be captured in a graph and replayed on
new label maps.  The bytes equal the reference's arithmetic (Pillow's integer resampling) bit for bit, with two stated
differences: no JPEG round trip in between, and the background fill colour is the exact floor(S_c / N).
No CPU fallback: without a GPU these functions raise."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._check import require
from .inference import CLIP_MEAN, CLIP_STD, style_names

SIZE = 224           # T.Resize(224), T.CenterCrop(224)
FACE_MAX_ROWS = 128  # a `face` cut of more rows is dropped (segm_utils.py:116)
COEFF_TAPS = 16      # upk_style_crops_u8's coeff_out record: (first tap, taps, k[16])


class Segmenter:
    """A label list and its style groups (segm_utils.Segmenter): `groups` maps a style name to the label names it is
    made of, in the order the reference produces them.  The group named 'background' is filled instead of cut, the
    group named 'face' keeps the picture's own background and is dropped above 128 rows; every other group is masked."""

    def __init__(self, label_names, groups):
        self.label_names = list(label_names)
        self.label2id = {name: i for i, name in enumerate(self.label_names)}
        self.groups = OrderedDict((k, tuple(v)) for k, v in groups.items())
        self.names = list(self.groups)
        self.group_ids = OrderedDict((k, tuple(self.label2id[l] for l in v)) for k, v in self.groups.items())
        require(len(self.label_names) <= 256 and 1 <= len(self.names) <= 32, "a segmenter has up to 256 labels and 32 groups",
                ValueError)
        self.label_groups = [0] * 256  # label -> bitmask of the groups it belongs to
        for g, ids in enumerate(self.group_ids.values()):
            for i in ids:
                self.label_groups[i] |= 1 << g
        self.group_flags = [_lib.STYLE_FILL if k == 'background' else
                            (FACE_MAX_ROWS << 8) if k == 'face' else _lib.STYLE_MASK for k in self.names]

    def slot_groups(self, slots):
        """Group index per slot name, -1 for a name this segmenter does not produce."""
        return [self.names.index(s) if s in self.names else -1 for s in slots]


LIP = Segmenter(
    ['background', 'hat', 'hair', 'glove', 'eyeglass', 'top', 'dress', 'coat', 'socks', 'pants', 'jumpsuits', 'scarf', 'skirt',
     'face', 'left-arm', 'right-arm', 'left-leg', 'right-leg', 'left-shoe', 'right-shoe'],
    OrderedDict([('face', ['eyeglass', 'face']), ('background', ['background']), ('hair', ['hair']), ('headwear', ['hat']),
                 ('top', ['top', 'dress', 'jumpsuits', 'scarf']), ('bottom', ['skirt', 'dress', 'pants', 'jumpsuits']),
                 ('shoes', ['left-shoe', 'right-shoe', 'socks']), ('outer', ['coat'])]))
DEEPFASHION_MM = Segmenter(
    ['background', 'top', 'outer', 'skirt', 'dress', 'pants', 'leggings', 'headwear', 'eyeglass', 'neckwear', 'belt', 'footwear',
     'bag', 'hair', 'face', 'skin', 'ring', 'wrist wearing', 'socks', 'gloves', 'necklace', 'rompers', 'earrings', 'tie'],
    OrderedDict([('face', ['eyeglass', 'face']), ('background', ['background']), ('skin', ['skin'])]))
SEGMENTERS = {'lip': LIP, 'mm': DEEPFASHION_MM}


def LipSegmenter():
    """segm_utils.LipSegmenter: the LIP label set and its eight style groups."""
    return LIP


def DeepfashionMMSegmenter():
    """segm_utils.DeepfashionMMSegmenter: the DeepFashion-MultiModal label set (face, background, skin)."""
    return DEEPFASHION_MM


def get_segmenter(segmenter):
    if isinstance(segmenter, Segmenter):
        return segmenter
    require(isinstance(segmenter, str) and segmenter in SEGMENTERS, "segmenter must be a Segmenter or one of %s, got %r" % (
        sorted(SEGMENTERS), segmenter), ValueError)
    return SEGMENTERS[segmenter]


def _maps(pictures, segm):
    """(pictures uint8 [B, H, W, 3], label maps uint8 [B, H, W]) on one device, dense inside a row (any row pitch and
    sample stride).  Everything that can be refused on the host is refused before anything is uploaded."""
    out = []
    for name, t, dims in (("pictures", pictures, 4), ("segm", segm, 3)):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t) if t.flags.writeable else np.array(t))  # (PIL's arrays are read-only)
        require(torch.is_tensor(t), "%s must be a uint8 tensor or array, got %s" % (name, type(t).__name__), TypeError)
        require(t.dtype == torch.uint8, "%s must be uint8, got %s" % (name, t.dtype), TypeError)
        require(t.dim() == dims, "%s must be %s, got %s" % (name, "[B, H, W, 3]" if dims == 4 else "[B, H, W]", tuple(t.shape)),
                ValueError)
        out.append(t)
    pictures, segm = out
    require(pictures.shape[3] == 3, "3-channel pictures only, got %s" % (tuple(pictures.shape),), ValueError)
    require(min(pictures.shape[:3]) >= 1, "pictures must not be empty, got %s" % (tuple(pictures.shape),), ValueError)
    require(tuple(segm.shape) == tuple(pictures.shape[:3]), "segm %s does not match pictures %s" % (
        tuple(segm.shape), tuple(pictures.shape)), ValueError)
    if not (pictures.is_cuda and segm.is_cuda):
        require(torch.cuda.is_available(), "the style crops are made on the MI355X (upk_segm_boxes_u8, upk_style_crops_u8): "
                "no GPU is visible and there is no CPU fallback for the HIP path", RuntimeError)
    dev = pictures.device if pictures.is_cuda else segm.device if segm.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with _lib.host_io():
        pictures, segm = (t if t.is_cuda else t.contiguous().to(dev) for t in (pictures, segm))
    require(pictures.device == segm.device, "pictures and segm are on different devices", ValueError)
    if pictures.stride(3) != 1 or pictures.stride(2) != 3 or pictures.stride(1) < 3 * pictures.shape[2] or pictures.stride(0) < 0:
        pictures = pictures.contiguous()
    if segm.stride(2) != 1 or segm.stride(1) < segm.shape[2] or segm.stride(0) < 0:
        segm = segm.contiguous()
    return pictures, segm


def _boxes(ctx, pictures, segm, seg):
    b, h, w = (int(v) for v in segm.shape)
    boxes = torch.empty((b, len(seg.names), 8), dtype=torch.int32, device=segm.device)
    ctx.segm_boxes(segm, segm.stride(1), segm.stride(0), pictures, pictures.stride(1), pictures.stride(0), b, h, w,
                   seg.label_groups, len(seg.names), boxes)
    return boxes


def style_boxes(pictures, segm, segmenter='lip'):
    """int32 device tensor [B, G, 8] = left, right, top, bottom, N, S_r, S_g, S_b per group of the segmenter, in its
    group order: the reference's get_mask_range with margin 0 (right / bottom are the INDEX of the last masked column /
    row; 0, W, 0, H without a masked pixel), the mask count and the integer channel sums over the mask.  One launch."""
    seg = get_segmenter(segmenter)
    pictures, segm = _maps(pictures, segm)
    return _boxes(_lib.get_context(segm.device), pictures, segm, seg)


def style_crops(pictures, segm, segmenter='lip', slots=style_names, out_u8=False):
    """Segmenter.forward and clip_transform for a batch: pictures uint8 [B, H, W, 3] and label maps uint8 [B, H, W]
    (device tensors are read in place whatever their row pitch and sample stride; host tensors / arrays are uploaded)
    -> (styles fp32 [B, len(slots), 3, 224, 224] CLIP-normalised, valid int32 [B, len(slots)], the crops' bytes uint8
    [B, len(slots), 224, 224, 3] or None), all on the device.  A slot whose name the segmenter does not produce
    ('accesories') is empty; an empty slot and an invalid crop (an empty cut, a face of more than 128 rows, a
    background without a pixel) hold clip_norm(0) and valid 0.  Two launches on the current stream, no synchronisation,
    nothing crosses to the host."""
    seg = get_segmenter(segmenter)
    slots = list(slots)
    require(1 <= len(slots) <= 32 and all(isinstance(s, str) for s in slots), "slots must be 1 .. 32 style names, got %r" % (
        slots,), ValueError)
    pictures, segm = _maps(pictures, segm)
    b, h, w = (int(v) for v in segm.shape)
    dev = segm.device
    ctx = _lib.get_context(dev)
    boxes = _boxes(ctx, pictures, segm, seg)
    styles = torch.empty((b, len(slots), 3, SIZE, SIZE), dtype=torch.float32, device=dev)
    valid = torch.empty((b, len(slots)), dtype=torch.int32, device=dev)
    u8 = torch.empty((b, len(slots), SIZE, SIZE, 3), dtype=torch.uint8, device=dev) if out_u8 else None
    ctx.style_crops(pictures, pictures.stride(1), pictures.stride(0), segm, segm.stride(1), segm.stride(0), b, h, w,
                    seg.label_groups, len(seg.names), boxes, seg.group_flags, seg.slot_groups(slots),
                    list(CLIP_MEAN) + list(CLIP_STD), u8, styles, valid)
    return styles, valid, u8
