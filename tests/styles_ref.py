"""numpy + Pillow + torch-CPU restatement of the reference's style crops: Segmenter.forward (ldm/data/segm_utils.py:42-150,
the LIP and DeepFashion-MultiModal tables of :152-228) followed by what its consumer does to a crop (clip_transform,
deepfashion_inshop.py:128-133, 208-216).  torchvision is not needed: T.ToPILImage on fl(u / 255) returns u for every byte
(tests/test_styles_host.py checks all 256), T.Resize on a PIL picture is Pillow's integer resampling (tests/resize_ref.py,
pinned to PIL.Image.resize), T.CenterCrop and T.Normalize are restated here.

Two deliberate differences from the reference's file flow, both selectable / visible here:
  * the crop's bytes go straight on (the reference stores every crop as a JPEG and decodes it again);
  * fill='exact' takes the background fill colour as floor(S_c / N); fill='float32' is the reference's own expression
    (a float32 mean of u / 255 values, mul(255).byte()), which differs only where rounding noise decides.
The fixtures of the GPU tests live here too, so the host tests can assert their properties without a device."""
from collections import OrderedDict

import numpy as np
import torch

import resize_ref as rr

SIZE = 224
STYLE_NAMES = ['face', 'hair', 'headwear', 'background', 'top', 'outer', 'bottom', 'shoes', 'accesories']
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

LIP_LABELS = ['background', 'hat', 'hair', 'glove', 'eyeglass', 'top', 'dress', 'coat', 'socks', 'pants', 'jumpsuits', 'scarf',
              'skirt', 'face', 'left-arm', 'right-arm', 'left-leg', 'right-leg', 'left-shoe', 'right-shoe']
LIP_GROUPS = OrderedDict([('face', ['eyeglass', 'face']), ('background', ['background']), ('hair', ['hair']),
                          ('headwear', ['hat']), ('top', ['top', 'dress', 'jumpsuits', 'scarf']),
                          ('bottom', ['skirt', 'dress', 'pants', 'jumpsuits']),
                          ('shoes', ['left-shoe', 'right-shoe', 'socks']), ('outer', ['coat'])])
MM_LABELS = ['background', 'top', 'outer', 'skirt', 'dress', 'pants', 'leggings', 'headwear', 'eyeglass', 'neckwear', 'belt',
             'footwear', 'bag', 'hair', 'face', 'skin', 'ring', 'wrist wearing', 'socks', 'gloves', 'necklace', 'rompers',
             'earrings', 'tie']
MM_GROUPS = OrderedDict([('face', ['eyeglass', 'face']), ('background', ['background']), ('skin', ['skin'])])
TABLES = {'lip': (LIP_LABELS, LIP_GROUPS), 'mm': (MM_LABELS, MM_GROUPS)}


def group_ids(segmenter):
    """name -> label ids, in the reference's group order."""
    labels, groups = TABLES[segmenter]
    return OrderedDict((k, [labels.index(l) for l in v]) for k, v in groups.items())


def binary_mask(segm, ids):
    mask = np.zeros(segm.shape, dtype=bool)
    for i in ids:
        mask |= segm == i
    return mask


def mask_range(mask):
    """get_mask_range with margin 0: (left, right, top, bottom); right / bottom are the INDEX of the last masked column /
    row; 0, W, 0, H for an empty mask."""
    h, w = mask.shape
    cols = np.nonzero(mask.sum(0))[0]
    rows = np.nonzero(mask.sum(1))[0]
    if cols.size == 0:
        return 0, w, 0, h
    return int(cols[0]), int(cols[-1]), int(rows[0]), int(rows[-1])


def box_record(picture, mask):
    """left, right, top, bottom, N, S_r, S_g, S_b."""
    sums = [int(picture[..., c][mask].astype(np.int64).sum()) for c in range(3)]
    return list(mask_range(mask)) + [int(mask.sum())] + sums


def boxes(pictures, segm, segmenter):
    """int32 [B, G, 8]."""
    ids = group_ids(segmenter)
    return np.array([[box_record(p, binary_mask(s, v)) for v in ids.values()] for p, s in zip(pictures, segm)], dtype=np.int32)


def pad_amounts(ch, cw):
    """(columns added left and right, rows added above and below) for a ch x cw cut: p = (ch - cw) // 2, floor division."""
    p = (ch - cw) // 2
    return (p, 0) if p > 0 else (0, -p) if p < 0 else (0, 0)


def resized_size(h, w):
    """T.Resize(224) on an h x w picture: (oh, ow)."""
    if w <= h:
        return (h, w) if w == SIZE else (int(SIZE * h / w), SIZE)
    return (h, w) if h == SIZE else (SIZE, int(SIZE * w / h))


def center_offset(n):
    """T.CenterCrop(224) on an axis of n >= 224 samples (Python's round: half to even)."""
    return int(round((n - SIZE) / 2.0))


def image_transform(u8):
    """T.ToPILImage, T.Resize(224), T.CenterCrop((224, 224)) on the bytes [h, w, 3] -> [224, 224, 3]."""
    oh, ow = resized_size(*u8.shape[:2])
    x = rr.resize(u8, (oh, ow)) if (oh, ow) != u8.shape[:2] else u8
    t, l = center_offset(oh), center_offset(ow)
    return np.ascontiguousarray(x[t:t + SIZE, l:l + SIZE])


def fill_colour(picture, mask, fill):
    """The background's fill bytes per channel, or None when the mask is empty (the reference's mean is NaN there)."""
    if not mask.any():
        return None
    if fill == 'exact':
        return [int(picture[..., c][mask].astype(np.int64).sum()) // int(mask.sum()) for c in range(3)]
    assert fill == 'float32'
    img = torch.from_numpy(np.ascontiguousarray(picture.transpose(2, 0, 1))).to(torch.float32).div(255)  # T.ToTensor
    m = torch.from_numpy(mask)
    return [int(torch.masked_select(img[c], m).mean().mul(255).byte()) for c in range(3)]


def crop(picture, mask, name, fill='exact'):
    """Segmenter.crop for the group `name` -> (bytes [224, 224, 3], valid).  valid is geometric: a non-empty cut and the
    face rule; a valid cut that is black everywhere gives the zero bytes the reference returns for it."""
    zero = np.zeros((SIZE, SIZE, 3), dtype=np.uint8)
    if name == 'background':
        colour = fill_colour(picture, mask, fill)
        if colour is None:
            return zero, 0
        return image_transform(np.where(mask[..., None], picture, np.array(colour, dtype=np.uint8))), 1
    left, right, top, bottom = mask_range(mask)
    content = picture * mask[..., None] if name != 'face' else picture
    cut = content[top:bottom, left:right]
    ch, cw = cut.shape[:2]
    if ch <= 0 or cw <= 0 or (name == 'face' and ch > 128):
        return zero, 0
    if not cut.any():  # (the reference returns zeros for a cut that sums to zero; resampling zeros gives the same bytes)
        return zero, 1
    px, py = pad_amounts(ch, cw)
    return image_transform(np.pad(cut, ((py, py), (px, px), (0, 0)))), 1


def clip_norm(u8):
    """T.ToTensor + T.Normalize on bytes [..., 224, 224, 3] -> fp32 [..., 3, 224, 224]: fl(fl(fl(u / 255) - mean) / std)."""
    t = np.moveaxis(u8, -1, -3).astype(np.float32) / np.float32(255.0)
    mean = np.array(MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.array(STD, dtype=np.float32).reshape(3, 1, 1)
    return np.ascontiguousarray((t - mean) / std)


def forward(picture, segm, segmenter, fill='exact'):
    """Segmenter.forward: name -> (bytes, valid) in the reference's group order."""
    return OrderedDict((k, crop(picture, binary_mask(segm, v), k, fill)) for k, v in group_ids(segmenter).items())


def styles(pictures, segm, segmenter, slots=STYLE_NAMES, fill='exact'):
    """-> (styles fp32 [B, S, 3, 224, 224], valid int32 [B, S], bytes uint8 [B, S, 224, 224, 3]); a slot the segmenter does
    not produce is empty: zero bytes, valid 0."""
    zero = (np.zeros((SIZE, SIZE, 3), dtype=np.uint8), 0)
    per = [forward(p, s, segmenter, fill) for p, s in zip(pictures, segm)]
    u8 = np.stack([np.stack([f.get(k, zero)[0] for k in slots]) for f in per])
    valid = np.array([[f.get(k, zero)[1] for k in slots] for f in per], dtype=np.int32)
    return clip_norm(u8), valid, u8


def implied_sizes(box, name, h, w):
    """For a VALID crop: ((ph, oh, cy), (pw, ow, cx)), the padded size, the resized size and the centre offset per axis."""
    if name == 'background':
        ph, pw = h, w
    else:
        ch, cw = int(box[3] - box[2]), int(box[1] - box[0])
        px, py = pad_amounts(ch, cw)
        ph, pw = ch + 2 * py, cw + 2 * px
    oh, ow = resized_size(ph, pw)
    return (ph, oh, center_offset(oh)), (pw, ow, center_offset(ow))


# ---------------------------------------------------------------------------------------------------------------------
# fixtures of tests/test_styles_gpu.py (random bytes, label maps built by hand)

def random_pictures(b, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


def rect(segm, label, top, left, rows, cols):
    segm[top:top + rows, left:left + cols] = label


def lip_64x48():
    """B = 3.  A masked w x h block gives the cut (h - 1) x (w - 1).  Sample 0: face 10 x 6 (ch - cw = 4), hair 6 x 17 (-11),
    a one-row hat (invalid), top 16 x 11 (5), pants 8 x 16 (-8), a one-column shoe (invalid), a coat of 3 x 2 pixels: the
    two-by-one cut that becomes 448 x 224.  Sample 1: a dress (top AND bottom) touching all four borders, everything else
    but the background empty.  Sample 2: ch - cw of 1, -1, -3, 2, 0 and 3."""
    L = LIP_LABELS.index
    segm = np.zeros((3, 64, 48), dtype=np.uint8)
    s = segm[0]
    rect(s, L('face'), 2, 5, 11, 7)
    rect(s, L('eyeglass'), 5, 6, 2, 5)
    rect(s, L('hair'), 14, 3, 7, 18)
    rect(s, L('hat'), 22, 4, 1, 7)
    rect(s, L('top'), 24, 10, 17, 12)
    rect(s, L('pants'), 42, 20, 9, 17)
    rect(s, L('left-shoe'), 52, 40, 9, 1)
    rect(s, L('coat'), 60, 44, 3, 2)
    s = segm[1]
    rect(s, L('dress'), 20, 10, 30, 25)
    s[0, 10] = s[63, 20] = s[30, 0] = s[31, 47] = L('dress')
    s = segm[2]
    rect(s, L('face'), 1, 1, 9, 8)       # 8 x 7: 1
    rect(s, L('hair'), 1, 12, 6, 7)      # 5 x 6: -1
    rect(s, L('scarf'), 12, 2, 5, 8)     # 4 x 7: -3
    rect(s, L('skirt'), 20, 4, 13, 11)   # 12 x 10: 2
    rect(s, L('socks'), 36, 8, 10, 10)   # 9 x 9: 0
    rect(s, L('coat'), 48, 20, 14, 11)   # 13 x 10: 3
    return random_pictures(3, 64, 48, 6448), segm


def mm_37x29():
    """B = 2, odd sizes: face (with an eyeglass strip), skin in two separate blobs, the rest background."""
    L = MM_LABELS.index
    segm = np.zeros((2, 37, 29), dtype=np.uint8)
    rect(segm[0], L('face'), 3, 9, 10, 9)
    rect(segm[0], L('eyeglass'), 6, 8, 2, 11)
    rect(segm[0], L('skin'), 15, 2, 5, 4)
    rect(segm[0], L('skin'), 28, 20, 8, 9)
    rect(segm[0], L('top'), 14, 8, 12, 12)
    rect(segm[1], L('skin'), 0, 0, 37, 13)
    rect(segm[1], L('face'), 30, 20, 7, 9)
    return random_pictures(2, 37, 29, 3731), segm  # (a seed that keeps the fill fractions inside [0.01, 0.99])


def lip_300x260(face_rows):
    """B = 1: a top whose cut (251 x 240) is larger than 224 on both axes, and a face whose cut has `face_rows` rows."""
    L = LIP_LABELS.index
    segm = np.zeros((1, 300, 260), dtype=np.uint8)
    rect(segm[0], L('top'), 40, 10, 252, 241)
    rect(segm[0], L('face'), 5, 100, face_rows + 1, 91)
    return random_pictures(1, 300, 260, 300260), segm


def lip_1101x750():
    """B = 1, the high-resolution limit: the background and one large group (pants, the cut 900 x 650)."""
    L = LIP_LABELS.index
    segm = np.zeros((1, 1101, 750), dtype=np.uint8)
    rect(segm[0], L('pants'), 100, 50, 901, 651)
    return random_pictures(1, 1101, 750, 1101750), segm


def fill_fractions(pictures, segm, segmenter):
    """(S_c mod N) / N per (sample, channel) of the background group; empty masks are left out."""
    ids = group_ids(segmenter)['background']
    out = []
    for p, s in zip(pictures, segm):
        m = binary_mask(s, ids)
        n = int(m.sum())
        if n:
            out.append([(int(p[..., c][m].astype(np.int64).sum()) % n) / n for c in range(3)])
    return np.array(out)
