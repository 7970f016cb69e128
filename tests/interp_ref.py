"""A fresh numpy restatement of the pose-interpolation contract (include/upk.h, upk_pose_interp_f32), and the
exact-rational census of the (alpha, c1, c2) triples whose truncated box coordinate depends on HOW the blend is evaluated.

The restatement shares no code with upgpt_amd: boxes from the occupancy rule (an element that is neither -1 nor 0), the box
blend in Python floats (IEEE fp64, one rounded operation per operator, no fused multiply-add), the SMPL blend in numpy fp32
(likewise one rounded operation per operator), 1 - alpha in fp64 for both.  tests/test_interp_host.py anchors it to the
reference's own functions (inference.interp_mask, torch's alpha * x + (1 - alpha) * y)."""
from fractions import Fraction

import numpy as np

BG, FG = np.float32(-1.0), np.float32(-0.99215686)
ALPHAS20 = [i / 20 for i in range(21)]
COORDS = range(32)


def box_of(mask):
    """[r0, r1, c0, c1] of the occupied elements of a [h, w] map, or four times -1."""
    occ = (mask != -1.0) & (mask != 0.0)
    rows, cols = np.nonzero(occ.any(axis=1))[0], np.nonzero(occ.any(axis=0))[0]
    if rows.size == 0:
        return [-1, -1, -1, -1]
    return [int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])]


def blend_coord(alpha, c1, c2):
    """int(fl(fl(alpha * c1) + fl((1 - alpha) * c2))): every Python float operator is one rounded fp64 operation."""
    a = float(alpha)
    b = 1.0 - a
    return int(a * float(c1) + b * float(c2))


def frame_box(alpha, src_box, dst_box, h, w):
    """Frame box, clamped as the kernel clamps (lower bounds to [0, size], upper bounds to [-1, size - 1])."""
    if src_box[1] < 0 or dst_box[1] < 0:
        return [-1, -1, -1, -1]
    r0, r1, c0, c1 = (blend_coord(alpha, s, d) for s, d in zip(src_box, dst_box))
    return [min(max(r0, 0), h), min(max(r1, -1), h - 1), min(max(c0, 0), w), min(max(c1, -1), w - 1)]


def interp(src_mask, dst_mask, src_smpl, dst_smpl, alphas):
    """-> (boxes int32 [n + 2, 4], masks fp32 [n, 1, h, w], smpl fp32 [n, 1, d]) of numpy inputs [h, w], [h, w], [d], [d]."""
    src_mask, dst_mask = np.asarray(src_mask, np.float32), np.asarray(dst_mask, np.float32)
    x, y = np.asarray(src_smpl, np.float32).reshape(-1), np.asarray(dst_smpl, np.float32).reshape(-1)
    h, w = src_mask.shape
    n = len(alphas)
    sb, db = box_of(src_mask), box_of(dst_mask)
    boxes = np.zeros((n + 2, 4), np.int32)
    boxes[0], boxes[1] = sb, db
    masks = np.full((n, 1, h, w), BG, np.float32)
    smpl = np.zeros((n, 1, x.size), np.float32)
    for i, alpha in enumerate(alphas):
        r0, r1, c0, c1 = boxes[2 + i] = frame_box(alpha, sb, db, h, w)
        if r1 >= r0 and c1 >= c0 and r1 >= 0 and c1 >= 0:
            masks[i, 0, r0:r1 + 1, c0:c1 + 1] = FG
        a32, b32 = np.float32(alpha), np.float32(1.0 - float(alpha))  # (the subtraction in fp64, then rounded)
        smpl[i, 0] = (a32 * x).astype(np.float32) + (b32 * y).astype(np.float32)
    return boxes, masks, smpl


# ---- exact arithmetic: what other evaluations of the same expression would give

def fl(x, p):
    """The Fraction x rounded to a binary floating-point number of p significand bits, to nearest, ties to even
    (no overflow or underflow in the range used here)."""
    x = Fraction(x)
    if x == 0:
        return x
    s, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - p + 1)
    q = x / ulp
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return s * n * ulp


def trunc(x):
    return int(x)  # (Fraction.__trunc__: toward zero)


def evaluations(alpha, c1, c2):
    """The truncated coordinate under {the contract, an fp64 FMA on the first product, an fp64 FMA on the second product,
    fp32 evaluation}; alpha a Python float."""
    a = Fraction(alpha)  # (exact)
    b = fl(1 - a, 53)
    want = trunc(fl(fl(a * c1, 53) + fl(b * c2, 53), 53))
    fma1 = trunc(fl(a * c1 + fl(b * c2, 53), 53))
    fma2 = trunc(fl(fl(a * c1, 53) + b * c2, 53))
    a32 = fl(a, 24)
    b32 = fl(1 - a32, 24)
    f32 = trunc(fl(fl(a32 * c1, 24) + fl(b32 * c2, 24), 24))
    return want, fma1, fma2, f32


def census():
    """(fma, f32): the (alpha, c1, c2) over ALPHAS20 x COORDS x COORDS whose truncation changes under an fp64 fused
    multiply-add (either operand order) / under fp32 evaluation."""
    fma, f32 = [], []
    for alpha in ALPHAS20:
        for c1 in COORDS:
            for c2 in COORDS:
                want, m1, m2, s = evaluations(alpha, c1, c2)
                if m1 != want or m2 != want:
                    fma.append((alpha, c1, c2))
                if s != want:
                    f32.append((alpha, c1, c2))
    return fma, f32


_HAZARDS = None


def hazards():
    """The union of the two census lists, computed once: the input of the kernel test."""
    global _HAZARDS
    if _HAZARDS is None:
        fma, f32 = census()
        _HAZARDS = (fma, f32, sorted(set(fma) | set(f32)))
    return _HAZARDS


def box_mask(h, w, r0, r1, c0, c1, fg=FG):
    m = np.full((h, w), BG, np.float32)
    m[r0:r1 + 1, c0:c1 + 1] = fg
    return m


def write_pose_folder(folder, mask=None, hw=(256, 192)):
    """A pose folder as the demo has them: a pickle (a list whose first dict holds pred_body_pose (1, 72), pred_betas
    (1, 10), pred_camera (3,)), an RGB JPEG and a mode-P mask PNG with the values {0, 1}.  -> (first dict, mask array)."""
    import os
    import pickle

    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    rng = np.random.default_rng(11)
    first = {"pred_body_pose": rng.standard_normal((1, 72)).astype(np.float32),
             "pred_betas": rng.standard_normal((1, 10)).astype(np.float32),
             "pred_camera": rng.standard_normal(3).astype(np.float32), "bbox": [0, 0, 1, 1]}
    with open(os.path.join(str(folder), "pose.p"), "wb") as f:
        pickle.dump([first, {"other": 1}], f)
    Image.fromarray(rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)).save(os.path.join(str(folder), "pose.jpg"))
    if mask is None:
        mask = np.zeros(hw, np.uint8)
        mask[hw[0] // 8:hw[0] - 9, hw[1] // 4:hw[1] - 30] = 1
    im = Image.fromarray(mask, mode="P")
    im.putpalette([0, 0, 0, 255, 255, 255] + [0] * (254 * 3))
    im.save(os.path.join(str(folder), "pose_mask.png"))
    return first, mask
