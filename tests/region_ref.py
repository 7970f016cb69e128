"""numpy restatement of upk_region_mask_u8 and upk_composite_u8 (include/upk.h): the formulas as they are
written there, a loop over window offsets, int64 arithmetic, nothing clever."""
import numpy as np


def label_set(labels):
    """The 256-bit set as upk_region_mask_u8 takes it: 8 words, bit l % 32 of word l / 32."""
    words = [0] * 8
    for l in labels:
        words[int(l) >> 5] |= 1 << (int(l) & 31)
    return words


def dilate(sel, r):
    """M(y, x) = 1 when some sel(y', x') = 1 with |y - y'| <= r and |x - x'| <= r; outside the picture: unselected."""
    h, w = sel.shape[-2:]
    pad = np.zeros(sel.shape[:-2] + (h + 2 * r, w + 2 * r), dtype=bool)
    pad[..., r:r + h, r:r + w] = sel
    out = np.zeros(sel.shape, dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[..., dy:dy + h, dx:dx + w]
    return out


def region(segm, labels, r, f):
    """segm uint8 [B, H, W] -> (mask_u8 [B, H, W], keep fp32 [B, 1, H / f, W / f], cells int32 [B])."""
    segm = np.asarray(segm)
    b, h, w = segm.shape
    assert h % f == 0 and w % f == 0
    m = dilate(np.isin(segm, np.asarray(sorted(labels), dtype=np.int64)), r)
    edited = m.reshape(b, h // f, f, w // f, f).any(axis=(2, 4))
    keep = np.where(edited, np.float32(0.0), np.float32(1.0)).astype(np.float32)[:, None]
    return (m * np.uint8(255)).astype(np.uint8), keep, edited.sum(axis=(1, 2)).astype(np.int32)


def alpha(mask, fr):
    """A = (255 s + n / 2) / n, s the sum of (mask != 0) over the (2 fr + 1)^2 window with clamped coordinates."""
    m = (np.asarray(mask) != 0).astype(np.int64)
    h, w = m.shape[-2:]
    yy, xx = np.arange(h), np.arange(w)
    s = np.zeros(m.shape, dtype=np.int64)
    for dy in range(-fr, fr + 1):
        rows = m[..., np.clip(yy + dy, 0, h - 1), :]
        for dx in range(-fr, fr + 1):
            s += rows[..., :, np.clip(xx + dx, 0, w - 1)]
    n = (2 * fr + 1) ** 2
    return ((255 * s + n // 2) // n).astype(np.uint8)


def composite(orig, gen, mask, fr):
    """out_c = (A gen_c + (255 - A) orig_c + 127) / 255 -> (out uint8 [..., H, W, 3], A uint8 [..., H, W])."""
    a8 = alpha(mask, fr)
    a = a8.astype(np.int64)[..., None]
    out = (a * np.asarray(gen).astype(np.int64) + (255 - a) * np.asarray(orig).astype(np.int64) + 127) // 255
    return out.astype(np.uint8), a8


def chebyshev_far(sel, d):
    """True where every selected pixel is farther than d (Chebyshev) away."""
    return ~dilate(np.asarray(sel, dtype=bool), d)
