"""The host side of the style crops, no GPU: tests/styles_ref.py (the restatement the GPU tests compare with) is pinned to
Pillow and to the reference's rules case by case, the fixtures of the GPU tests are shown to hold what they claim, and the
package's tables and argument checks are exercised."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import styles_ref as sr
from upgpt_amd import _lib, styles
from upgpt_amd.inference import CLIP_MEAN, CLIP_STD, get_empty_style, style_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w) of a padded cut -> the T.Resize(224) size
RESIZE_SHAPES = {(100, 99): (226, 224), (5, 4): (280, 224), (2, 1): (448, 224), (57, 58): (224, 227), (1101, 750): (328, 224),
                 (256, 176): (325, 224)}


def test_to_pil_image_returns_every_byte():
    """T.ToPILImage on the float tensor is mul(255).byte(); on fl(u / 255) it gives u back for all 256 values."""
    u = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(u.to(torch.float32).div(255).mul(255).byte(), u)


@pytest.mark.parametrize("shape", list(RESIZE_SHAPES))
def test_image_transform_equals_pillow_resize_and_crop(shape):
    h, w = shape
    oh, ow = RESIZE_SHAPES[shape]
    assert sr.resized_size(h, w) == (oh, ow)
    pic = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(pic).resize((ow, oh), Image.BILINEAR))
    t, l = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
    assert np.array_equal(sr.image_transform(pic), pil[t:t + 224, l:l + 224])


def test_resize_leaves_a_short_side_of_224_alone():
    assert sr.resized_size(224, 224) == (224, 224) and sr.resized_size(300, 224) == (300, 224)
    assert sr.resized_size(224, 231) == (224, 231)
    pic = np.random.default_rng(3).integers(0, 256, (231, 224, 3), dtype=np.uint8)
    assert np.array_equal(sr.image_transform(pic), pic[4:228])  # (3.5 rounds to the even 4)


def test_range_rule_on_hand_made_masks():
    m = np.zeros((10, 12), dtype=bool)
    assert sr.mask_range(m) == (0, 12, 0, 10)  # empty mask: 0, W, 0, H
    m[2:6, 3:9] = True
    assert sr.mask_range(m) == (3, 8, 2, 5)  # the INDEX of the last column / row
    pic = np.full((10, 12, 3), 200, dtype=np.uint8)
    u8, valid = sr.crop(pic, m, 'top')
    assert valid == 1
    # ... used as exclusive ends: the cut is 3 x 5, the last masked row and column are dropped
    assert (5 - 2, 8 - 3) == (3, 5) and sr.pad_amounts(3, 5) == (0, 1)
    assert np.array_equal(u8, sr.image_transform(np.pad(pic[2:5, 3:8], ((1, 1), (0, 0), (0, 0)))))
    row = np.zeros((10, 12), dtype=bool)
    row[4, 2:9] = True
    assert sr.mask_range(row) == (2, 8, 4, 4) and sr.crop(pic, row, 'top')[1] == 0  # a single row: an empty cut
    col = np.zeros((10, 12), dtype=bool)
    col[1:8, 5] = True
    assert sr.mask_range(col) == (5, 5, 1, 7) and sr.crop(pic, col, 'top')[1] == 0  # a single column
    assert not sr.crop(pic, row, 'top')[0].any()
    # an empty mask of a masked group: the cut is the whole (zeroed) picture, valid with zero bytes
    u8, valid = sr.crop(pic, np.zeros((10, 12), dtype=bool), 'hair')
    assert valid == 1 and not u8.any()
    # an empty `face` mask: the whole unmasked picture (the reference's behaviour, kept)
    u8, valid = sr.crop(pic, np.zeros((10, 12), dtype=bool), 'face')
    assert valid == 1 and bool((u8 != 0).any())


@pytest.mark.parametrize("d,pads", [(-3, (0, 2)), (-1, (0, 1)), (0, (0, 0)), (1, (0, 0)), (2, (1, 0)), (5, (2, 0))])
def test_pad_rule(d, pads):
    cw = 9
    ch = cw + d
    assert sr.pad_amounts(ch, cw) == pads
    ph, pw = ch + 2 * pads[1], cw + 2 * pads[0]
    assert ph - pw in (0, 1)  # square to within a row, never wider than high
    pic = np.random.default_rng(40 + d).integers(1, 256, (30, 30, 3), dtype=np.uint8)
    m = np.zeros((30, 30), dtype=bool)
    m[4:4 + ch + 1, 6:6 + cw + 1] = True
    padded = np.zeros((ph, pw, 3), dtype=np.uint8)
    padded[pads[1]:pads[1] + ch, pads[0]:pads[0] + cw] = pic[4:4 + ch, 6:6 + cw]
    u8, valid = sr.crop(pic, m, 'outer')
    assert valid == 1 and np.array_equal(u8, sr.image_transform(padded))


def test_half_even_centre_offsets():
    assert [sr.center_offset(n) for n in (224, 225, 226, 227, 228, 229, 231, 448)] == [0, 0, 1, 2, 2, 2, 4, 112]


def test_face_rule_at_128_and_129_rows():
    pic = np.random.default_rng(9).integers(0, 256, (200, 150, 3), dtype=np.uint8)
    for rows, want in ((128, 1), (129, 0)):
        m = np.zeros((200, 150), dtype=bool)
        m[10:10 + rows + 1, 20:120] = True
        assert sr.mask_range(m)[3] - sr.mask_range(m)[2] == rows
        u8, valid = sr.crop(pic, m, 'face')
        assert valid == want and bool(u8.any()) == bool(want)
        assert sr.crop(pic, m, 'top')[1] == 1  # (the rule is the face's alone)
    m = np.zeros((200, 150), dtype=bool)
    m[10:60, 20:70] = True
    m[10:30, 40:70] = False  # (an L: part of the box is outside the mask)
    face, top = sr.crop(pic, m, 'face')[0], sr.crop(pic, m, 'top')[0]
    assert not np.array_equal(face, top)  # the face keeps the picture's own background inside its box


FIXTURES = {"lip_64x48": (sr.lip_64x48, 'lip'), "mm_37x29": (sr.mm_37x29, 'mm'), "lip_300x260_128": (lambda: sr.lip_300x260(128), 'lip'),
            "lip_300x260_129": (lambda: sr.lip_300x260(129), 'lip'), "lip_1101x750": (sr.lip_1101x750, 'lip')}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_exact_fill_equals_the_float32_expression_on_the_fixtures(name):
    """The fixtures keep (S_c mod N) / N inside [0.01, 0.99], away from where float32 rounding noise decides the byte;
    there the reference's own expression gives the exact floor(S_c / N)."""
    make, segmenter = FIXTURES[name]
    pics, segm = make()
    frac = sr.fill_fractions(pics, segm, segmenter)
    print(name, "fractions", np.round(frac, 3).tolist())
    assert frac.size and bool(((frac >= 0.01) & (frac <= 0.99)).all())
    ids = sr.group_ids(segmenter)['background']
    for p, s in zip(pics, segm):
        m = sr.binary_mask(s, ids)
        assert sr.fill_colour(p, m, 'exact') == sr.fill_colour(p, m, 'float32')
        assert np.array_equal(sr.crop(p, m, 'background', 'exact')[0], sr.crop(p, m, 'background', 'float32')[0])


def test_constant_colour_is_where_the_two_fills_differ():
    """Documented, not reproduced: for a constant-colour region the mean is an exact integer k and the reference's float32
    expression returns k or k - 1 as rounding falls; floor(S_c / N) is k."""
    differ = 0
    for n in (7, 100, 4507):
        m = np.zeros((70, 70), dtype=bool)
        m.reshape(-1)[:n] = True
        for k in range(0, 256, 5):
            pic = np.full((70, 70, 3), k, dtype=np.uint8)
            exact, f32 = sr.fill_colour(pic, m, 'exact'), sr.fill_colour(pic, m, 'float32')
            assert exact == [k] * 3 and all(v in (k, k - 1) for v in f32)
            differ += exact != f32
    print("constant colour: %d of %d cases differ" % (differ, 3 * 52))
    assert differ > 0
    assert sr.fill_colour(np.zeros((4, 4, 3), dtype=np.uint8), np.zeros((4, 4), dtype=bool), 'exact') is None  # N == 0


def test_the_64x48_fixture_holds_every_case_it_names():
    pics, segm = sr.lip_64x48()
    bx = sr.boxes(pics, segm, 'lip')
    names = list(sr.group_ids('lip'))
    d = {(b, n): int((bx[b, g, 3] - bx[b, g, 2]) - (bx[b, g, 1] - bx[b, g, 0])) for b in range(3) for g, n in enumerate(names)
         if bx[b, g, 4] > 0 and n != 'background'}
    vals = set(d.values())
    assert any(v > 0 and v % 2 for v in vals) and any(v > 0 and v % 2 == 0 for v in vals)
    assert any(v < 0 and v % 2 for v in vals) and any(v < 0 and v % 2 == 0 for v in vals)
    assert {-3, -1, 0, 1, 2} <= vals
    g = names.index
    assert bx[1, g('top'), :4].tolist() == [0, 47, 0, 63] == bx[1, g('bottom'), :4].tolist()  # touches all four borders
    assert bx[1, g('hair'), :5].tolist() == [0, 48, 0, 64, 0]  # an empty group
    assert bx[0, g('headwear'), 2] == bx[0, g('headwear'), 3] and bx[0, g('headwear'), 4] == 7  # one row
    assert bx[0, g('shoes'), 0] == bx[0, g('shoes'), 1] and bx[0, g('shoes'), 4] == 9  # one column
    assert (bx[0, g('outer'), 3] - bx[0, g('outer'), 2], bx[0, g('outer'), 1] - bx[0, g('outer'), 0]) == (2, 1)
    _, valid, u8 = sr.styles(pics, segm, 'lip')
    slot = sr.STYLE_NAMES.index
    assert valid[0].tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 0]
    assert valid[:, slot('background')].tolist() == [1, 1, 1] and valid[:, slot('accesories')].tolist() == [0, 0, 0]
    assert sr.implied_sizes(bx[0, g('outer')], 'outer', 64, 48) == ((2, 448, 112), (1, 224, 0))
    assert bool(u8[0, slot('outer')].any())


def test_the_large_fixtures_hold_what_they_name():
    for rows, want in ((128, 1), (129, 0)):
        pics, segm = sr.lip_300x260(rows)
        bx = sr.boxes(pics, segm, 'lip')[0]
        assert bx[0, 3] - bx[0, 2] == rows
        top = bx[list(sr.group_ids('lip')).index('top')]
        assert (top[3] - top[2], top[1] - top[0]) == (251, 240)  # larger than 224 on both axes
        assert sr.styles(pics, segm, 'lip')[1][0, 0] == want
    pics, segm = sr.lip_1101x750()
    bx = sr.boxes(pics, segm, 'lip')[0]
    bottom = bx[list(sr.group_ids('lip')).index('bottom')]
    assert (bottom[3] - bottom[2], bottom[1] - bottom[0]) == (900, 650)
    assert sr.implied_sizes(bx[1], 'background', 1101, 750) == ((1101, 328, 52), (750, 224, 0))


def test_group_tables_and_slot_order():
    assert style_names == sr.STYLE_NAMES
    for key, seg, n in (('lip', styles.LIP, 8), ('mm', styles.DEEPFASHION_MM, 3)):
        labels, groups = sr.TABLES[key]
        assert seg is styles.get_segmenter(key) and len(seg.names) == n
        assert seg.label_names == labels and list(seg.groups.items()) == [(k, tuple(v)) for k, v in groups.items()]
        assert list(seg.group_ids.items()) == [(k, tuple(v)) for k, v in sr.group_ids(key).items()]
        for label in range(256):
            want = sum(1 << g for g, ids in enumerate(sr.group_ids(key).values()) if label in ids)
            assert seg.label_groups[label] == want
        flags = dict(zip(seg.names, seg.group_flags))
        assert flags['background'] == _lib.STYLE_FILL and flags['face'] == 128 << 8
        assert all(v == _lib.STYLE_MASK for k, v in flags.items() if k not in ('background', 'face'))
    assert styles.LIP.slot_groups(style_names) == [0, 2, 3, 1, 4, 7, 5, 6, -1]
    assert styles.DEEPFASHION_MM.slot_groups(style_names) == [0, -1, -1, 1, -1, -1, -1, -1, -1]
    assert styles.LIP.label_groups[styles.LIP.label2id['dress']] == (1 << 4) | (1 << 5)  # a label of two groups
    assert tuple(np.float32(v) for v in CLIP_MEAN + CLIP_STD) == tuple(np.float32(v) for v in sr.MEAN + sr.STD)


def test_aliases_of_the_reference_import_paths():
    from ldm.data import generate_utils, segm_utils
    assert segm_utils.LipSegmenter() is styles.LIP and segm_utils.DeepfashionMMSegmenter() is styles.DEEPFASHION_MM
    assert generate_utils.LipSegmenter is segm_utils.LipSegmenter
    assert segm_utils.Segmenter is styles.Segmenter


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    for name in ("upk_segm_boxes_u8", "upk_style_crops_u8"):
        assert ("int %s(upk_ctx* ctx" % name) in header and name in _lib.SYMBOLS
        assert hasattr(_lib.load_library(), name)
    assert "#define UPK_STYLE_FILL 0x1" in header and "#define UPK_STYLE_MASK 0x2" in header


def test_the_empty_style_is_clip_norm_of_zeros():
    """A missing style in the reference's datasets is clip_norm(torch.zeros(3, 224, 224)), float32 arithmetic, which is
    what the kernel writes.  The demo's get_empty_style() forms the same expression in float64; cast to fp32 it is the same
    bits in channels 0 and 1 and ONE ulp away in channel 2 (3216865239 against 3216865240)."""
    want = sr.clip_norm(np.zeros((224, 224, 3), dtype=np.uint8))
    ref = ((torch.zeros(3, 224, 224) - torch.tensor(sr.MEAN).view(3, 1, 1)) / torch.tensor(sr.STD).view(3, 1, 1)).numpy()
    assert np.array_equal(want.view(np.uint32), ref.view(np.uint32))
    demo = get_empty_style().to(torch.float32).numpy()
    diff = want.view(np.uint32).astype(np.int64) - demo.view(np.uint32).astype(np.int64)
    assert [int(np.abs(diff[c]).max()) for c in range(3)] == [0, 0, 1]


def test_argument_errors_decidable_without_a_device():
    pics = np.zeros((2, 8, 6, 3), dtype=np.uint8)
    segm = np.zeros((2, 8, 6), dtype=np.uint8)
    with pytest.raises(ValueError, match="segmenter"):
        styles.style_crops(pics, segm, segmenter='coco')
    with pytest.raises(ValueError, match="slots"):
        styles.style_crops(pics, segm, slots=[])
    with pytest.raises(ValueError, match="slots"):
        styles.style_crops(pics, segm, slots=['face'] * 33)
    with pytest.raises(TypeError, match="pictures must be uint8"):
        styles.style_crops(pics.astype(np.float32), segm)
    with pytest.raises(TypeError, match="segm must be uint8"):
        styles.style_crops(pics, segm.astype(np.int64))
    with pytest.raises(TypeError, match="pictures must be a uint8 tensor"):
        styles.style_crops([1, 2], segm)
    with pytest.raises(ValueError, match=r"pictures must be \[B, H, W, 3\]"):
        styles.style_crops(pics[0], segm)
    with pytest.raises(ValueError, match="3-channel"):
        styles.style_crops(np.zeros((2, 8, 6, 4), dtype=np.uint8), segm)
    with pytest.raises(ValueError, match="does not match"):
        styles.style_crops(pics, segm[:, :7])
    with pytest.raises(ValueError, match="does not match"):
        styles.style_boxes(pics, segm[:1])
    with pytest.raises(ValueError, match="32 groups"):
        styles.Segmenter(['l%d' % i for i in range(40)], {'g%d' % i: ['l%d' % i] for i in range(33)})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            styles.style_crops(pics, segm)
