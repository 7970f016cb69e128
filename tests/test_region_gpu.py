"""upk_region_mask_u8 and upk_composite_u8 on the GPU against the numpy restatement tests/region_ref.py, bit
for bit: mask bytes, keep (as uint32), cells, the blended bytes and alpha; every output optional in turn, pitched outputs
untouched outside their rows, every refusal with its code and no launch, and both launches captured and replayed."""
import numpy as np
import pytest
import torch

import region_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(8, 8, 8), (16, 8, 8), (32, 24, 8), (24, 20, 4), (64, 48, 16)]  # (H, W, factor)
RADII = [0, 1, 7, 8, 9, 32]
FEATHERS = [0, 1, 2, 5, 16]
POISON = 0x5A
EINVAL, ESHAPE = -1, -2


def pitched(arr, pad, gap, fill=POISON):
    """A device copy of uint8 [B, H, ROW...] with `pad` extra bytes per row and `gap` between samples -> (view, buffer)."""
    arr = np.ascontiguousarray(arr)
    b, h = arr.shape[:2]
    row = int(np.prod(arr.shape[2:]))
    pitch, ss = row + pad, h * (row + pad) + gap
    buf = torch.full((b * ss + 8,), fill, dtype=torch.uint8, device=DEV)
    rows = buf.as_strided((b, h, row), (ss, pitch, 1))
    rows.copy_(torch.from_numpy(arr.reshape(b, h, row)).to(DEV))
    return buf.as_strided(arr.shape, (ss, pitch, 1) if arr.ndim == 3 else (ss, pitch, arr.shape[3], 1)), buf


def outside_rows(buf, view, row):
    """The bytes of `buf` that are not inside a row of `view`."""
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    b, h = view.shape[:2]
    keep.as_strided((b, h, row), (view.stride(0), view.stride(1), 1)).fill_(False)
    return buf[keep]


def region(ctx, segm, labels, r, f, pad=0, gap=0, want=("mask", "keep", "cells")):
    b, h, w = segm.shape
    sg, _ = pitched(segm, pad, gap)
    mask, mbuf = pitched(np.zeros((b, h, w), np.uint8), pad, gap)
    mbuf.fill_(POISON)
    keep = torch.full((b, 1, h // f, w // f), 7.0, device=DEV)
    cells = torch.full((b,), -9, dtype=torch.int32, device=DEV)
    on = lambda name, t: t if name in want else None
    ctx.region_mask(sg, sg.stride(1), sg.stride(0), b, h, w, labels, r, f, on("mask", mask), mask.stride(1), mask.stride(0),
                    on("keep", keep), on("cells", cells))
    torch.cuda.synchronize()
    return mask, mbuf, keep, cells


def check_region(ctx, segm, labels, r, f, pad=0, gap=0):
    want_mask, want_keep, want_cells = rr.region(segm, labels, r, f)
    mask, mbuf, keep, cells = region(ctx, segm, labels, r, f, pad, gap)
    tag = (segm.shape, r, f, pad, gap)
    assert np.array_equal(mask.cpu().numpy(), want_mask), tag
    assert np.array_equal(keep.cpu().numpy().view(np.uint32), want_keep.view(np.uint32)), tag
    assert np.array_equal(cells.cpu().numpy(), want_cells), tag
    assert bool(outside_rows(mbuf, mask, segm.shape[2]).eq(POISON).all()), tag
    return want_mask


def compose(ctx, orig, gen, mask, fr, pad=0, gap=0, alpha=True):
    b, h, w = mask.shape
    o, _ = pitched(orig, pad, gap)
    g, _ = pitched(gen, 3 * pad, gap)
    m, _ = pitched(mask, pad, gap)
    out, obuf = pitched(np.zeros((b, h, w, 3), np.uint8), pad, gap)
    al, abuf = pitched(np.zeros((b, h, w), np.uint8), 2 * pad, gap)
    obuf.fill_(POISON), abuf.fill_(POISON)
    ctx.composite(o, o.stride(1), o.stride(0), g, g.stride(1), g.stride(0), m, m.stride(1), m.stride(0), b, h, w, fr, out,
                  out.stride(1), out.stride(0), al if alpha else None, al.stride(1), al.stride(0))
    torch.cuda.synchronize()
    return out, obuf, al, abuf


def check_compose(ctx, orig, gen, mask, fr, pad=0, gap=0):
    want_out, want_a = rr.composite(orig, gen, mask, fr)
    out, obuf, al, abuf = compose(ctx, orig, gen, mask, fr, pad, gap)
    tag = (mask.shape, fr, pad, gap)
    assert np.array_equal(out.cpu().numpy(), want_out), tag
    assert np.array_equal(al.cpu().numpy(), want_a), tag
    assert bool(outside_rows(obuf, out, 3 * mask.shape[2]).eq(POISON).all()), tag
    assert bool(outside_rows(abuf, al, mask.shape[2]).eq(POISON).all()), tag


def random_maps(b, h, w, seed):
    rng = np.random.default_rng(seed)
    segm = rng.integers(0, 20, (b, h, w), dtype=np.uint8)
    segm[rng.random((b, h, w)) < 0.9] = 0  # sparse: dilation has something to do
    return segm


def pictures(b, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_region_equals_restatement(ctx, shape):
    h, w, f = shape
    case = 0
    for b in (1, 3):
        segm = random_maps(b, h, w, h * 7 + w + b)
        for r in RADII:
            pad, gap = ((0, 0), (3, 0), (0, 5), (3, 7))[case % 4]
            check_region(ctx, segm, [5, 6, 10, 11], r, f, pad, gap)
            case += 1
    check_region(ctx, random_maps(3, h, w, 99), [5], 8, f, 3, 5)
    for fother in (1, 2, 4, 8, 16):  # every factor the map allows
        if h % fother == 0 and w % fother == 0:
            check_region(ctx, random_maps(2, h, w, fother), [5, 7], 3, fother)


@pytest.mark.parametrize("shape", SHAPES)
def test_single_pixels_cross_cell_and_band_edges_by_one(ctx, shape):
    h, w, f = shape
    spots = {(0, 0), (h - 1, w - 1), (min(7, h - 1), w // 2), (min(8, h - 1), w // 2), (h // 2, f - 1), (h // 2, min(f, w - 1)),
             (min(15, h - 1), 0), (min(16, h - 1), w - 1)}
    for y, x in sorted(spots):
        segm = np.zeros((1, h, w), np.uint8)
        segm[0, y, x] = 5
        for r in (0, 1):
            mask = check_region(ctx, segm, [5], r, f)
            assert int((mask != 0).sum()) == (min(y + r, h - 1) - max(y - r, 0) + 1) * (min(x + r, w - 1) - max(x - r, 0) + 1)


def test_widths_that_are_no_multiple_of_four(ctx):
    for h, w, f in ((9, 7, 1), (10, 70, 2), (5, 130, 1), (3, 1, 1)):
        segm = random_maps(2, h, w, w)
        segm[0, h // 2, w // 2] = 5
        for r, pad in ((0, 0), (1, 1), (9, 0)):
            mask = check_region(ctx, segm, [5, 6], r, f, pad, pad)
        orig, gen = pictures(2, h, w, h)
        for fr, pad in ((0, 0), (2, 1), (16, 0)):
            check_compose(ctx, orig, gen, mask, fr, pad, 4 * pad)


def test_empty_full_and_the_end_labels(ctx):
    h, w, f = 32, 24, 8
    segm = random_maps(2, h, w, 4)
    segm[0, 3, 4], segm[1, 30, 20] = 255, 255
    for r in (0, 9):
        _, _, keep, cells = region(ctx, segm, [], r, f)
        assert bool(keep.eq(1.0).all()) and cells.tolist() == [0, 0]
        check_region(ctx, segm, [], r, f)
        check_region(ctx, segm, list(range(256)), r, f)
        check_region(ctx, segm, [0], r, f, 3, 2)
        check_region(ctx, segm, [255], r, f)
        check_region(ctx, segm, [0, 255], r, f)
        check_region(ctx, segm, [31, 32, 63, 64, 255], r, f)
    check_region(ctx, np.full((2, h, w), 7, np.uint8), [7], 0, f)
    assert region(ctx, np.full((2, h, w), 7, np.uint8), [7], 0, f)[3].tolist() == [12, 12]


def test_largest_supported_picture(ctx):
    """512 x 384 at dilate 32 / feather 16: the largest staging, more than one word per row, 32 bands."""
    h, w = 512, 384
    segm = random_maps(2, h, w, 12)
    segm[segm != 5] = 0
    segm[1] = 0
    segm[1, 200:260, 100:190] = 5
    mask = check_region(ctx, segm, [5], 32, 8)
    check_region(ctx, segm, [5], 32, 1)
    orig, gen = pictures(2, h, w, 5)
    check_compose(ctx, orig, gen, mask, 16)


@pytest.mark.parametrize("shape", SHAPES)
def test_composite_equals_restatement(ctx, shape):
    h, w, _ = shape
    yy, xx = np.mgrid[0:h, 0:w]
    corner = np.zeros((h, w), np.uint8)
    corner[0, 0] = corner[h - 1, w - 1] = 255
    masks = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "corner": corner,
             "checker": (((yy + xx) & 1) * 3).astype(np.uint8),  # (any non-zero byte is inside)
             "random": (np.random.default_rng(h).random((h, w)) < 0.3).astype(np.uint8) * 255}
    case = 0
    for b in (1, 3):
        orig, gen = pictures(b, h, w, h + w + b)
        for name, m in masks.items():
            mask = np.stack([np.roll(m, i, axis=1) for i in range(b)])
            for fr in FEATHERS:
                pad, gap = ((0, 0), (3, 0), (0, 5), (1, 2), (4, 8))[case % 5]
                check_compose(ctx, orig, gen, mask, fr, pad, gap)
                case += 1
    orig, gen = pictures(1, h, w, 1)
    out, _, al, _ = compose(ctx, orig, gen, masks["empty"][None], 16)
    assert np.array_equal(out.cpu().numpy(), orig) and not bool(al.any())
    out, _, al, _ = compose(ctx, orig, gen, masks["full"][None], 16)
    assert np.array_equal(out.cpu().numpy(), gen) and bool(al.eq(255).all())


def test_every_output_is_optional(ctx):
    h, w, f = 32, 24, 8
    segm = random_maps(3, h, w, 8)
    want = rr.region(segm, [5, 6], 3, f)
    for names in (("mask",), ("keep",), ("cells",), ("mask", "keep"), ("keep", "cells"), ("mask", "cells")):
        mask, mbuf, keep, cells = region(ctx, segm, [5, 6], 3, f, 3, 4, want=names)
        assert np.array_equal(mask.cpu().numpy(), want[0]) if "mask" in names else bool(mbuf.eq(POISON).all())
        assert np.array_equal(keep.cpu().numpy(), want[1]) if "keep" in names else bool(keep.eq(7.0).all())
        assert np.array_equal(cells.cpu().numpy(), want[2]) if "cells" in names else bool(cells.eq(-9).all())
    orig, gen = pictures(3, h, w, 2)
    out, _, al, abuf = compose(ctx, orig, gen, want[0], 2, 3, 4, alpha=False)
    assert np.array_equal(out.cpu().numpy(), rr.composite(orig, gen, want[0], 2)[0]) and bool(abuf.eq(POISON).all())


def test_refusals_launch_nothing(ctx):
    from upgpt_amd._lib import UpkError
    b, h, w, f = 2, 16, 16, 8
    segm = torch.zeros((b, h, w), dtype=torch.uint8, device=DEV)
    mask = torch.full((b, h, w), POISON, dtype=torch.uint8, device=DEV)
    keep = torch.full((b, 1, h // f, w // f), 7.0, device=DEV)
    cells = torch.full((b,), -9, dtype=torch.int32, device=DEV)
    good = dict(segm=segm, segm_pitch=w, segm_ss=h * w, batch=b, h=h, w=w, labels=[0], dilate=2, factor=f, mask_u8=mask, mask_pitch=w,
                mask_ss=h * w, keep=keep, cells=cells)
    bad = [(dict(segm=None), EINVAL), (dict(labels=None), EINVAL), (dict(mask_u8=None, keep=None, cells=None), EINVAL),
           (dict(batch=0), EINVAL), (dict(h=0), EINVAL), (dict(w=-2), EINVAL), (dict(dilate=-1), EINVAL), (dict(dilate=33), EINVAL),
           (dict(factor=3), EINVAL), (dict(factor=0), EINVAL), (dict(factor=32), EINVAL), (dict(h=12), EINVAL), (dict(w=12), EINVAL),
           (dict(segm_pitch=w - 1), EINVAL), (dict(mask_pitch=w - 1), EINVAL), (dict(keep=keep.data_ptr() + 2), EINVAL),
           (dict(cells=cells.data_ptr() + 1), EINVAL), (dict(mask_ss=h * w - 1), EINVAL), (dict(mask_ss=0), EINVAL),
           (dict(mask_u8=segm), EINVAL), (dict(batch=65536, mask_u8=None), ESHAPE),
           (dict(batch=1, w=16384 * 8, h=8, segm_pitch=16384 * 8, mask_u8=None), ESHAPE),  # a row too wide for a band's bit rows
           (dict(batch=1, h=4096, w=512, segm_pitch=512, factor=1, mask_u8=None, keep=None), ESHAPE)]  # too tall for the count
    for change, code in bad:
        with pytest.raises(UpkError) as e:
            ctx.region_mask(**dict(good, **change))
        assert e.value.code == code, (change, str(e.value))
    torch.cuda.synchronize()
    assert bool(mask.eq(POISON).all()) and bool(keep.eq(7.0).all()) and bool(cells.eq(-9).all()) and not bool(segm.any())

    orig = torch.zeros((b, h, w, 3), dtype=torch.uint8, device=DEV)
    gen = torch.ones((b, h, w, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((b, h, w, 3), POISON, dtype=torch.uint8, device=DEV)
    al = torch.full((b, h, w), POISON, dtype=torch.uint8, device=DEV)
    mk = torch.full((b, h, w), 255, dtype=torch.uint8, device=DEV)
    wide = lambda px: torch.full((4 * 4096 * px,), POISON, dtype=torch.uint8, device=DEV)  # (a row too wide to stage)
    good = dict(orig=orig, orig_pitch=3 * w, orig_ss=3 * h * w, gen=gen, gen_pitch=3 * w, gen_ss=3 * h * w, mask_u8=mk, mask_pitch=w,
                mask_ss=h * w, batch=b, h=h, w=w, feather=2, out=out, out_pitch=3 * w, out_ss=3 * h * w, alpha_out=al, alpha_pitch=w,
                alpha_ss=h * w)
    bad = [(dict(orig=None), EINVAL), (dict(gen=None), EINVAL), (dict(mask_u8=None), EINVAL), (dict(out=None), EINVAL),
           (dict(batch=0), EINVAL), (dict(h=-1), EINVAL), (dict(w=0), EINVAL), (dict(feather=-1), EINVAL), (dict(feather=17), EINVAL),
           (dict(orig_pitch=3 * w - 1), EINVAL), (dict(gen_pitch=w), EINVAL), (dict(out_pitch=3 * w - 1), EINVAL),
           (dict(mask_pitch=w - 1), EINVAL), (dict(alpha_pitch=w - 1), EINVAL), (dict(out=orig), EINVAL), (dict(out=gen), EINVAL),
           (dict(out=gen.data_ptr() + 3 * h * w), EINVAL), (dict(alpha_out=mk), EINVAL), (dict(alpha_out=out), EINVAL),
           (dict(out_ss=3 * h * w - 1), EINVAL), (dict(alpha_ss=0), EINVAL), (dict(batch=65536), ESHAPE),
           (dict(batch=1, w=4096, h=4, orig=wide(3), orig_pitch=3 * 4096, gen=wide(3), gen_pitch=3 * 4096, out=wide(3), out_pitch=3 * 4096,
                 mask_u8=wide(1), mask_pitch=4096, alpha_out=wide(1), alpha_pitch=4096), ESHAPE)]
    for change, code in bad:
        with pytest.raises(UpkError) as e:
            ctx.composite(**dict(good, **change))
        assert e.value.code == code, (change, str(e.value))
    torch.cuda.synchronize()
    assert bool(out.eq(POISON).all()) and bool(al.eq(POISON).all()) and not bool(orig.any()) and bool(gen.eq(1).all())
    ctx.composite(**dict(good, batch=1, out_ss=0, alpha_ss=-5))  # sample strides are ignored for one sample
    torch.cuda.synchronize()
    assert bool(out[0].eq(1).all()) and bool(out[1].eq(POISON).all()) and bool(al[0].eq(255).all())


def test_capture_and_replay_follow_the_label_map(ctx):
    b, h, w, f = 2, 32, 24, 8
    first, second = random_maps(b, h, w, 1), random_maps(b, h, w, 2)
    orig, gen = pictures(b, h, w, 3)
    sg = torch.from_numpy(first).to(DEV)
    o, g = torch.from_numpy(orig).to(DEV), torch.from_numpy(gen).to(DEV)
    mask = torch.full((b, h, w), POISON, dtype=torch.uint8, device=DEV)
    keep = torch.full((b, 1, h // f, w // f), 7.0, device=DEV)
    cells = torch.full((b,), -9, dtype=torch.int32, device=DEV)
    out = torch.full((b, h, w, 3), POISON, dtype=torch.uint8, device=DEV)
    al = torch.full((b, h, w), POISON, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.graph_begin()
        ctx.region_mask(sg, w, h * w, b, h, w, [5, 6], 3, f, mask, w, h * w, keep, cells)
        ctx.composite(o, 3 * w, 3 * h * w, g, 3 * w, 3 * h * w, mask, w, h * w, b, h, w, 2, out, 3 * w, 3 * h * w, al, w, h * w)
        graph = ctx.graph_end()
        s.synchronize()
        assert bool(mask.eq(POISON).all()) and bool(out.eq(POISON).all())  # (captured, not run)
        got = []
        for segm in (first, second):
            sg.copy_(torch.from_numpy(segm).to(DEV))  # the label map is rewritten between the replays
            ctx.graph_launch(graph)
            s.synchronize()
            got.append([t.cpu().numpy().copy() for t in (mask, keep, cells, out, al)])
    ctx.graph_destroy(graph)
    assert not np.array_equal(got[0][0], got[1][0])
    for segm, (m, k, c, ob, ab) in zip((first, second), got):
        wm, wk, wc = rr.region(segm, [5, 6], 3, f)
        wo, wa = rr.composite(orig, gen, wm, 2)
        assert np.array_equal(m, wm) and np.array_equal(k.view(np.uint32), wk.view(np.uint32)) and np.array_equal(c, wc)
        assert np.array_equal(ob, wo) and np.array_equal(ab, wa)
