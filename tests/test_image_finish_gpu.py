"""upk_image_finish_u8 through the C ABI on the MI355X, byte-EXACT against tests/finish_ref.py (the reference's torch
expression and the three torchvision transforms restated on the CPU).  No tolerance anywhere: the contract of
include/upk.h is a fixed sequence of single correctly rounded fp32 operations followed by a truncation, and the CPU
restatement executes the same sequence."""
import numpy as np
import pytest
import torch

import finish_ref as fr
from upgpt_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLE, INPUT, DENORM = _lib.FINISH_SAMPLE, _lib.FINISH_INPUT, _lib.FINISH_DENORM
NCHW, NHWC = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC
MODES = {"sample": SAMPLE, "input": INPUT, "denorm": DENORM}
LAYOUTS = {"nchw": NCHW, "nhwc": NHWC}
# the caller's DENORM constants as include/upk.h states them (NOT imported from the code under test)
DM = [np.float32(1 / 0.226862954), np.float32(1 / 0.26130258), np.float32(1 / 0.27577711),
      np.float32(-0.48145466), np.float32(-0.4578275), np.float32(-0.40821073)]
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
# (H, W, crop_size): the two UPGPT sizes; (h - ch, w - cw) = (5, 7): 2.5 -> 2 and 3.5 -> 4, so neither floor nor
# round-half-up passes; 224 x 224 uncropped (the style crops); widths / offsets that are no multiples of 4
SHAPES = {"256x192": (256, 192, [256, 176]), "512x384": (512, 384, [512, 352]), "half_even": (37, 47, [32, 40]),
          "224": (224, 224, None), "odd_w": (40, 50, [36, 45]), "odd_left": (24, 30, [24, 28])}
SENTINEL = 0xA5


def window(h, w, crop):
    return (0, 0, h, w) if crop is None else fr.center_crop_offsets(h, w, crop)


def base_input(mode, B, H, W, seed):
    """Random NCHW fp32 in the mode's documented range."""
    g = torch.Generator().manual_seed(seed)
    if mode == SAMPLE:  # decoder output: mostly inside [-1, 1], a good part beyond the clamp
        return torch.randn(B, 3, H, W, generator=g) * 0.8
    if mode == INPUT:
        return torch.rand(B, 3, H, W, generator=g) * 2 - 1
    img = torch.rand(B, 3, H, W, generator=g)  # CLIP-normalised [0, 1] image
    return (img - torch.tensor(CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_STD).view(1, 3, 1, 1)


def adversarial(mode, c):
    """In-range values of channel c where a last-bit error flips a byte: the exact pre-images of every k / 255 and
    their fp32 neighbours, the ends of the range and their inner neighbours, -0.0, and for SAMPLE values just outside
    (and far outside) the clamp."""
    k = np.arange(256, dtype=np.float64) / 255.0
    if mode == DENORM:
        v = ((k + float(DM[3 + c])) * float(DM[c])).astype(np.float32)
    else:
        v = (2.0 * k - 1.0).astype(np.float32)
    one = np.float32(1.0)
    inner = np.float32(1.0 - 2.0 ** -24)
    vals = [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf)),
            np.array([one, -one, inner, -inner, -0.0, 0.0], dtype=np.float32)]
    if mode == SAMPLE:
        vals.append(np.array([np.nextafter(one, np.float32(2)), -np.nextafter(one, np.float32(2)), 1.5, -1.5, 100., -100.,
                              3.0e38, -3.0e38], dtype=np.float32))
    # (INPUT: the outer neighbours of -1 and 1 stay defined for the reference's .byte(): t * 255 is inside (-1, 256))
    return torch.from_numpy(np.concatenate(vals))


def plant(x, win, mode):
    """Writes adversarial(mode, c) into channel c of sample 0 (and the last sample), row-major from the window's first
    pixel, as many as fit."""
    top, left, ch, cw = win
    for b in {0, x.shape[0] - 1}:
        for c in range(3):
            v = adversarial(mode, c)[:ch * cw]
            blk = x[b, c, top:top + ch, left:left + cw].reshape(-1).clone()
            blk[:v.numel()] = v
            x[b, c, top:top + ch, left:left + cw] = blk.view(ch, cw)
    return x


def expected(mode, x, crop, saturate=False):
    """[B] uint8 HWC arrays of the reference's expression for NCHW x."""
    if mode == SAMPLE:
        t = fr.sample_value(x, crop) if crop is not None else (torch.clamp(x, -1., 1.) + 1.0) / 2.0
    elif mode == INPUT:
        nhwc = x.permute(0, 2, 3, 1)
        t = fr.input_value(nhwc, crop) if crop is not None else (nhwc.permute(0, 3, 1, 2) + 1.0) / 2.0
    else:
        t = fr.denorm_value(x)
        t = fr.center_crop(t, crop) if crop is not None else t
    return np.stack([fr.to_pil_array(ti, saturate) for ti in t])


def run(ctx, mode, layout, x, win, dst=None, dst_x=0):
    """One launch on NCHW host tensor x (laid out as `layout` on the device) -> the destination as a host array."""
    B, _, H, W = x.shape
    src = (x.permute(0, 2, 3, 1) if layout == NHWC else x).contiguous().to(DEV)
    top, left, ch, cw = win
    if dst is None:
        dst = torch.full((B, ch, cw, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    ctx.image_finish(src, layout, B, H, W, 3 * H * W, top, left, ch, cw, dst, dst.stride(1), dst_x, dst.stride(0), mode,
                     DM if mode == DENORM else None)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def report(tag, got, want):
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ" % (tag, bad, want.size))
    return bad


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_bytes_equal_the_reference_expression(ctx, mode, layout, shape):
    """Random inputs in the documented range with the adversarial values planted, B = 1 and 8, both layouts, every shape
    (fast path and per-pixel path): every byte equals the CPU restatement's."""
    H, W, crop = SHAPES[shape]
    win = window(H, W, crop)
    for B in (1, 8):
        x = plant(base_input(MODES[mode], B, H, W, seed=B + 10 * H), win, MODES[mode])
        want = expected(MODES[mode], x, crop)
        got = run(ctx, MODES[mode], LAYOUTS[layout], x, win)
        assert got.shape == want.shape
        assert report("%s %s %s B=%d" % (mode, layout, shape, B), got, want) == 0


def test_the_window_offsets_of_the_half_even_case():
    """(the shape above exercises the rule only if its offsets are the half-to-even ones)"""
    assert window(*SHAPES["half_even"]) == (2, 4, 32, 40)
    assert window(*SHAPES["256x192"]) == (0, 8, 256, 176) and window(*SHAPES["512x384"]) == (0, 16, 512, 352)


@pytest.mark.parametrize("mode", list(MODES))
def test_non_finite_values_and_saturation(ctx, mode):
    """NaN -> 0, -inf -> 0, +inf -> 255 in every mode, and finite values outside the documented range saturate (where
    the reference's .byte() is undefined): against the restatement with the saturation include/upk.h documents."""
    m = MODES[mode]
    H, W = 16, 24
    x = base_input(m, 2, H, W, seed=5)
    specials = torch.tensor([float("nan"), float("-inf"), float("inf"), 3.0, -3.0, 1.0e30, -1.0e30, 7.5, -7.5])
    x[:, :, 0, :specials.numel()] = specials
    for layout in (NCHW, NHWC):
        got = run(ctx, m, layout, x, (0, 0, H, W))
        assert got[:, 0, 0].tolist() == [[0, 0, 0]] * 2, "NaN"
        assert got[:, 0, 1].tolist() == [[0, 0, 0]] * 2, "-inf"
        assert got[:, 0, 2].tolist() == [[255, 255, 255]] * 2, "+inf"
        assert report("%s saturating" % mode, got, expected(m, x, None, saturate=True)) == 0


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dst_x", [0, 176, 177])
def test_destination_window_inside_a_strip(ctx, dst_x, layout):
    """A 256 x 176 crop written at x = 0 / 176 / 177 of a wider strip with spare rows and a padded row pitch: the window
    holds the picture, every other byte keeps its sentinel."""
    H, W, crop = SHAPES["256x192"]
    win = window(H, W, crop)
    B, rows, width = 2, 256 + 3, 3 * 176 + 5
    for mode in (SAMPLE, DENORM):
        x = plant(base_input(mode, B, H, W, seed=dst_x), win, mode)
        store = torch.full((B, rows, width + 7, 3), SENTINEL, dtype=torch.uint8, device=DEV)  # (pitch > width * 3)
        dst = store[:, :, :width]
        got = run(ctx, mode, LAYOUTS[layout], x, win, dst=dst, dst_x=dst_x)
        want = np.full((B, rows, width, 3), SENTINEL, dtype=np.uint8)
        want[:, :256, dst_x:dst_x + 176] = expected(mode, x, crop)
        assert report("strip x=%d" % dst_x, got, want) == 0
        assert bool((store[:, :, width:] == SENTINEL).all())


def test_components_side_by_side_need_no_concat_pass(ctx):
    """Four launches at x = 0, cw, 2 cw, 3 cw build the reference's torch.cat([...], 2) strip."""
    H, W, crop = SHAPES["256x192"]
    win = window(H, W, crop)
    B, cw = 2, 176
    xs = [base_input(m, B, H, W, seed=20 + i) for i, m in enumerate((INPUT, SAMPLE, SAMPLE, INPUT))]
    dst = torch.full((B, 256, 4 * cw, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    for i, (x, m) in enumerate(zip(xs, (INPUT, SAMPLE, SAMPLE, INPUT))):
        got = run(ctx, m, NHWC if m == INPUT else NCHW, x, win, dst=dst, dst_x=i * cw)
    vals = [fr.input_value(xs[0].permute(0, 2, 3, 1), crop), fr.sample_value(xs[1], crop), fr.sample_value(xs[2], crop),
            fr.input_value(xs[3].permute(0, 2, 3, 1), crop)]
    want = np.stack([fr.to_pil_array(torch.cat([v[b] for v in vals], 2)) for b in range(B)])
    assert report("concat strip", got, want) == 0


def test_batch_stride_of_a_style_crop_view(ctx):
    """styles[:, s] of a [B, S, 3, 224, 224] tensor: the batch stride is S images."""
    B, S = 2, 3
    st = base_input(DENORM, B * S, 224, 224, seed=3).view(B, S, 3, 224, 224)
    dev = st.to(DEV)
    dst = torch.full((B, 224, S * 224, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    for s in range(S):
        v = dev[:, s]
        ctx.image_finish(v, NCHW, B, 224, 224, v.stride(0), 0, 0, 224, 224, dst, dst.stride(1), s * 224, dst.stride(0),
                         DENORM, DM)
    torch.cuda.synchronize()
    want = np.stack([fr.to_pil_array(torch.cat([fr.denorm_value(c) for c in sb], 2)) for sb in st])
    assert report("styles strip", dst.cpu().numpy(), want) == 0


@pytest.mark.parametrize("shape", ["256x192", "odd_w"])
def test_graph_replay_and_reproducibility(ctx, shape):
    """Two eager runs give the same bytes, and so does a replay of the launch captured in a graph."""
    H, W, crop = SHAPES[shape]
    top, left, ch, cw = win = window(H, W, crop)
    B = 8
    x = plant(base_input(SAMPLE, B, H, W, seed=9), win, SAMPLE)
    a = run(ctx, SAMPLE, NCHW, x, win)
    b = run(ctx, SAMPLE, NCHW, x, win)
    assert np.array_equal(a, b) and np.array_equal(a, expected(SAMPLE, x, crop))
    src = x.to(DEV)
    dst = torch.full((B, ch, cw, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.graph_begin()
        ctx.image_finish(src, NCHW, B, H, W, 3 * H * W, top, left, ch, cw, dst, dst.stride(1), 0, dst.stride(0), SAMPLE)
        g = ctx.graph_end()
        s.synchronize()
        assert bool((dst == SENTINEL).all())  # (captured, not run)
        ctx.graph_launch(g)
        s.synchronize()
        first = dst.cpu().numpy()
        dst.fill_(SENTINEL)
        ctx.graph_launch(g)
    s.synchronize()
    ctx.graph_destroy(g)
    assert np.array_equal(first, a) and np.array_equal(dst.cpu().numpy(), a)


def test_error_codes(ctx):
    H, W = 32, 48
    src = torch.zeros(2, 3, H, W, device=DEV)
    dst = torch.full((2, H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    pitch, bs = dst.stride(1), dst.stride(0)

    def call(src=src, layout=NCHW, B=2, h=H, w=W, sbs=3 * H * W, top=0, left=0, ch=H, cw=W, dst=dst, pitch=pitch, dst_x=0,
             dbs=bs, mode=SAMPLE, dm=None):
        ctx.image_finish(src, layout, B, h, w, sbs, top, left, ch, cw, dst, pitch, dst_x, dbs, mode, dm)

    call()  # (the baseline is valid)
    bad = [dict(src=None), dict(dst=None), dict(src=src.data_ptr() + 2), dict(layout=2), dict(mode=3), dict(B=0),
           dict(top=1), dict(left=1), dict(top=-1, ch=H - 1), dict(ch=H + 1), dict(cw=W + 4),  # window outside the source
           dict(dst_x=1), dict(pitch=W * 3 - 1), dict(dst_x=-1, cw=W - 1),  # destination window outside the pitch
           dict(sbs=3 * H * W - 1), dict(dbs=bs - 1), dict(mode=DENORM), dict(mode=DENORM, dm=[0.0] * 6),
           dict(mode=DENORM, dm=[1.0, 1.0, float("nan"), 0.0, 0.0, 0.0])]
    for kw in bad:
        with pytest.raises(_lib.UpkError) as e:
            call(**kw)
        assert e.value.code == -1, kw  # UPK_EINVAL
    torch.cuda.synchronize()
    call(mode=DENORM, dm=DM)
    torch.cuda.synchronize()
