"""upk_resize_bilinear_u8 through the C ABI on the MI355X against tests/resize_ref.py (pinned to Pillow by
tests/test_resize_host.py): EQUAL ON EVERY BYTE AND EVERY FLOAT BIT.  No tolerance anywhere: both passes are integer
arithmetic and the fp32 finishing is three correctly rounded operations in a fixed order."""
import numpy as np
import pytest
import torch

import resize_ref as rr
from upgpt_amd import _lib, prepare

try:
    from PIL import Image
except ImportError:  # (the comparison with Pillow itself is then left to the host tests)
    Image = None

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
# name -> (h, w, pad (x, y), oh, ow, B)
CASES = {
    "clipped_windows": (11, 9, (0, 0), 5, 4, 1),      # every tap window is clipped at a border
    "dataset_pad8": (256, 176, (8, 0), 128, 96, 3),
    "demo_pad4_5taps": (256, 192, (4, 0), 128, 96, 2),  # 200 -> 96: non-integer scale, 5 taps
    "enlarging": (20, 30, (0, 0), 40, 60, 2),           # fs clamped to 1
    "vertical_only": (64, 45, (0, 0), 37, 45, 2),       # odd width, 37 rows: no multiple of a band height
    "horizontal_only": (64, 45, (0, 0), 64, 24, 2),
    "both_pads": (13, 7, (3, 2), 6, 5, 2),
    "eight_taps": (96, 64, (0, 0), 24, 16, 1),          # scale 4: 9-wide tables, 8 taps
}


def pictures(B, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)


def tables(in_size, out_size):
    t = prepare.resample_coeffs(in_size, out_size)
    if t is None:
        return None
    prepare.validate_table(t, in_size, out_size)
    return torch.from_numpy(t[0]).to(DEV), torch.from_numpy(t[1]).to(DEV), t[2]


def run(ctx, src, pad, oh, ow, u8=True, nchw=True, nhwc=True, dst=None):
    """One launch on the device tensor src [B, h, w, 3] (any pitch / sample stride) -> host arrays (None where not asked)."""
    B, h, w = src.shape[:3]
    if u8 and dst is None:
        dst = torch.full((B, oh, ow, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f1 = torch.full((B, 3, oh, ow), float("nan"), device=DEV) if nchw else None
    f2 = torch.full((B, oh, ow, 3), float("nan"), device=DEV) if nhwc else None
    ctx.resize_bilinear(src, B, h, w, src.stride(1), src.stride(0), pad[0], pad[1], oh, ow, tables(w + 2 * pad[0], ow),
                        tables(h + 2 * pad[1], oh), dst if u8 else None, dst.stride(1) if u8 else 0,
                        dst.stride(0) if u8 else 0, f1, f2)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (dst if u8 else None, f1, f2)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(tag, got, want):
    """got = (u8, nchw, nhwc) host arrays, want = resize_ref.lr_transform's triple; prints the counts, then asserts."""
    g_u8, g_nchw, g_nhwc = got
    w_nchw, w_nhwc, w_u8 = want
    bad = [-1 if g is None else int((g != w).sum()) for g, w in ((g_u8, w_u8),)]
    bad += [-1 if g is None else int((bits(g) != bits(w)).sum()) for g, w in ((g_nchw, w_nchw), (g_nhwc, w_nhwc))]
    print("%s: %d bytes, %d nchw floats, %d nhwc floats differ (-1: not asked) of %d" % (tag, bad[0], bad[1], bad[2], w_u8.size))
    assert all(b <= 0 for b in bad), tag


@pytest.mark.parametrize("case", list(CASES))
def test_bytes_and_float_bits_equal_the_restatement(ctx, case):
    h, w, pad, oh, ow, B = CASES[case]
    pics = pictures(B, h, w, seed=h * 1000 + w)
    want = rr.lr_transform(pics, (oh, ow), pad)
    check(case, run(ctx, torch.from_numpy(pics).to(DEV), pad, oh, ow), want)
    if Image is not None:  # ... and Pillow itself on the padded picture
        for b in range(B):
            padded = np.pad(pics[b], ((pad[1], pad[1]), (pad[0], pad[0]), (0, 0)), mode="edge")
            pil = np.asarray(Image.fromarray(padded).resize((ow, oh), Image.BILINEAR))
            assert np.array_equal(want[2][b], pil), (case, b)


@pytest.mark.parametrize("spare", [7, 8])
def test_strided_source_view_and_padded_destination_pitch(ctx, spare):
    """(256, 176) pad (8, 0) -> (128, 96), B = 3 from a non-contiguous batch view: the pictures are columns 6..182 of
    every second sample of a wider store at an odd byte offset; the destination rows are wider than 3 * ow (a pitch the
    dword stores can take, and one they cannot) and its spare bytes keep their sentinel."""
    h, w, pad, oh, ow, B = CASES["dataset_pad8"]
    store = pictures(2 * B, h + 3, w + 11, seed=5)
    dev = torch.from_numpy(store).to(DEV)
    view = dev[::2, 1:1 + h, 6:6 + w]
    assert view.stride(0) > h * view.stride(1) and view.data_ptr() % 4 != 0 and not view.is_contiguous()
    want = rr.lr_transform(store[::2, 1:1 + h, 6:6 + w], (oh, ow), pad)
    wide = torch.full((B, oh + 2, ow + spare, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    dst = wide[:, :oh, :ow]
    assert dst.stride(1) > 3 * ow
    got = run(ctx, view, pad, oh, ow, dst=dst)
    check("strided view", got, want)
    rest = wide.cpu().numpy().copy()
    rest[:, :oh, :ow] = SENTINEL
    assert bool((rest == SENTINEL).all())
    # a destination the dword stores cannot take (odd base) goes per pixel, same bytes
    flat = torch.full((B * oh * ow * 3 + 1,), SENTINEL, dtype=torch.uint8, device=DEV)
    odd = flat[1:].view(B, oh, ow, 3)
    assert odd.data_ptr() % 4 != 0
    check("odd destination", run(ctx, view, pad, oh, ow, dst=odd), want)


def test_image_transform_case_fp32_only(ctx):
    """(48, 48) -> (48, 48): both passes skipped, no table at all, fp32 outputs only: ToTensor, x * 2 - 1."""
    pics = pictures(2, 48, 48, seed=48)
    got = run(ctx, torch.from_numpy(pics).to(DEV), (0, 0), 48, 48, u8=False)
    want = rr.lr_transform(pics, (48, 48))
    assert np.array_equal(want[2], pics)
    check("image_transform", got, want)
    assert np.array_equal(bits(got[2]), bits(pics.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)))


def test_every_byte_value_finishes_exactly(ctx):
    """All 256 byte values through the fp32 finishing (one row, passes skipped)."""
    pics = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 1, 256, 3)
    got = run(ctx, torch.from_numpy(pics).to(DEV), (0, 0), 1, 256)
    check("all bytes", got, rr.lr_transform(pics, (1, 256)))


@pytest.mark.parametrize("kind", ["const255", "const0", "checker"])
def test_saturation_and_coefficient_sum_rounding(ctx, kind):
    """(32, 24) -> (16, 12): constant 255 must stay 255 although the 22-bit weights do not sum to exactly 2^22."""
    h, w, oh, ow = 32, 24, 16, 12
    if kind == "checker":
        yy, xx = np.mgrid[:h, :w]
        pics = np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], (2, h, w, 3)).copy()
    else:
        pics = np.full((2, h, w, 3), 255 if kind == "const255" else 0, dtype=np.uint8)
    want = rr.lr_transform(pics, (oh, ow))
    if kind != "checker":
        assert bool((want[2] == pics[0, 0, 0, 0]).all())
    check(kind, run(ctx, torch.from_numpy(pics).to(DEV), (0, 0), oh, ow), want)


def test_destinations_alone_and_together_agree(ctx):
    h, w, pad, oh, ow, B = CASES["demo_pad4_5taps"]
    pics = pictures(B, h, w, seed=77)
    src = torch.from_numpy(pics).to(DEV)
    want = rr.lr_transform(pics, (oh, ow), pad)
    all3 = run(ctx, src, pad, oh, ow)
    check("all three", all3, want)
    for i, flags in enumerate((dict(nchw=False, nhwc=False), dict(u8=False, nhwc=False), dict(u8=False, nchw=False))):
        alone = run(ctx, src, pad, oh, ow, **flags)
        assert [a is None for a in alone] == [j != i for j in range(3)]
        check("alone %d" % i, alone, want)
        assert np.array_equal(alone[i], all3[i]) or np.array_equal(bits(alone[i]), bits(all3[i]))
    assert np.array_equal(bits(all3[1].transpose(0, 2, 3, 1)), bits(all3[2]))  # nchw and nhwc hold the same floats
    assert np.array_equal(bits(rr.to_lr(all3[0])), bits(all3[2]))  # ... which are the finishing of the bytes


def test_python_surface(ctx):
    """prepare.resize_u8 / lr_transform: device and host input, out_u8, the table cache."""
    h, w, pad, oh, ow, B = CASES["dataset_pad8"]
    pics = pictures(B, h, w, seed=9)
    want = rr.lr_transform(pics, (oh, ow), pad)
    u8 = prepare.resize_u8(torch.from_numpy(pics).to(DEV), [oh, ow], pad)
    assert u8.is_cuda and u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), want[2])
    assert np.array_equal(prepare.resize_u8(pics, [oh, ow], pad).cpu().numpy(), want[2])  # (a host array is uploaded)
    out = torch.zeros(B, oh, ow, 3, dtype=torch.uint8, device=DEV)
    lr, lr_image = prepare.lr_transform(torch.from_numpy(pics), [oh, ow], pad, out_u8=out)
    assert lr.shape == (B, 3, oh, ow) and lr_image.shape == (B, oh, ow, 3) and lr.is_cuda and lr_image.is_cuda
    assert lr.dtype == lr_image.dtype == torch.float32 and lr.is_contiguous() and lr_image.is_contiguous()
    assert np.array_equal(bits(lr.cpu().numpy()), bits(want[0])) and np.array_equal(bits(lr_image.cpu().numpy()), bits(want[1]))
    assert np.array_equal(out.cpu().numpy(), want[2])
    assert prepare.device_coeffs(u8.device, w + 2 * pad[0], ow) is prepare.device_coeffs(u8.device, w + 2 * pad[0], ow)
    assert prepare.device_coeffs(u8.device, 64, 64) is None


def test_one_launch_per_call(ctx):
    h, w, pad, oh, ow, B = CASES["dataset_pad8"]
    src = torch.from_numpy(pictures(B, h, w, seed=1)).to(DEV)
    prepare.lr_transform(src, [oh, ow], pad)  # (tables uploaded)
    torch.cuda.synchronize()
    before = ctx.lib.upk_kernel_launches(ctx.h, 0)
    prepare.lr_transform(src, [oh, ow], pad)
    mid = ctx.lib.upk_kernel_launches(ctx.h, 0)
    run(ctx, src, pad, oh, ow)
    after = ctx.lib.upk_kernel_launches(ctx.h, 0)
    assert (mid - before, after - mid) == (1, 1)


def test_refusals_launch_nothing(ctx):
    h, w, oh, ow = 16, 12, 8, 6
    src = torch.from_numpy(pictures(2, h, w, seed=2)).to(DEV)
    dst = torch.full((2, oh, ow, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f = torch.zeros(2, 3, oh, ow, device=DEV)
    xt, yt = tables(w, ow), tables(h, oh)

    def call(src=src, B=2, h=h, w=w, px=0, py=0, oh=oh, ow=ow, xt=xt, yt=yt, dst=dst, pitch=3 * ow, ss=3 * ow * oh, f1=f, f2=None):
        ctx.resize_bilinear(src, B, h, w, 3 * w, 3 * w * h, px, py, oh, ow, xt, yt, dst, pitch, ss, f1, f2)

    call()  # (the baseline is valid)
    torch.cuda.synchronize()
    before = ctx.lib.upk_kernel_launches(ctx.h, 0)
    bad = [dict(src=None), dict(dst=None, f1=None), dict(B=0), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=0), dict(px=-1),
           dict(py=-1), dict(xt=None), dict(yt=None), dict(xt=(xt[0], None, xt[2])), dict(yt=(None, yt[1], yt[2])),
           dict(xt=(xt[0], xt[1], 0)), dict(yt=(yt[0], yt[1], -3)), dict(pitch=3 * ow - 1), dict(ss=3 * ow * oh - 1)]
    for kw in bad:
        with pytest.raises(_lib.UpkError) as e:
            call(**kw)
        assert e.value.code == -1, kw  # UPK_EINVAL
    # a row of 30000 pixels: 90000 bytes, not one staged row fits the 64 KiB band (no pass needs a table: 1 x 30000 as is)
    with pytest.raises(_lib.UpkError) as e:
        call(h=1, w=30000, oh=1, ow=30000, xt=None, yt=None, pitch=90000, ss=90000)
    assert e.value.code == -2  # UPK_ESHAPE
    # 9 staged rows of one output row at 3 * 3000 bytes each do not fit either
    y9 = tables(4 * 2, 2)
    assert y9[2] == 9
    with pytest.raises(_lib.UpkError) as e:
        call(h=8, w=3000, oh=2, ow=3000, xt=None, yt=y9, pitch=9000, ss=18000)
    assert e.value.code == -2
    assert ctx.lib.upk_kernel_launches(ctx.h, 0) == before
    torch.cuda.synchronize()
    assert bool((dst.cpu() != SENTINEL).any())  # (the baseline call wrote; the refused ones could not be told apart here)


def host_band(in_h, out_h, out_w, yksize):
    """The launcher's band rule as include/upk.h states it: (output rows per workgroup, staged rows allocated).  cap rows of
    3 * out_w bytes fit 64 KiB; a band of bh rows of a resampling table reads at most ceil((bh - 1) in / out) + yksize rows;
    bh starts at 8 and shrinks until that fits."""
    cap = 65536 // (3 * out_w)
    span = lambda bh: -(-(bh - 1) * in_h // out_h) + yksize
    bh = min(8, out_h)
    while bh > 1 and span(bh) > cap:
        bh -= 1
    return bh, max(min(span(bh), cap), yksize)


@pytest.mark.parametrize("w", [1000, 999])
def test_tables_outside_the_resampling_geometry_go_row_by_row(ctx, w):
    """The band is sized for tables of the resampling geometry.  A valid table whose rows read far apart (output rows
    alternate between the top and the bottom of the picture) spans more rows than the band's allocation: the workgroup
    then stages one output row at a time, with the same integer arithmetic.  64 -> 32 rows at 1000 (dword stores) and
    999 (per pixel) pixels: the host keeps bands of 8 output rows with 17 staged rows, every band of this table spans
    all 64 input rows."""
    h, oh = 64, 32
    bh, rows = host_band(h, oh, w, 3)
    assert (bh, rows) == (8, 17)
    bounds = np.array([[0 if y % 2 == 0 else h - 3, 3] for y in range(oh)], dtype=np.int32)
    for y0 in range(0, oh, bh):  # the branch under test: every band's real span exceeds what is staged at once
        band = bounds[y0:y0 + bh]
        assert int((band[:, 0] + band[:, 1]).max() - band[:, 0].min()) == h > rows
    k = np.tile(np.array([1 << 20, 1 << 21, 1 << 20], dtype=np.int32), (oh, 1))
    k[1::2] = np.array([1 << 21, 1 << 20, 1 << 20], dtype=np.int32)  # (rows differ in weights too)
    prepare.validate_table((bounds, k, 3), h, oh)
    pics = pictures(2, h, w, seed=3)
    want_u8 = np.stack([rr.one_pass(p, bounds, k, 0) for p in pics])
    src = torch.from_numpy(pics).to(DEV)
    dst = torch.full((2, oh, w, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f2 = torch.zeros(2, oh, w, 3, device=DEV)
    ctx.resize_bilinear(src, 2, h, w, 3 * w, 3 * w * h, 0, 0, oh, w, None, (torch.from_numpy(bounds).to(DEV),
                        torch.from_numpy(k).to(DEV), 3), dst, 3 * w, 3 * w * oh, None, f2)
    torch.cuda.synchronize()
    check("row by row w=%d" % w, (dst.cpu().numpy(), None, f2.cpu().numpy()), (None, rr.to_lr(want_u8), want_u8))


def test_graph_replay_gives_the_same_bytes(ctx):
    """One launch captured on a side stream (a single chain) replays to the eager bytes."""
    h, w, pad, oh, ow, B = CASES["dataset_pad8"]
    pics = pictures(B, h, w, seed=11)
    src = torch.from_numpy(pics).to(DEV)
    want = rr.lr_transform(pics, (oh, ow), pad)
    xt, yt = tables(w + 2 * pad[0], ow), tables(h, oh)
    dst = torch.full((B, oh, ow, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f1 = torch.zeros(B, 3, oh, ow, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.graph_begin()
        ctx.resize_bilinear(src, B, h, w, src.stride(1), src.stride(0), pad[0], pad[1], oh, ow, xt, yt, dst, dst.stride(1),
                            dst.stride(0), f1, None)
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
    assert np.array_equal(first, want[2]) and np.array_equal(dst.cpu().numpy(), want[2])
    assert np.array_equal(bits(f1.cpu().numpy()), bits(want[0]))


def test_torch_cuda_graph_replay_gives_the_same_bytes(ctx):
    """The same launch captured by torch.cuda.graph (a single chain, nothing else in the capture; the tables are on the
    device before it begins) replays to the eager bytes."""
    h, w, pad, oh, ow, B = CASES["demo_pad4_5taps"]
    pics = pictures(B, h, w, seed=12)
    src = torch.from_numpy(pics).to(DEV)
    want = rr.lr_transform(pics, (oh, ow), pad)
    xt, yt = tables(w + 2 * pad[0], ow), tables(h, oh)
    dst = torch.full((B, oh, ow, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f2 = torch.zeros(B, oh, ow, 3, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.resize_bilinear(src, B, h, w, src.stride(1), src.stride(0), pad[0], pad[1], oh, ow, xt, yt, dst, dst.stride(1),
                            dst.stride(0), None, f2)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())  # (captured, not run)
    for _ in range(2):
        dst.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want[2]) and np.array_equal(bits(f2.cpu().numpy()), bits(want[1]))
