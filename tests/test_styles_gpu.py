"""upk_segm_boxes_u8 and upk_style_crops_u8 on the MI355X against tests/styles_ref.py (pinned to Pillow and to the reference's
rules by tests/test_styles_host.py): EQUAL ON EVERY BYTE, EVERY FLOAT BIT AND EVERY BOX INTEGER.  No tolerance anywhere: the
boxes are integer minima, maxima and sums, both resampling passes are integer arithmetic on coefficients specified operation
by operation in double, and the normalisation is three correctly rounded fp32 operations in a fixed order.  Pictures are
random bytes; the label maps are built by hand (tests/styles_ref.py) and the host tests assert what each of them holds."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import styles_ref as sr
from upgpt_amd import _lib, evaluate, prepare, styles
from upgpt_amd.inference import CLIP_MEAN, CLIP_STD, InferenceModel, get_empty_style, style_names

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
GUARD = 4096  # sentinel bytes before and after every destination
FIXTURES = {"lip_64x48": (sr.lip_64x48, 'lip'), "mm_37x29": (sr.mm_37x29, 'mm'), "lip_300x260_128": (lambda: sr.lip_300x260(128), 'lip'),
            "lip_300x260_129": (lambda: sr.lip_300x260(129), 'lip'), "lip_1101x750": (sr.lip_1101x750, 'lip')}
_cache = {}


def fixture(name):
    """(pictures, label maps, segmenter name, the restatement's (styles, valid, bytes), its boxes): computed once, shared."""
    if name not in _cache:
        make, segmenter = FIXTURES[name]
        pics, segm = make()
        _cache[name] = (pics, segm, segmenter, sr.styles(pics, segm, segmenter), sr.boxes(pics, segm, segmenter))
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(tag, got, want):
    """got / want = (styles, valid, bytes); prints the counts, then asserts equality of every element."""
    g_f, g_v, g_u = (None if t is None else (t.cpu().numpy() if torch.is_tensor(t) else t) for t in got)
    w_f, w_v, w_u = want
    bad = (int((g_u != w_u).sum()) if g_u is not None else -1, int((bits(g_f) != bits(w_f)).sum()) if g_f is not None else -1,
           int((g_v != w_v).sum()))
    print("%s: %d bytes, %d floats, %d valid flags differ (-1: not asked) of %d bytes" % (tag, bad[0], bad[1], bad[2], w_u.size))
    assert all(b <= 0 for b in bad), tag


def strided(pics, segm):
    """Device views of larger stores: an odd base address, a row pitch above the row, every second sample."""
    b, h, w = segm.shape
    big_p = torch.full((2 * b, h + 3, w + 5, 3), 7, dtype=torch.uint8, device=DEV)
    big_s = torch.full((2 * b, h + 2, w + 9), 14, dtype=torch.uint8, device=DEV)  # (14 is MM's `face`: it must not be read)
    vp, vs = big_p[::2, 2:2 + h, 3:3 + w], big_s[1::2, 1:1 + h, 5:5 + w]
    vp.copy_(torch.from_numpy(pics))
    vs.copy_(torch.from_numpy(segm))
    assert vp.data_ptr() % 4 and vs.data_ptr() % 4 and not vp.is_contiguous() and not vs.is_contiguous()
    assert vp.stride(1) > 3 * w and vs.stride(1) > w and vp.stride(0) > h * vp.stride(1)
    return vp, vs


@pytest.mark.parametrize("name", list(FIXTURES))
def test_boxes_equal_the_restatement(name):
    pics, segm, segmenter, _, want = fixture(name)
    got = styles.style_boxes(torch.from_numpy(pics).to(DEV), torch.from_numpy(segm).to(DEV), segmenter)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    print("%s: %d of %d box integers differ" % (name, int((got != want).sum()), want.size))
    assert np.array_equal(got, want)
    if name == "mm_37x29":
        vp, vs = strided(pics, segm)
        assert np.array_equal(styles.style_boxes(vp, vs, segmenter).cpu().numpy(), want)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_crops_equal_the_restatement_on_every_byte_and_float_bit(name):
    pics, segm, segmenter, want, _ = fixture(name)
    if name == "mm_37x29":  # odd sizes, strided views of larger buffers, unaligned base
        src = strided(pics, segm)
    else:
        src = torch.from_numpy(pics).to(DEV), torch.from_numpy(segm).to(DEV)
    got = styles.style_crops(src[0], src[1], segmenter, out_u8=True)
    assert got[0].shape == (len(pics), 9, 3, 224, 224) and got[0].dtype == torch.float32 and got[0].is_contiguous()
    assert got[1].shape == (len(pics), 9) and got[1].dtype == torch.int32 and got[2].shape == (len(pics), 9, 224, 224, 3)
    check(name, got, want)
    assert np.array_equal(bits(sr.clip_norm(got[2].cpu().numpy())), bits(got[0].cpu().numpy()))  # the floats are the bytes' finishing
    if name == "lip_300x260_129":
        assert want[1][0, 0] == 0 and fixture("lip_300x260_128")[3][1][0, 0] == 1  # the face rule, 129 beside 128 rows
    if name == "lip_64x48":  # host arrays are uploaded; the fp32 output alone is the same floats
        alone = styles.style_crops(pics, segm, segmenter)
        assert alone[2] is None
        check(name + " (host arrays, fp32 only)", alone, want)


def raw_call(ctx, pics, segm, seg, slots, coeff=False, guard=GUARD):
    """The two launches through the C ABI with every destination inside a sentinel-filled store -> dict of host arrays plus the
    stores' guard verdict."""
    b, h, w = segm.shape
    n_g, n_s = len(seg.names), len(slots)
    sizes = {"boxes": b * n_g * 8 * 4, "u8": b * n_s * 224 * 224 * 3, "f32": b * n_s * 3 * 224 * 224 * 4, "valid": b * n_s * 4,
             "coeff": b * n_s * 2 * 224 * (2 + styles.COEFF_TAPS) * 4}
    store = {k: torch.full((guard + n + guard,), SENTINEL, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    view = {k: store[k][guard:guard + n] for k, n in sizes.items()}
    p, s = torch.from_numpy(pics).to(DEV), torch.from_numpy(segm).to(DEV)
    ctx.segm_boxes(s, s.stride(1), s.stride(0), p, p.stride(1), p.stride(0), b, h, w, seg.label_groups, n_g, view["boxes"])
    ctx.style_crops(p, p.stride(1), p.stride(0), s, s.stride(1), s.stride(0), b, h, w, seg.label_groups, n_g, view["boxes"],
                    seg.group_flags, seg.slot_groups(slots), list(CLIP_MEAN) + list(CLIP_STD), view["u8"], view["f32"],
                    view["valid"], view["coeff"] if coeff else None)
    torch.cuda.synchronize()
    out = {"boxes": view["boxes"].cpu().numpy().view(np.int32).reshape(b, n_g, 8),
           "u8": view["u8"].cpu().numpy().reshape(b, n_s, 224, 224, 3),
           "f32": view["f32"].cpu().numpy().view(np.float32).reshape(b, n_s, 3, 224, 224),
           "valid": view["valid"].cpu().numpy().view(np.int32).reshape(b, n_s),
           "coeff": view["coeff"].cpu().numpy().view(np.int32).reshape(b, n_s, 2, 224, 2 + styles.COEFF_TAPS)}
    out["guards"] = {k: bool((store[k][:guard] == SENTINEL).all() and (store[k][guard + sizes[k]:] == SENTINEL).all()) for k in sizes}
    return out


def expected_coeffs(in_size, out_size, offset):
    """[224, 18] records (first tap, taps, k[16]) of output indices offset .. offset + 223 from prepare.resample_coeffs."""
    want = np.zeros((224, 2 + styles.COEFF_TAPS), dtype=np.int32)
    t = prepare.resample_coeffs(in_size, out_size)
    if t is None:  # a skipped pass: the single tap that returns the byte
        want[:, 0], want[:, 1], want[:, 2] = np.arange(224) + offset, 1, 1 << 22
        return want
    bounds, k, ksize = t
    assert ksize <= styles.COEFF_TAPS
    want[:, :2] = bounds[offset:offset + 224]
    want[:, 2:2 + ksize] = k[offset:offset + 224]
    return want


@pytest.mark.parametrize("name", ["lip_64x48", "lip_300x260_128", "lip_1101x750"])
def test_coeff_out_equals_resample_coeffs_and_nothing_is_written_outside(ctx, name):
    """The tables the kernel built in double for the rows and columns it produces are prepare.resample_coeffs' (pinned to
    Pillow by tests/test_resize_host.py) for the sizes the boxes imply; the same call shows the destinations' surroundings
    untouched and the raw ABI results equal to the restatement."""
    pics, segm, segmenter, want, want_boxes = fixture(name)
    seg = styles.get_segmenter(segmenter)
    out = raw_call(ctx, pics, segm, seg, style_names, coeff=True)
    print(name, "guards", out["guards"])
    assert all(out["guards"].values())
    assert np.array_equal(out["boxes"], want_boxes)
    check(name + " (C ABI)", (out["f32"], out["valid"], out["u8"]), want)
    b, h, w = segm.shape
    for i in range(b):
        for s, slot in enumerate(style_names):
            if not want[1][i, s]:
                assert not out["coeff"][i, s].any(), (i, slot)
                continue
            (ph, oh, cy), (pw, ow, cx) = sr.implied_sizes(want_boxes[i, seg.names.index(slot)], slot, h, w)
            bad_y = int((out["coeff"][i, s, 0] != expected_coeffs(ph, oh, cy)).sum())
            bad_x = int((out["coeff"][i, s, 1] != expected_coeffs(pw, ow, cx)).sum())
            print("%s sample %d %s: rows %d -> %d at %d: %d differ; columns %d -> %d at %d: %d differ" % (
                name, i, slot, ph, oh, cy, bad_y, pw, ow, cx, bad_x))
            assert bad_y == 0 and bad_x == 0, (i, slot)


def test_a_picture_gives_the_same_bits_alone_and_in_a_batch():
    pics, segm, segmenter, want, _ = fixture("lip_64x48")
    whole = styles.style_crops(pics, segm, segmenter, out_u8=True)
    alone = styles.style_crops(pics[2:3], segm[2:3], segmenter, out_u8=True)
    for a, w in zip(alone, whole):
        assert torch.equal(a[0], w[2])
    check("alone", alone, tuple(t[2:3] for t in want))


def test_empty_slots_and_invalid_crops_hold_the_empty_style():
    pics, segm, segmenter, want, _ = fixture("lip_64x48")
    got_f, got_v, got_u = (t.cpu().numpy() for t in styles.style_crops(pics, segm, segmenter, out_u8=True))
    empty = sr.clip_norm(np.zeros((224, 224, 3), dtype=np.uint8))  # clip_norm(torch.zeros(3, 224, 224)) of the datasets
    demo = get_empty_style().to(torch.float32).numpy()  # the demo's float64 expression, cast as mix_style casts it
    slot = style_names.index
    cases = [(0, slot('accesories')), (2, slot('accesories')), (0, slot('headwear')), (0, slot('shoes'))]  # empty slot, one row, one column
    for b, s in cases:
        assert got_v[b, s] == 0 and not got_u[b, s].any()
        assert np.array_equal(bits(got_f[b, s]), bits(empty)), (b, s)
        # the float64 expression rounds to the same bits in channels 0 and 1 and to the neighbouring float in channel 2
        assert np.array_equal(bits(got_f[b, s, :2]), bits(demo[:2]))
        assert np.array_equal(bits(got_f[b, s, 2]).astype(np.int64), bits(demo[2]).astype(np.int64) + 1)
    assert got_v[1, slot('hair')] == 1 and np.array_equal(bits(got_f[1, slot('hair')]), bits(empty))  # valid and black


def test_refusals_launch_nothing(ctx):
    pics, segm, segmenter, _, _ = fixture("mm_37x29")
    seg = styles.get_segmenter(segmenter)
    b, h, w = segm.shape
    p, s = torch.from_numpy(pics).to(DEV), torch.from_numpy(segm).to(DEV)
    boxes = torch.zeros(b, 3, 8, dtype=torch.int32, device=DEV)
    u8 = torch.full((b, 2, 224, 224, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    f32 = torch.zeros(b, 2, 3, 224, 224, device=DEV)
    valid = torch.full((b, 2), -7, dtype=torch.int32, device=DEV)
    ms = list(CLIP_MEAN) + list(CLIP_STD)

    def call_boxes(segm=s, spitch=w, pic=p, ppitch=3 * w, B=b, h=h, w=w, lg=seg.label_groups, G=3, boxes=boxes):
        ctx.segm_boxes(segm, spitch, spitch * h, pic, ppitch, ppitch * h, B, h, w, lg, G, boxes)

    def call_crops(pic=p, ppitch=3 * w, segm=s, spitch=w, B=b, h=h, w=w, lg=seg.label_groups, G=3, boxes=boxes,
                   flags=seg.group_flags, slots=(0, -1), ms=ms, u8=u8, f32=f32, valid=valid):
        ctx.style_crops(pic, ppitch, ppitch * h, segm, spitch, spitch * h, B, h, w, lg, G, boxes, flags, slots, ms, u8, f32, valid)

    call_boxes()  # (the baselines are valid)
    call_crops()
    torch.cuda.synchronize()
    assert bool((u8 != SENTINEL).any()) and valid.cpu().tolist() == [[1, 0]] * b
    before = ctx.lib.upk_kernel_launches(ctx.h, 0)
    wide = [0] * 256
    common = [dict(segm=None), dict(pic=None), dict(lg=None), dict(boxes=None), dict(B=0), dict(h=0), dict(w=-1), dict(G=33),
              dict(G=0), dict(ppitch=3 * w - 1), dict(spitch=w - 1)]
    for kw in common:
        for call in (call_boxes, call_crops):
            with pytest.raises(_lib.UpkError) as e:
                call(**kw)
            assert e.value.code == -1, kw  # UPK_EINVAL
    for kw in (dict(flags=None), dict(slots=None), dict(ms=None), dict(valid=None), dict(u8=None, f32=None), dict(slots=(0, 3)),
               dict(slots=(-2, 0)), dict(slots=(0,) * 33), dict(slots=()), dict(flags=[-1, 0, 0]), dict(ms=ms[:3] + [0.0, 1.0, 1.0])):
        with pytest.raises(_lib.UpkError) as e:
            call_crops(**kw)
        assert e.value.code == -1, kw
    for kw in (dict(h=1345, w=8, ppitch=24, spitch=8), dict(h=8, w=1345, ppitch=3 * 1345, spitch=1345)):  # an oversize picture
        for call in (call_boxes, call_crops):
            with pytest.raises(_lib.UpkError) as e:
                call(lg=wide, **kw)
            assert e.value.code == -2, kw  # UPK_ESHAPE
    assert ctx.lib.upk_kernel_launches(ctx.h, 0) == before


def test_two_launches_per_style_crops(ctx):
    pics, segm, segmenter, _, _ = fixture("mm_37x29")
    p, s = torch.from_numpy(pics).to(DEV), torch.from_numpy(segm).to(DEV)
    styles.style_crops(p, s, segmenter)
    torch.cuda.synchronize()
    n0 = ctx.lib.upk_kernel_launches(ctx.h, 0)
    styles.style_crops(p, s, segmenter, out_u8=True)
    n1 = ctx.lib.upk_kernel_launches(ctx.h, 0)
    styles.style_boxes(p, s, segmenter)
    n2 = ctx.lib.upk_kernel_launches(ctx.h, 0)
    assert (n1 - n0, n2 - n1) == (2, 1)


def test_graph_replay_on_new_label_maps_gives_the_new_crops():
    """Captured once by torch.cuda.graph (after a warm-up call), replayed after the label maps and pictures in the captured
    buffers were replaced: the new answer comes out, so no box found on the host is baked into the capture."""
    pics, segm, segmenter, want, _ = fixture("lip_64x48")
    p = torch.from_numpy(pics[:1]).to(DEV)
    s = torch.from_numpy(segm[:1]).to(DEV)
    styles.style_crops(p, s, segmenter, out_u8=True)  # warm-up: the context and its workspace exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = styles.style_crops(p, s, segmenter, out_u8=True)
    torch.cuda.synchronize()
    for i in (0, 2, 1):
        p.copy_(torch.from_numpy(pics[i:i + 1]))
        s.copy_(torch.from_numpy(segm[i:i + 1]))
        g.replay()
        torch.cuda.synchronize()
        check("replay on sample %d" % i, out, tuple(t[i:i + 1] for t in want))
    assert not np.array_equal(want[2][0], want[2][2])


def test_extract_styles_feeds_mix_style_bitwise_like_the_restatement():
    from upgpt_amd import synth
    from upgpt_amd.clip_image import FrozenClipImageEmbedder2
    pics, segm, segmenter, want, _ = fixture("lip_64x48")
    enc = FrozenClipImageEmbedder2(width=256, layers=2, heads=4, output_dim=768)
    enc.load_state_dict({k: synth.synth_tensor("extra_cond_models.0." + k, tuple(v.shape)) for k, v in enc.state_dict().items()})
    im = object.__new__(InferenceModel)
    im.device, im.clip_image_encoder, im.clip_text_encoder = "cuda", enc.cuda(), None
    s = im.extract_styles(Image.fromarray(pics[0]), Image.fromarray(segm[0]), segmenter)
    assert s.shape == (9, 3, 224, 224) and s.dtype == torch.float32 and s.is_cuda
    styles_equal = np.array_equal(bits(s.cpu().numpy()), bits(want[0][0]))
    got = im.mix_style(s, {}, mask=["hair"])
    ref = im.mix_style(torch.from_numpy(want[0][0].copy()), {}, mask=["hair"])
    emb_equal = np.array_equal(bits(got.float().cpu().numpy()), bits(ref.float().cpu().numpy()))
    print("extract_styles: crops bitwise equal %s, embeddings bitwise equal %s" % (styles_equal, emb_equal))
    assert got.shape == (9, 768) and bool(torch.isfinite(got.float()).all())
    assert styles_equal and emb_equal
    assert torch.equal(im.extract_styles(pics[0], torch.from_numpy(segm[0]).to(DEV), segmenter), im.extract_styles(pics[0], segm[0]))


def _decoded(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return np.asarray(Image.open(io.BytesIO(f.getvalue())).convert("RGB"))


def test_run_styles_writes_the_valid_groups_files(tmp_path):
    pics, segm, segmenter, _, _ = fixture("mm_37x29")
    segm = segm.copy()
    segm[1][segm[1] == sr.MM_LABELS.index('face')] = 0
    segm[1, 5, 3:20] = sr.MM_LABELS.index('face')  # a one-row face: no face.jpg for the second picture
    ids = ["WOMEN/Dresses/id_0001_01_1_front", "MEN/Tees/id_0002_02_4_full"]
    for i, name in enumerate(ids):
        os.makedirs(tmp_path / "img" / os.path.dirname(name), exist_ok=True)
        os.makedirs(tmp_path / "segm" / os.path.dirname(name), exist_ok=True)
        Image.fromarray(pics[i]).save(tmp_path / "img" / (name + ".jpg"))
        Image.fromarray(segm[i]).save(tmp_path / "segm" / (name + "_segm.png"))
    decoded = np.stack([np.asarray(Image.open(tmp_path / "img" / (name + ".jpg")).convert("RGB")) for name in ids])
    want = sr.styles(decoded, segm, 'mm', list(sr.MM_GROUPS))
    assert want[1].tolist() == [[1, 1, 1], [0, 1, 1]]
    assert evaluate.run_styles(tmp_path / "img", tmp_path / "segm", tmp_path / "styles", 'mm') == 2
    for i, name in enumerate(ids):
        d = tmp_path / "styles" / os.path.dirname(name) / os.path.basename(name).replace('_', '/', 1)
        assert sorted(os.listdir(d)) == sorted(k + ".jpg" for g, k in enumerate(sr.MM_GROUPS) if want[1][i, g]), name
        for g, k in enumerate(sr.MM_GROUPS):
            if want[1][i, g]:
                assert np.array_equal(np.asarray(Image.open(d / (k + ".jpg")).convert("RGB")), _decoded(want[2][i, g])), (name, k)
    (tmp_path / "img" / (ids[1] + ".jpg")).unlink()
    with pytest.raises(ValueError, match="id_0002_02_4_full.jpg"):
        evaluate.run_styles(tmp_path / "img", tmp_path / "segm", tmp_path / "styles2", 'mm')
