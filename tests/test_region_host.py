"""The host side of region-locked editing, no GPU: the guarantees of the arithmetic shown on the numpy
restatement tests/region_ref.py (what the GPU tests compare the kernels with), region_labels, the facade's refusals that
need no device, and the declarations of the new entry points."""
import os

import numpy as np
import pytest
import torch

import region_ref as rr
from upgpt_amd import _lib, edit, styles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 24, 8), (64, 48, 8), (16, 8, 8), (24, 24, 4)]  # (H, W, factor)
DILATE = [0, 1, 3, 9, 40]
FEATHER = [0, 1, 2, 5]
TOP = styles.LIP.label2id['top']


def random_maps(h, w, seed):
    """Three samples: a few rectangles of `top` among other labels, one isolated pixel of it, and none of it."""
    rng = np.random.default_rng(seed)
    segm = rng.integers(0, 20, (3, h, w), dtype=np.uint8)
    segm[segm == TOP] = 0
    y, x = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
    segm[0, y:y + 3, x:x + 2] = TOP
    segm[0, h - 1, w - 1] = TOP
    segm[1, int(rng.integers(0, h)), int(rng.integers(0, w))] = TOP
    return segm


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_keeps_what_it_promises(shape):
    h, w, f = shape
    segm = random_maps(h, w, h * 100 + w)
    rng = np.random.default_rng(h + w)
    orig = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    gen = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    sel = segm == TOP
    for r in DILATE:
        mask, keep, cells = rr.region(segm, [TOP], r, f)
        assert mask.dtype == np.uint8 and keep.dtype == np.float32 and cells.dtype == np.int32
        assert mask.shape == (3, h, w) and keep.shape == (3, 1, h // f, w // f) and cells.shape == (3,)
        assert set(np.unique(mask)) <= {0, 255} and set(np.unique(keep)) <= {0.0, 1.0}
        assert np.array_equal(mask != 0, ~rr.chebyshev_far(sel, r))
        assert np.array_equal(cells, (keep == 0).sum(axis=(1, 2, 3)))
        assert cells[2] == 0 and bool((keep[2] == 1).all()) and not mask[2].any()  # a sample without the label
        assert cells[0] > 0 and cells[1] > 0
        # a kept cell holds no mask pixel, an edited cell at least one
        blocks = (mask != 0).reshape(3, h // f, f, w // f, f).any(axis=(2, 4))
        assert np.array_equal(blocks, keep[:, 0] == 0)
        for fr in FEATHER:
            out, a = rr.composite(orig, gen, mask, fr)
            assert out.dtype == np.uint8 and a.dtype == np.uint8 and out.shape == orig.shape and a.shape == mask.shape
            far = rr.chebyshev_far(sel, r + fr)
            assert not a[far].any() and np.array_equal(out[far], orig[far])  # farther than r + fr: the input's bytes
            assert np.array_equal(out[a == 0], orig[a == 0]) and np.array_equal(out[a == 255], gen[a == 255])
            assert np.array_equal(out[2], orig[2])
            if fr == 0:
                assert np.array_equal(a, mask)
            lo, hi = np.minimum(orig, gen), np.maximum(orig, gen)
            assert bool(((out >= lo) & (out <= hi)).all())


def test_alpha_replicates_the_edges():
    m = np.zeros((6, 7), dtype=np.uint8)
    m[0, 0] = 9  # (any non-zero byte counts)
    a = rr.alpha(m, 1)
    assert a[0, 0] == (255 * 4 + 4) // 9 and a[0, 1] == a[1, 0] == (255 * 2 + 4) // 9 and a[1, 1] == (255 + 4) // 9
    assert not a[2:].any() and not a[:, 2:].any()
    assert bool((rr.alpha(np.full((5, 4), 255, np.uint8), 5) == 255).all())
    assert rr.label_set([0, 31, 32, 255]) == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]


def test_region_labels():
    lip = styles.LIP
    ids = lambda *names: tuple(sorted(lip.label2id[n] for n in names))
    assert edit.region_labels("top") == ids("top", "dress", "jumpsuits", "scarf") == tuple(sorted(lip.group_ids["top"]))
    assert edit.region_labels("label:top") == ids("top") == (TOP,)
    assert edit.region_labels("coat") == ids("coat") and edit.region_labels("outer") == ids("coat")
    assert edit.region_labels(["top", "bottom"]) == ids("top", "dress", "jumpsuits", "scarf", "skirt", "pants")
    assert edit.region_labels(("label:hair", "shoes"), lip) == ids("hair", "left-shoe", "right-shoe", "socks")
    assert edit.region_labels("skin", "mm") == (styles.DEEPFASHION_MM.label2id["skin"],)
    assert edit.region_labels("top", "mm") == (styles.DEEPFASHION_MM.label2id["top"],)  # (no such group there: the label)
    for bad in ("trousers", "label:bottom", "", [], ["top", "nope"], None, 5, ["top", 3]):
        with pytest.raises(ValueError, match="groups: face, background.*labels: background, hat"):
            edit.region_labels(bad)
    with pytest.raises(ValueError, match="segmenter"):
        edit.region_labels("top", "coco")


def test_facade_refusals_need_no_device():
    segm = np.zeros((2, 16, 8), dtype=np.uint8)
    pics = np.zeros((2, 16, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="unknown region"):
        edit.region_mask(segm, "sleeve")
    with pytest.raises(TypeError, match="segm must be uint8"):
        edit.region_mask(segm.astype(np.int32), "top")
    with pytest.raises(TypeError, match="segm must be a uint8 tensor"):
        edit.region_mask([[1]], "top")
    with pytest.raises(ValueError, match=r"segm must be \[B, H, W\]"):
        edit.region_mask(segm[0], "top")
    with pytest.raises(ValueError, match="dilate"):
        edit.region_mask(segm, "top", dilate=33)
    with pytest.raises(ValueError, match="dilate"):
        edit.region_mask(segm, "top", dilate=-1)
    with pytest.raises(ValueError, match="factor"):
        edit.region_mask(segm, "top", factor=3)
    with pytest.raises(ValueError, match="multiple of factor"):
        edit.region_mask(segm, "top", factor=16)
    with pytest.raises(TypeError, match="gen must be uint8"):
        edit.composite(pics, pics.astype(np.float32), segm)
    with pytest.raises(ValueError, match=r"orig must be \[B, H, W, 3\]"):
        edit.composite(pics[0], pics, segm)
    with pytest.raises(ValueError, match="3-channel"):
        edit.composite(np.zeros((2, 16, 8, 4), np.uint8), np.zeros((2, 16, 8, 4), np.uint8), segm)
    with pytest.raises(ValueError, match="do not match"):
        edit.composite(pics, pics[:1], segm)
    with pytest.raises(ValueError, match="do not match"):
        edit.composite(pics, pics, segm[:, :8])
    with pytest.raises(ValueError, match="feather"):
        edit.composite(pics, pics, segm, feather=17)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            edit.region_mask(segm, "top")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            edit.composite(pics, pics, segm)


def test_edit_region_refusals_need_no_device():
    from upgpt_amd.inference import InferenceModel

    class Model:
        num_downs, image_size = 3, [32, 24]

    m = object.__new__(InferenceModel)
    m.device, m.model = "cpu", Model()
    pic, segm = np.zeros((256, 192, 3), np.uint8), np.zeros((256, 192), np.uint8)
    with pytest.raises(ValueError, match="unknown region"):
        m.edit_region(pic, segm, "sleeve", {})
    with pytest.raises(ValueError, match="the model works on 256 x 192"):
        m.edit_region(pic[:128], segm[:128], "top", {})
    with pytest.raises(ValueError, match="does not match"):
        m.edit_region(pic, segm[:, :100], "top", {})
    with pytest.raises(ValueError, match="at most 8"):
        m.edit_region(np.zeros((9, 256, 192, 3), np.uint8), np.zeros((9, 256, 192), np.uint8), "top", {})
    with pytest.raises(ValueError, match="feather"):
        m.edit_region(pic, segm, "top", {}, feather=40)
    with pytest.raises(TypeError, match="picture must be uint8"):
        m.edit_region(pic.astype(np.float32), segm, "top", {})


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    for name in ("upk_region_mask_u8", "upk_composite_u8"):
        assert ("int %s(upk_ctx* ctx" % name) in header and name in _lib.SYMBOLS
        assert hasattr(_lib.load_library(), name)
    assert callable(_lib.Context.region_mask) and callable(_lib.Context.composite)
    assert "region.hip" in __import__("upgpt_amd.build", fromlist=["SOURCES"]).SOURCES
    from upgpt_amd.ddpm import LatentDiffusion
    from upgpt_amd.inference import InferenceModel
    assert callable(LatentDiffusion.edit_images) and callable(InferenceModel.edit_region)
