"""The host half of the test split's loader (upgpt_amd/data.py): the NEAREST index tables against Pillow, the look-up tables
against tests/batch_ref.py, names and index building, key order, and everything that is refused.  No GPU."""
import csv
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import batch_ref as br
from upgpt_amd import _lib, build, data, evaluate, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_KEYS = ["image", "txt", "fname", "src_image", "styles", "smpl", "smpl_image", "person_mask"]


@pytest.mark.parametrize("in_size,out_size", br.NEAREST_PAIRS)
def test_nearest_table_is_pillows(in_size, out_size):
    tab = data.nearest_table(in_size, out_size)
    assert tab.dtype == np.int32 and tab.shape == (out_size,)
    assert np.array_equal(tab, br.nearest_index(in_size, out_size))
    data.validate_table(tab, in_size)
    # ... on bytes too, both axes at once
    pic = np.random.default_rng(in_size).integers(0, 256, (in_size, in_size), dtype=np.uint8)
    assert np.array_equal(pic[tab][:, tab], br.resize(pic, (out_size, out_size), Image.NEAREST))


def test_the_closed_form_is_not_pillows_at_256_to_24():
    """floor((i + 0.5) * in / out) is the tempting simplification; Pillow accumulates xo += a instead, and at 256 -> 24, a
    256-wide mask meeting a 24-wide latent, the two differ."""
    closed = np.floor((np.arange(24) + 0.5) * 256 / 24).astype(np.int64)
    pil = br.nearest_index(256, 24)
    assert not np.array_equal(closed, pil)
    assert np.array_equal(data.nearest_table(256, 24), pil)


def test_table_validation():
    with pytest.raises(ValueError, match="leaves the 4-sample axis"):
        data.validate_table(np.array([0, 4], dtype=np.int32), 4)
    with pytest.raises(ValueError, match="leaves"):
        data.validate_table(np.array([-1, 2], dtype=np.int32), 4)
    with pytest.raises(ValueError, match="positive"):
        data.nearest_table(0, 4)


def test_mask_lut_and_the_two_bbox_values():
    lut = data.mask_lut()
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = br.person_mask(ramp, (16, 16), 'mask').numpy().reshape(-1)
    assert lut.dtype == np.float32 and np.array_equal(lut.view(np.uint32), want.view(np.uint32))
    m = np.zeros((16, 12), dtype=np.uint8)
    m[3:9, 2:7] = 255
    box = br.person_mask(m, (4, 3), 'bbox').numpy()
    assert sorted(set(box.reshape(-1).tolist())) == [float(np.float32(inference.MASK_BG)), float(np.float32(inference.MASK_FG))]
    assert lut[0] == np.float32(inference.MASK_BG) and lut[1] == np.float32(inference.MASK_FG)


@pytest.mark.parametrize("segmenter", ["lip", "mm"])
@pytest.mark.parametrize("config", sorted(br.LOSS_WEIGHTS))
def test_loss_lut(segmenter, config):
    weights = br.known_weights(br.LOSS_WEIGHTS[config], segmenter)
    lut = data.loss_lut(weights, segmenter)
    labels = np.arange(256, dtype=np.uint8).reshape(16, 16)
    n = len(br.label2id(segmenter))
    labels[labels >= n] = 0  # (the restatement's table stops at the last label)
    want = br.get_mask(labels, weights, segmenter).reshape(-1)
    assert np.array_equal(lut[labels.reshape(-1)].view(np.uint32), want.view(np.uint32))
    assert bool((lut[n:] == 1.0).all())
    if segmenter == "mm":  # the configs name LIP labels the MultiModal table does not have
        with pytest.raises(ValueError, match="left-arm"):
            data.loss_lut(br.LOSS_WEIGHTS[config], segmenter)


def test_mode_f_pictures_pass_nearest_and_to_tensor_unchanged():
    w = np.array([[0.2, 0.5, 2.0, 8.0, 1.0, 0.30000001192092896]], dtype=np.float32).repeat(6, 0)
    out = br.to_tensor(br.resize(w, (3, 6), Image.NEAREST)).numpy()
    assert out.dtype == np.float32 and np.array_equal(out[0].view(np.uint32), w[:3].view(np.uint32))


def test_smpl_mean_expression_on_a_grid_of_byte_triples():
    """torch.mean(x, 0) * 2. - 1. of three channels is fl(fl(fl(fl(r + g) + b) / 3) * 2 - 1), and NOT the multiply by
    fl(1 / 3)."""
    v = np.arange(0, 256, 5, dtype=np.uint8)
    r, g, b = (t.reshape(-1) for t in np.meshgrid(v, v, v, indexing="ij"))
    x = br.to_tensor(np.stack([r, g, b], -1)[None])  # [3, 1, n]
    want = (torch.mean(x, 0, keepdim=True) * 2. - 1.).numpy().reshape(-1)
    f = [t.astype(np.float32) / np.float32(255) for t in (r, g, b)]
    s = (f[0] + f[1]) + f[2]
    assert np.array_equal((s / np.float32(3) * np.float32(2) - np.float32(1)).view(np.uint32), want.view(np.uint32))
    assert not np.array_equal((s * np.float32(1 / 3) * np.float32(2) - np.float32(1)).view(np.uint32), want.view(np.uint32))


def test_names():
    src, dst = 'WOMEN/Blouses_Shirts/id_00003115/01_7_additional.jpg', 'WOMEN/Blouses_Shirts/id_00003115/01_2_side.jpg'
    long_name = 'fashionWOMENBlouses_Shirtsid0000311501_7additional___fashionWOMENBlouses_Shirtsid0000311501_2side'
    assert data.convert_fname(src) == long_name.split('___')[0] == br.convert_fname(src)
    assert data.get_name(src, dst) == long_name == br.get_name(src, dst)
    assert inference.convert_fname(long_name) == [src[:-4], dst[:-4]]  # (generate_utils' function is the inverse)
    assert data.style_names == br.STYLE_NAMES


def test_alias_of_the_reference_import_path(tmp_path):
    from ldm.data import deepfashion_inshop as di
    assert di.DeepFashionPair is data.DeepFashionPair and di.DeepFashionSample is data.DeepFashionSample
    assert di.get_name is data.get_name and di.convert_fname is data.convert_fname and di.style_names is data.style_names
    (tmp_path / "a" / "b").mkdir(parents=True)
    (tmp_path / "a" / "c").mkdir()
    assert sorted(di.list_subdirectories(str(tmp_path))) == [str(tmp_path / "a" / "b"), str(tmp_path / "a" / "c")]
    assert callable(evaluate.run_split)


def test_index_building(tmp_path):
    kw = br.make_tree(tmp_path)
    ds = data.DeepFashionPair(**kw)
    ref = br.RefPair(**kw)
    assert len(ds) == len(ref) == 5
    assert ds.pairs == [(r['from'], r['to']) for r in ref.df]  # two pair files, in order
    assert ds.pairs[3] == (br.image_name(3), br.image_name(4))
    assert ds.vae_z_size == (32, 24) and data.DeepFashionPair(**kw, image_size=[64, 48], f=8).vae_z_size == (8, 6)
    kept = data.DeepFashionPair(**kw, df_filter="keep")
    assert kept.pairs == [p for p in ds.pairs if p[0] != br.image_name(1)] and len(kept) == 4
    men = data.DeepFashionPair(**kw, men_factor=2)
    extra = [p for p in ds.pairs if p[0].startswith("MEN/")]
    assert len(extra) == 2 and men.pairs == ds.pairs + extra + extra
    one = data.DeepFashionPair(**dict(kw, pair_file=kw["pair_file"][1]))  # a single path
    assert one.pairs == ds.pairs[3:]
    assert ds.texts[ds.map[br.image_name(0)]['text']].startswith("a person")
    with pytest.raises(ValueError, match="no column"):
        data.DeepFashionPair(**kw, df_filter="nope")


def test_max_size_takes_sklearns_subset(tmp_path):
    kw = br.make_tree(tmp_path)
    try:
        from sklearn import model_selection
    except ImportError:  # the import is lazy, and its absence is said so
        with pytest.raises(ImportError, match="sklearn is not installed"):
            data.DeepFashionPair(**kw, max_size=2, test_split_seed=7)
        return
    ds = data.DeepFashionPair(**kw, max_size=2, test_split_seed=7)
    full = data.DeepFashionPair(**kw).pairs
    _, want = model_selection.train_test_split(full, test_size=2, random_state=7)
    assert ds.pairs == [tuple(p) for p in want] and len(ds) == 2


def test_key_order():
    """test_step passes N = len(batch): the key set is part of the interface."""
    mk = lambda cls, **kw: cls.batch_keys(SimpleNamespace(**dict(dict(image_only=False, loss_weight=None), **kw)))
    assert list(mk(data.DeepFashionPair)) == PAIR_KEYS
    assert list(mk(data.DeepFashionPair, loss_weight={"face": 2.0})) == PAIR_KEYS + ["loss_w"]
    assert list(mk(data.DeepFashionPair, image_only=True)) == ["image", "txt"]
    assert list(mk(data.DeepFashionSample)) == ["src_image", "styles", "image", "txt", "smpl", "smpl_image", "person_mask"]


@pytest.mark.parametrize("kw", [dict(dropout=0.1), dict(random_style=True), dict(shuffle=True), dict(resize_size=256),
                                dict(pad=[8, 0])])
def test_refused_keywords(kw, tmp_path):
    with pytest.raises(NotImplementedError, match=list(kw)[0]):
        data.DeepFashionPair(str(tmp_path), "img_256", [], "map.csv", **kw)
    assert list(kw)[0] in data.DeepFashionPair.__doc__


def test_other_constructor_errors(tmp_path):
    kw = br.make_tree(tmp_path)
    with pytest.raises(ValueError, match="input_mask_type"):
        data.DeepFashionPair(**kw, input_mask_type="box")
    with pytest.raises(TypeError, match="unknown keywords"):
        data.DeepFashionPair(**kw, colour="red")
    with pytest.raises(ValueError, match="left-arm"):
        data.DeepFashionPair(**kw, loss_weight=br.LOSS_WEIGHTS["mm_512"])


def _first_batch(ds):
    return next(iter(ds.batches(2)))


def _gpu_or_value_error(ds, match):
    with pytest.raises(ValueError, match=match):
        _first_batch(ds)


def test_every_unloadable_sample_raises_value_error_naming_it(tmp_path):
    """What the reference would silently replace by the next sample.  Every check runs on the host, before a device is
    needed, so the errors are the same with and without a GPU."""
    kw = br.make_tree(tmp_path / "t")
    root = tmp_path / "t"
    n0, n1 = br.image_name(0), br.image_name(1)
    stem1 = n1[:-4]
    # a missing picture
    os.rename(root / "img_256" / n1, root / "img_256" / "moved.jpg")
    _gpu_or_value_error(data.DeepFashionPair(**kw), "cannot read the picture .*" + os.path.basename(n1))
    # a picture of another size than its batch
    Image.fromarray(np.zeros((32, 48, 3), dtype=np.uint8)).save(str(root / "img_256" / n1))
    _gpu_or_value_error(data.DeepFashionPair(**kw), "first picture of its batch")
    os.replace(root / "img_256" / "moved.jpg", root / "img_256" / n1)
    # an RGB mask
    mask_file = root / "smpl_256" / (stem1 + "_mask.png")
    good = Image.open(str(mask_file)).copy()
    good.convert("RGB").save(str(mask_file))
    _gpu_or_value_error(data.DeepFashionPair(**kw, input_mask_type="bbox"), "2-D uint8 map")
    # an all-zero mask: refused in bbox mode only
    Image.fromarray(np.zeros((64, 64), dtype=np.uint8)).save(str(mask_file))
    _gpu_or_value_error(data.DeepFashionPair(**kw, input_mask_type="bbox"), os.path.basename(str(mask_file)) + ".*no non-zero pixel")
    good.save(str(mask_file))
    # an empty `styles` cell
    rows = br.read_csv(kw["data_file"])
    rows[0]["styles"] = ""
    with open(kw["data_file"], "w", newline='') as f:
        wr = csv.DictWriter(f, list(rows[0]))
        wr.writeheader()
        wr.writerows(rows)
    _gpu_or_value_error(data.DeepFashionPair(**kw), "empty `styles` cell")
    # an image the map file does not have
    with open(kw["pair_file"][0], "a") as f:
        f.write("MEN/x/id_1/01_1_front.jpg,%s,True\n" % n0)
    with pytest.raises(ValueError, match="not in the map file"):
        next(iter(data.DeepFashionPair(**kw).batches(1, start=3, stop=4)))


def test_a_missing_style_file_is_no_error_and_nothing_runs_without_a_gpu(tmp_path):
    """The tree lacks (image 1, hair) and every 'accesories': loading passes all host checks and stops where the device is
    needed."""
    kw = br.make_tree(tmp_path)
    assert not (tmp_path / "styles" / br.image_name(1)[:-4] / "hair.jpg").exists()
    if torch.cuda.is_available():  # (with a device the same call simply succeeds; tests/test_batch_gpu.py looks at the values)
        assert list(_first_batch(data.DeepFashionPair(**kw))) == PAIR_KEYS
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _first_batch(data.DeepFashionPair(**kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeepFashionPair(**kw)[0]
    m = np.zeros((2, 16, 12), dtype=np.uint8)
    for mode in ("mask", "bbox"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            data.person_mask(m, [4, 3], mode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.person_mask(np.zeros((1, 24, 32, 3), dtype=np.uint8), [3, 4], "smpl")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.loss_weight(m, [4, 3], {"face": 2.0}, "mm")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.clip_normalize(np.zeros((1, 224, 224, 3), dtype=np.uint8))


def test_argument_errors_of_the_low_level_functions():
    m = np.zeros((2, 16, 12), dtype=np.uint8)
    with pytest.raises(ValueError, match="mode"):
        data.person_mask(m, [4, 3], "box")
    with pytest.raises(ValueError, match="size"):
        data.person_mask(m, [4], "mask")
    with pytest.raises(TypeError, match="uint8"):
        data.person_mask(m.astype(np.float32), [4, 3], "mask")
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        data.person_mask(m[0], [4, 3], "mask")
    with pytest.raises(ValueError, match="left-arm"):
        data.loss_weight(m, [4, 3], {"left-arm": 2.0}, "mm")
    with pytest.raises(TypeError, match="uint8"):
        data.clip_normalize(np.zeros((1, 224, 224, 3), dtype=np.float32))


def test_entry_points_are_declared_exported_and_built_without_contraction():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    for name in ("upk_cond_bbox_u8", "upk_cond_gather_u8", "upk_cond_smpl_u8", "upk_clip_normalize_u8"):
        assert ("int %s(upk_ctx* ctx" % name) in header and name in _lib.SYMBOLS
        assert hasattr(_lib.load_library(), name)
    assert "batch.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "batch.hip"))
    assert build.FILE_FLAGS["batch.hip"] == ["-ffp-contract=off"]
