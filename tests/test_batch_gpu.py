"""The test split's loader on the MI355X (upgpt_amd/data.py, csrc/batch.hip) against tests/batch_ref.py, the restatement of
DeepFashionPair.__getitem__ whose resizes are Pillow's own.  Every comparison is bit for bit (torch.equal on fp32)."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import batch_ref as br
import finish_ref as fr
import upgpt_amd
from upgpt_amd import data, evaluate, synth

pytestmark = pytest.mark.gpu
PAIR_KEYS = ["image", "txt", "fname", "src_image", "styles", "smpl", "smpl_image", "person_mask"]
# (map, latent): the three sizes of the issue (12 and 13 columns: below one 16-byte load; 70 x 130: more than one trip per
# lane, no integer ratio), then widths that are multiples of 16, which take the 16-byte loads of the box pass, the last
# one the dataset's own 64 KB map
SIZES = [((16, 12), (4, 3)), ((37, 13), (5, 3)), ((70, 130), (8, 16)), ((64, 48), (8, 6)), ((256, 256), (32, 24))]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(got, want):
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(bits(got), bits(want))


def strided(arr, pad_rows, pitch, poison):
    """`arr` [B, H, W(, 3)] as a device view into a larger buffer filled with `poison`: row pitch `pitch` elements of the
    second-last axis, pad_rows extra rows per sample."""
    b, h, w = arr.shape[:3]
    big = torch.full((b, h + pad_rows, pitch) + tuple(arr.shape[3:]), poison, dtype=torch.uint8, device="cuda")
    view = big[:, :h, :w]
    view.copy_(torch.from_numpy(arr))
    assert not view.is_contiguous()
    return view


def box_maps(h, w, oh, ow):
    """Nine maps for one call: two rectangles (bytes 255 and 1), a single pixel in each corner, a full map, one pixel that
    NEAREST skips (a box is reported, the output is all background) and an all-zero map."""
    ys, xs = br.nearest_index(h, oh), br.nearest_index(w, ow)
    skip_y = next(y for y in range(1, h - 1) if y not in ys)  # (not a corner: those are maps 2 .. 5)
    skip_x = next(x for x in range(1, w - 1) if x not in xs)
    m = np.zeros((9, h, w), dtype=np.uint8)
    m[0, h // 4:h - 2, 1:w // 2] = 255
    m[1, 1:h // 3 + 1, w // 3:w - 1] = 1
    m[2, 0, 0] = m[3, 0, w - 1] = m[4, h - 1, 0] = 255
    m[5, h - 1, w - 1] = 1
    m[6] = 7
    m[7, skip_y, skip_x] = 255
    return m


@pytest.mark.parametrize("size,latent", SIZES)
def test_bbox_mode(size, latent):
    h, w = size
    m = box_maps(h, w, *latent)
    want = torch.stack([br.bbox_or_background(x, latent) for x in m])
    want_boxes = torch.tensor([br.box_of(x) for x in m], dtype=torch.int32)
    assert want_boxes[7].min() >= 0 and bool((want[7] == -1).all()) and bool((want[8] == -1).all())
    assert want_boxes[8].tolist() == [-1] * 4 and len({tuple(r) for r in want_boxes.tolist()}) == 9
    pitch = (w + 15) // 16 * 16 + 16
    views = {"dense": torch.from_numpy(m).cuda(), "host": m, "view16": strided(m, 2, pitch, 255), "view": strided(m, 3, w + 5, 255)}
    for name, src in views.items():
        got, boxes = data.person_mask(src, latent, 'bbox', return_boxes=True)
        print(name, size, latent, "boxes", boxes.cpu().tolist())
        assert torch.equal(boxes.cpu(), want_boxes), name
        assert same(got, want), name
    assert sorted(set(want.reshape(-1).tolist())) == [-1.0, float(np.float32(-0.99215686))]
    assert same(data.person_mask(views["dense"][:1], latent, 'bbox'), want[:1])  # B = 1, no boxes asked for


@pytest.mark.parametrize("size,latent", SIZES)
def test_mask_mode(size, latent):
    h, w = size
    rng = np.random.default_rng(h * w)
    m = np.stack([(np.arange(h * w) * k % 256).astype(np.uint8).reshape(h, w) for k in (1, 7)] +
                 [rng.integers(0, 256, (h, w), dtype=np.uint8)])
    assert all(len(np.unique(x)) == min(256, h * w) for x in m[:2])
    want = torch.stack([br.person_mask(x, latent, 'mask') for x in m])
    for name, src in {"dense": torch.from_numpy(m).cuda(), "view": strided(m, 3, w + 5, 99)}.items():
        assert same(data.person_mask(src, latent, 'mask'), want), name


@pytest.mark.parametrize("segmenter", ["lip", "mm"])
@pytest.mark.parametrize("config", sorted(br.LOSS_WEIGHTS))
def test_loss_weight(segmenter, config):
    weights = br.known_weights(br.LOSS_WEIGHTS[config], segmenter)
    n = len(br.label2id(segmenter))
    for (h, w), latent in SIZES[:4]:
        segm = np.random.default_rng(n + h).integers(0, n, (3, h, w), dtype=np.uint8)
        segm[0].reshape(-1)[:n] = np.arange(n)  # every label is there
        want = torch.stack([br.loss_w(x, latent, weights, segmenter) for x in segm])
        assert same(data.loss_weight(torch.from_numpy(segm).cuda(), latent, weights, segmenter), want)
        assert same(data.loss_weight(strided(segm, 1, w + 3, 200), latent, weights, segmenter), want)
    assert len(set(want.reshape(-1).tolist())) >= 2


@pytest.mark.parametrize("latent", [(3, 4), (24, 32)])
def test_smpl_mode(latent):
    """24 x 32 pictures: every byte value in each channel next to random bytes in the other two.  At 3 x 4 Pillow's bilinear
    resize runs first; at 24 x 32 it is skipped and all 768 triples of a picture reach the mean."""
    rng = np.random.default_rng(2432)
    pics = rng.integers(0, 256, (3, 24 * 32, 3), dtype=np.uint8)
    for c in range(3):
        pics[:, 256 * c:256 * (c + 1), c] = np.arange(256)
    pics = pics.reshape(3, 24, 32, 3)
    want = torch.stack([br.person_mask(p, latent, 'smpl') for p in pics])
    assert same(data.person_mask(torch.from_numpy(pics).cuda(), latent, 'smpl'), want)
    assert same(data.person_mask(strided(pics, 2, 40, 255), latent, 'smpl'), want)


def test_clip_normalize():
    """Three crops, a distinct ramp per channel (a transposed plane would show), every byte value in every channel; the middle
    crop is invalid and poisoned.  Dense input and an aligned view take the 16-byte path, the odd pitch the bytewise one."""
    y, x = np.mgrid[0:224, 0:224]
    crops = np.stack([np.stack([(x + 37 * c + 5 * y + 11 * n) % 256 for c in range(3)], -1) for n in range(3)]).astype(np.uint8)
    assert all(len(np.unique(crops[..., c])) == 256 for c in range(3))
    assert not np.array_equal(crops[..., 0], crops[..., 1]) and not np.array_equal(crops[0], crops[2])
    crops[1] = 255
    valid = torch.tensor([1, 0, 1], dtype=torch.int32)
    clean = crops.copy()
    clean[1] = 0
    want = br.clip_transform(clean)
    views = {"dense": torch.from_numpy(crops).cuda(), "host": crops, "view16": strided(crops, 6, 240, 255),
             "view": strided(crops, 1, 225, 255)}
    for name, src in views.items():
        assert same(data.clip_normalize(src, valid), want), name
    assert same(data.clip_normalize(views["dense"], valid.cuda())[1], br.clip_transform(np.zeros((224, 224, 3), dtype=np.uint8)))
    assert same(data.clip_normalize(views["dense"][::2]), want[::2])  # no valid: every crop is read
    small = np.random.default_rng(7).integers(0, 256, (2, 10, 7, 3), dtype=np.uint8)  # another size: bytewise
    assert same(data.clip_normalize(small), torch.from_numpy(br.sr.clip_norm(small)))
    wide = np.random.default_rng(8).integers(0, 256, (2, 9, 32, 3), dtype=np.uint8)  # 16-byte path, a last tile of one row
    assert same(data.clip_normalize(wide), torch.from_numpy(br.sr.clip_norm(wide)))


# ---------------------------------------------------------------------------------------------------------------------
# the dataset

def count_d2h(monkeypatch, fn):
    """fn() with every device -> host crossing of a tensor recorded: (method, dtype, elements) per crossing."""
    d2h = []
    T = torch.Tensor

    def moving(name):
        orig = getattr(T, name)

        def f(self, *a, **k):
            out = orig(self, *a, **k)
            if self.is_cuda and not (torch.is_tensor(out) and out.is_cuda):
                d2h.append((name, self.dtype, self.numel()))
            return out
        return f

    orig_copy = T.copy_

    def copy_(self, src, *a, **k):
        if torch.is_tensor(src) and src.is_cuda and not self.is_cuda:
            d2h.append(("copy_", src.dtype, src.numel()))
        return orig_copy(self, src, *a, **k)

    with monkeypatch.context() as mp:
        for name in ("cpu", "to", "numpy", "tolist", "item"):
            mp.setattr(T, name, moving(name))
        mp.setattr(T, "copy_", copy_)
        out = fn()
    return out, d2h


DATASET_CASES = {"bbox": dict(input_mask_type="bbox", loss_weight={"face": 8.0, "background": 0.5}),
                 "mask": dict(input_mask_type="mask"), "smpl": dict(input_mask_type="smpl")}


@pytest.mark.parametrize("case", sorted(DATASET_CASES))
def test_dataset_batches_equal_the_collated_restatement(case, tmp_path, monkeypatch):
    """5 pairs, pictures 64 x 48, latent 8 x 6, masks 64 x 64, smpl pictures 256 x 256 (the centre crop is a real window),
    batches of 2, 2, 1.  float64 smpl parameters in the 'mask' case: the pickle's dtype is kept."""
    kw = dict(br.make_tree(tmp_path, pose_dtype=np.float64 if case == "mask" else np.float32), image_size=[64, 48], f=8,
              **DATASET_CASES[case])
    ds, ref = data.DeepFashionPair(**kw), br.RefPair(**kw)
    keys = PAIR_KEYS + (["loss_w"] if case == "bbox" else [])
    assert len(ds) == 5
    next(iter(ds.batches(2)))  # (the index tables of the sizes in use are uploaded once, here)
    batches, copies = [], []
    it = iter(ds.batches(2))
    for _ in range(3):
        b, d2h = count_d2h(monkeypatch, lambda: next(it))
        batches.append(b)
        copies.append(d2h)
    assert next(it, None) is None and [len(b["fname"]) for b in batches] == [2, 2, 1]
    for b, copy in zip(batches, copies):  # the [B, 4] boxes in 'bbox' mode, and nothing else
        assert copy == ([("cpu", torch.int32, 4 * len(b["fname"]))] if case == "bbox" else []), copy
    for n, b in enumerate(batches):
        want = br.collate([ref[i] for i in range(2 * n, min(2 * n + 2, 5))])
        assert list(b) == keys == list(want)
        for k in keys:
            if torch.is_tensor(want[k]):
                assert b[k].is_cuda and same(b[k], want[k]), (n, k)
            else:
                assert b[k] == want[k], (n, k)
    b0 = batches[0]
    assert b0["image"].shape == (2, 64, 48, 3) and b0["smpl_image"].shape == (2, 256, 192, 3)
    assert b0["styles"].shape == (2, 9, 3, 224, 224) and b0["person_mask"].shape == (2, 1, 8, 6)
    assert b0["smpl"].shape == (2, 1, 85) and b0["smpl"].dtype == (torch.float64 if case == "mask" else torch.float32)
    assert b0["txt"][0].startswith("a person") and batches[1]["txt"][0] == ''  # (pair 2's target has no caption)
    # pair 1's source is image 1, whose hair crop is missing; 'accesories' is missing everywhere
    empty = br.clip_transform(np.zeros((224, 224, 3), dtype=np.uint8))
    hair, acc = br.STYLE_NAMES.index('hair'), br.STYLE_NAMES.index('accesories')
    assert same(b0["styles"][1, hair], empty) and same(b0["styles"][1, acc], empty) and not same(b0["styles"][0, hair], empty)
    # ds[i] is row i of its batch
    one = ds[3]
    assert list(one) == keys
    for k in keys:
        assert same(one[k], batches[1][k][1]) if torch.is_tensor(one[k]) else one[k] == batches[1][k][1], k
    # start / stop
    part = list(ds.batches(2, start=1, stop=2))
    assert len(part) == 1 and part[0]["fname"] == [batches[0]["fname"][1]]


def test_image_only_and_sample_datasets(tmp_path):
    kw = dict(br.make_tree(tmp_path), image_size=[64, 48], f=8)
    ref = br.RefPair(**kw)
    b = next(iter(data.DeepFashionPair(**kw, image_only=True).batches(2)))
    assert list(b) == ["image", "txt"] and same(b["image"], br.collate([ref[0], ref[1]])["image"])
    ds = data.DeepFashionSample(**kw, input_mask_type="bbox")
    name = br.image_name(2)
    one = ds[name]
    assert list(one) == ["src_image", "styles", "image", "txt", "smpl", "smpl_image", "person_mask"]
    assert same(one["image"], one["src_image"]) and same(one["image"], ref[1]["image"])  # (pair 1's target is image 2)
    want = br.RefPair(**kw, input_mask_type="bbox")[1]
    for k in ("smpl", "smpl_image", "person_mask", "txt"):
        assert same(one[k], want[k]) if torch.is_tensor(want[k]) else one[k] == want[k], k
    assert [len(x["txt"]) for x in ds.batches(4)] == [4, 2]


# ---------------------------------------------------------------------------------------------------------------------
# end to end: dataset folder -> results/

_cache = {}


def get_model():
    """The tiny recipe-weight model of the test_step tests: its style stage reads embeddings from batch['style_emb'],
    because batch['styles'] holds the crops, as in the reference's dataset."""
    if "m" not in _cache:
        extra = upgpt_amd.model_params("tiny")["extra_cond_stages"]
        extra["style_cond"] = dict(extra["style_cond"], cond_stage_key="style_emb")
        m = upgpt_amd.build_model("tiny", overrides={"extra_cond_stages": extra})
        synth.fill_module_(m)
        synth.fill_ema_(m, salt=1)
        _cache["m"] = m.cuda()
    return _cache["m"]


class WithEmbeddings:
    """The dataset with `txt` replaced by an embedding tensor (the tiny model's text stage is a pass-through) and the style
    embeddings added."""

    def __init__(self, ds):
        self.ds = ds

    def batches(self, batch_size):
        for i, b in enumerate(self.ds.batches(batch_size)):
            g = torch.Generator().manual_seed(i)
            n = len(b["fname"])
            yield dict(b, txt=torch.randn(n, 77, 768, generator=g), style_emb=0.45 * torch.randn(n, 9, 768, generator=g))


def _jpeg_decoded(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG")
    return np.asarray(Image.open(io.BytesIO(f.getvalue())))


def test_run_split_end_to_end(tmp_path):
    m = get_model()
    kw = dict(br.make_tree(tmp_path / "data", n_images=5, pairs=((0, 1), (1, 2), (2, 3), (3, 4)), pic=(256, 192), mask=(256, 256)),
              input_mask_type="bbox")
    ds, ref = data.DeepFashionPair(**kw), br.RefPair(**kw)
    assert len(ds) == 4 and ds.vae_z_size == (32, 24)
    out = evaluate.run_split(m, WithEmbeddings(ds), tmp_path / "out", batch_size=2, ddim_steps=2, ddim_eta=0.)
    assert out == tmp_path / "out" / "results" and not hasattr(m, "logger")
    names = [br.get_name(r['from'], r['to']) for r in ref.df]
    folders = ["concats", "gt", "recon", "samples", "smpl", "src", "styles"]
    assert sorted(os.listdir(out)) == folders
    for k in folders:
        assert sorted(os.listdir(out / k)) == sorted(n + ".jpg" for n in names), k
    want = br.collate([ref[i] for i in range(4)])
    for folder, key in (("gt", "image"), ("src", "src_image"), ("smpl", "smpl_image")):
        vals = fr.input_value(want[key], m.crop_size)
        for i, n in enumerate(names):
            got = np.asarray(Image.open(str(out / folder / (n + ".jpg"))))
            assert np.array_equal(got, _jpeg_decoded(fr.to_pil_array(vals[i]))), (folder, n)
