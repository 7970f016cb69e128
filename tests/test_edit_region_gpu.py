"""InferenceModel.edit_region end to end on the tiny model: byte for byte the hand-composed path (the numpy
restatement tests/region_ref.py for the keep-mask, LatentDiffusion.edit_images with the same keys, evaluate's finishing,
the restatement's composite), and the guarantees of a region-locked edit on the returned bytes.

The model is the fixture of tests/test_interp_gpu.py: upgpt_amd.build_model("tiny") with recipe weights inside an
InferenceModel made without the two full-size CLIP towers, which are not on this path."""
import numpy as np
import pytest
import torch

import region_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, F = 256, 192, 8
SEED, DILATE, FEATHER = 21, 8, 4
SAMPLERS = ["ddim", "dpmpp_2m"]
# 3 steps; DDIM takes 4: its uniform schedule (the reference's) needs a step count that divides the 1000 training steps,
# with 3 its last timestep is index 1000 of a 1000-entry table (tests/test_interp_gpu.py runs the same pair)
STEPS_OF = {"ddim": 4, "dpmpp_2m": 3}
STEPS = 4
_cache = {}


@pytest.fixture(scope="module")
def im():
    import upgpt_amd
    from upgpt_amd import synth
    from upgpt_amd.inference import InferenceModel
    model = upgpt_amd.build_model("tiny")
    synth.fill_module_(model)
    m = object.__new__(InferenceModel)
    m.device, m.model = DEV, model.cuda()
    return m


def inputs():
    from upgpt_amd.styles import LIP
    rng = np.random.default_rng(17)
    picture = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    segm = np.zeros((2, H, W), dtype=np.uint8)
    segm[:, :20] = LIP.label2id['hair']
    segm[0, 88:168, 64:144] = LIP.label2id['top']  # sample 0: a rectangle of `top` (12 x 12 cells once dilated by 8); sample 1: none
    return picture, segm


def conditioning(styles_seed=3):
    g = torch.Generator().manual_seed(3)
    one = {"txt": torch.randn(77, 768, generator=g), "smpl": 0.5 * torch.randn(1, 85, generator=g),
           "person_mask": torch.full((1, 32, 24), -1.0)}
    one["person_mask"][:, 3:29, 4:21] = -0.99215686
    one["styles"] = 0.45 * torch.randn(9, 768, generator=torch.Generator().manual_seed(styles_seed))
    return {k: v.unsqueeze(0).repeat([2] + [1] * v.dim()).to(DEV) for k, v in one.items()}


def keys():
    from upgpt_amd.rng import NoiseKeys
    return NoiseKeys(SEED, [0, 1], device=DEV)


def edited(im, sampler, styles_seed=3):
    key = (sampler, styles_seed)
    if key not in _cache:
        picture, segm = inputs()
        _cache[key] = im.edit_region(picture, segm, "top", conditioning(styles_seed), steps=STEPS_OF[sampler], sampler=sampler, dilate=DILATE,
                                     feather=FEATHER, noise_keys=keys())
    return _cache[key]


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_edit_region_equals_the_hand_composed_path(im, sampler):
    from upgpt_amd import _lib, edit, evaluate
    picture, segm = inputs()
    got = edited(im, sampler)
    assert set(got) == {"edited", "samples", "mask", "alpha", "cells"}
    labels = edit.region_labels("top")
    mask, keep, cells = rr.region(segm, labels, DILATE, F)
    cond = conditioning()
    image = (picture.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)  # image_transform
    cond["image"] = torch.from_numpy(image).to(DEV)
    extra = {} if sampler == "ddim" else {"sampler": sampler}
    with torch.no_grad():
        log = im.model.edit_images(cond, torch.from_numpy(keep).to(DEV), N=2, ddim_steps=STEPS_OF[sampler], noise_keys=keys(), use_ema=True,
                                   unconditional_guidance_scale=3., unconditional_guidance_label=[""], **extra)
    assert set(log) == {"reconstruction", "samples"} and tuple(log["samples"].shape) == (2, 3, H, W)
    gen = torch.empty((2, H, W, 3), dtype=torch.uint8, device=DEV)
    evaluate.finish_images(log["samples"].float(), gen, _lib.LAYOUT_NCHW, _lib.FINISH_SAMPLE)
    gen = gen.cpu().numpy()
    out, alpha = rr.composite(picture, gen, mask, FEATHER)
    for name, want in (("edited", out), ("samples", gen), ("mask", mask), ("alpha", alpha), ("cells", cells)):
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, name
        assert got[name].tobytes() == want.tobytes(), name
    assert got["cells"].dtype == np.int32 and got["cells"].tolist() == [int(cells[0]), 0] and cells[0] == 12 * 12


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_outside_the_region_the_input_inside_it_the_sample(im, sampler):
    picture, segm = inputs()
    got = edited(im, sampler)
    a = got["alpha"]
    assert np.array_equal(got["edited"][a == 0], picture[a == 0])
    assert np.array_equal(got["edited"][a == 255], got["samples"][a == 255])
    assert (a == 255).any() and (a[0] == 0).any() and ((a > 0) & (a < 255)).any()
    far = rr.chebyshev_far(segm == 5, DILATE + FEATHER)
    assert not a[far].any() and np.array_equal(got["edited"][far], picture[far])
    assert np.array_equal(got["edited"][1], picture[1]) and not a[1].any() and not got["mask"][1].any()  # an empty region
    assert not np.array_equal(got["edited"][0], picture[0])  # the region of sample 0 was generated
    assert not np.array_equal(got["samples"][1], picture[1])  # (the generated picture itself is not the input)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_same_keys_same_bytes_and_the_batch_is_left_alone(im, sampler):
    picture, segm = inputs()
    batch = conditioning()
    batch["image"] = torch.zeros(2, 8, 8, 3)  # (ignored: the picture is the image)
    before = {k: v.clone() for k, v in batch.items()}
    again = im.edit_region(torch.from_numpy(picture).to(DEV), torch.from_numpy(segm), "top", batch, steps=STEPS_OF[sampler], sampler=sampler,
                           dilate=DILATE, feather=FEATHER, noise_keys=keys())
    first = edited(im, sampler)
    for name in first:
        assert again[name].tobytes() == first[name].tobytes(), name
    assert set(batch) == set(before) and all(torch.equal(batch[k], before[k]) for k in before)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_another_style_changes_the_region_and_nothing_else(im, sampler):
    first, other = edited(im, sampler), edited(im, sampler, styles_seed=4)
    a = first["alpha"]
    assert np.array_equal(a, other["alpha"]) and np.array_equal(first["mask"], other["mask"])
    differ = (first["edited"] != other["edited"]).any(axis=3)
    assert differ[0][a[0] > 0].any()
    assert not differ[a == 0].any() and not differ[1].any()


def test_refusals(im):
    picture, segm = inputs()
    batch = conditioning()
    with pytest.raises(ValueError, match="the model works on 256 x 192"):
        im.edit_region(picture[:, :128], segm[:, :128], "top", batch, steps=STEPS)
    with pytest.raises(ValueError, match="at most 8"):
        im.edit_region(np.zeros((9, H, W, 3), np.uint8), np.zeros((9, H, W), np.uint8), "top", batch, steps=STEPS)
    with pytest.raises(ValueError, match="unknown region"):
        im.edit_region(picture, segm, "sleeve", batch, steps=STEPS)
    with pytest.raises(ValueError, match="keep must be"):
        cond = dict(batch, image=torch.zeros(2, H, W, 3, device=DEV))
        im.model.edit_images(cond, torch.ones(2, 1, 16, 12, device=DEV), N=2, ddim_steps=STEPS)
