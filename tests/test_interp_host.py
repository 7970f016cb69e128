"""Host side of pose interpolation: the restatement tests/interp_ref.py against the reference's own
functions, the census of the evaluation-sensitive truncations, the argument rules of prepare.interp_pose and
InferenceModel.interpolate (stub holder, as tests/test_glue.py), and the host part of prepare.load_pose."""
import os
import pickle
import types

import numpy as np
import pytest
import torch
from PIL import Image

import interp_ref as ir
from upgpt_amd import _lib, build, evaluate, inference, prepare
from upgpt_amd.inference import InferenceModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_and_build_list():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    assert "int upk_pose_interp_f32(upk_ctx* ctx" in header and "upk_pose_interp_f32" in _lib.SYMBOLS
    assert "pose.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pose.hip"))
    assert build.FILE_FLAGS["pose.hip"] == ["-ffp-contract=off"]
    import ldm.data.generate_utils as gu
    assert gu.interp_pose is prepare.interp_pose and gu.load_pose is prepare.load_pose
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n## 31. " in design and "upk_pose_interp_f32" in design
    assert "InferenceModel.interpolate" in open(os.path.join(ROOT, "README.md")).read()


def test_mask_foreground_constant():
    one = np.float32(1.0) / np.float32(255.0)
    assert np.float32(one * np.float32(2.0)) - np.float32(1.0) == np.float32(inference.MASK_FG) == ir.FG


def test_hazard_census_and_literal_case():
    fma, f32, union = ir.hazards()
    print("hazard census: %d triples under an fp64 FMA, %d under fp32 evaluation, %d in the union" % (len(fma), len(f32), len(union)))
    assert len(fma) > 0 and len(f32) > 0
    assert (len(fma), len(f32)) == (108, 170)  # (exact arithmetic: the counts do not depend on the machine)
    assert ir.blend_coord(0.05, 3, 3) == 2  # 0.05 * 3 + 0.95 * 3 = 2.9999999999999996
    assert (0.05, 3, 3) in union
    assert ir.evaluations(0.05, 3, 3)[0] == 2
    # the exact-rational evaluation of the contract IS what fp64 hardware computes
    for alpha, c1, c2 in union:
        assert ir.evaluations(alpha, c1, c2)[0] == ir.blend_coord(alpha, c1, c2)
    # alpha 0 and 1 are never hazards: the destination / source coordinate comes back unchanged
    assert all(0.0 < a < 1.0 for a, _, _ in union)


def test_restatement_equals_the_reference_on_the_hazard_set():
    """Boxes and masks against inference.interp_mask (numpy's mean-based get_coord, fp64 blend, astype(int32)) for every
    hazard triple on rows and on columns; the SMPL blend against torch's literal expression with a numpy float64 alpha."""
    _, _, union = ir.hazards()
    pairs = sorted({(c1, c2) for _, c1, c2 in union})
    by_pair = {}
    for a, c1, c2 in union:
        by_pair.setdefault((c1, c2), []).append(a)
    checked = 0
    for c1, c2 in pairs:
        src, dst = ir.box_mask(32, 32, c1, 31, c1, 31), ir.box_mask(32, 32, c2, 31, c2, 31)
        alphas = np.array(by_pair[(c1, c2)], dtype=np.float64)
        boxes, masks, _ = ir.interp(src, dst, np.zeros(1, np.float32), np.zeros(1, np.float32), alphas)
        for i, alpha in enumerate(alphas):
            want = inference.interp_mask(torch.from_numpy(src.copy())[None], torch.from_numpy(dst.copy())[None], alpha)
            assert torch.equal(torch.from_numpy(masks[i]), want), (alpha, c1, c2)
            assert boxes[2 + i, 0] == boxes[2 + i, 2] == ir.blend_coord(alpha, c1, c2)
            checked += 1
    assert checked == len(union)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(1, 85, generator=g), torch.randn(1, 85, generator=g)
    x[0, :4] = torch.tensor([1e-40, -3e-39, 65504.0, 0.0])
    y[0, :4] = torch.tensor([2e-41, 65504.0, -1e-38, 1e-45])
    alphas = np.array(ir.ALPHAS20, dtype=np.float64)
    _, _, smpl = ir.interp(ir.box_mask(2, 2, 0, 0, 0, 0), ir.box_mask(2, 2, 0, 0, 0, 0), x[0].numpy(), y[0].numpy(), alphas)
    for i, alpha in enumerate(alphas):
        assert isinstance(alpha, np.float64)
        want = alpha * x + (1 - alpha) * y
        assert want.dtype == torch.float32 and torch.equal(torch.from_numpy(smpl[i]), want), float(alpha)


def test_restatement_other_foregrounds_and_zeroed_masks():
    """The occupancy rule equals the reference's mean rule on the masks in use: {-1, 1}, foregrounds with zeros mixed
    in, and a mask whose background the reference already zeroed in place."""
    for fg in (1.0, -0.99215686):
        src, dst = ir.box_mask(32, 24, 3, 20, 2, 17, fg), ir.box_mask(32, 24, 9, 30, 5, 23, fg)
        src[5:9, 4:9] = 0.0  # holes inside the foreground
        dst[dst == -1.0] = 0.0  # what get_coord leaves behind
        for alpha in (0.0, 0.05, 0.3, 0.55, 1.0):
            _, masks, _ = ir.interp(src, dst, [0.0], [0.0], [alpha])
            want = inference.interp_mask(torch.from_numpy(src.copy())[None], torch.from_numpy(dst.copy())[None], np.float64(alpha))
            assert torch.equal(torch.from_numpy(masks[0]), want)
    assert ir.box_of(np.full((4, 4), -1.0, np.float32)) == [-1] * 4 and ir.box_of(np.zeros((4, 4), np.float32)) == [-1] * 4


def test_alpha_rules():
    assert prepare.check_alphas([1, 0.5, 0]).dtype == np.float64
    assert prepare.check_alphas(np.float32(0.25)).tolist() == [0.25]
    for bad in ([], [0.5, float("nan")], [1.0000001], [-1e-9], ["x"], None):
        with pytest.raises(ValueError):
            prepare.check_alphas(bad)


def test_interp_pose_argument_rules():
    m, s = torch.from_numpy(ir.box_mask(8, 6, 1, 5, 1, 4))[None], torch.zeros(1, 5)
    keep = m.clone()
    with pytest.raises(ValueError):
        prepare.interp_pose(m, m, s, s, [])
    with pytest.raises(ValueError):
        prepare.interp_pose(m, m, s, s, [0.5, 2.0])
    with pytest.raises(ValueError):
        prepare.interp_pose(m, m[:, :4], s, s, [0.5])
    with pytest.raises(ValueError):
        prepare.interp_pose(m, m, s, torch.zeros(1, 6), [0.5])
    with pytest.raises(TypeError):
        prepare.interp_pose(m.double(), m, s, s, [0.5])
    with pytest.raises(ValueError, match="no foreground"):  # (a host mask: checked before any upload)
        prepare.interp_pose(m, torch.full((1, 8, 6), -1.0), s, s, [0.5])
    with pytest.raises(ValueError, match="no foreground"):
        prepare.interp_pose(torch.zeros(1, 8, 6), m, s, s, [0.5])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            prepare.interp_pose(m, m, s, s, [0.5])
    assert torch.equal(m, keep)


class _Model:
    def __init__(self):
        self.calls = []

    def log_images(self, batch, **kw):
        n = len(batch["txt"])
        self.calls.append((n, kw, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}))
        return {"samples": torch.zeros(min(n, kw.get("N", 8)), 3, 4, 2) + len(self.calls)}


def _ref_interp_pose(src_mask, dst_mask, src_smpl, dst_smpl, alphas, return_boxes=False):
    _, masks, smpl = ir.interp(src_mask[0].numpy(), dst_mask[0].numpy(), src_smpl[0].numpy(), dst_smpl[0].numpy(), alphas)
    return {"smpl": torch.from_numpy(smpl), "person_mask": torch.from_numpy(masks)}


def _sample():
    g = torch.Generator().manual_seed(2)
    batch = {"image": torch.zeros(4, 2, 3), "txt": "a person", "styles": torch.randn(9, 8, generator=g),
             "smpl": torch.randn(1, 85, generator=g), "person_mask": torch.from_numpy(ir.box_mask(32, 24, 3, 28, 4, 20))[None]}
    dst = {"smpl": torch.randn(1, 85, generator=g), "person_mask": torch.from_numpy(ir.box_mask(32, 24, 3, 30, 8, 23))[None],
           "smpl_image": torch.zeros(2, 2, 3, dtype=torch.uint8)}
    return batch, dst


def test_interpolate_chunks_keys_and_inputs(monkeypatch):
    monkeypatch.setattr(prepare, "interp_pose", _ref_interp_pose)
    alphas = [1.0, 0.8, 0.7, 0.6, 0.4, 0.3, 0.2, 0.1, 0.0]  # the demo's default: nine
    batch, dst = _sample()
    keep_b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    keep_d = {k: v.clone() for k, v in dst.items()}
    holder = types.SimpleNamespace(device="cpu", model=_Model())
    out = InferenceModel.interpolate(holder, batch, dst, alphas, steps=3)
    assert [c[0] for c in holder.model.calls] == [8, 1]  # two log_images calls: 8 frames and 1
    assert out["samples"].shape == (9, 4, 2, 3)
    assert set(batch) == set(keep_b) and set(dst) == set(keep_d)
    for k, v in keep_b.items():
        assert torch.equal(batch[k], v) if torch.is_tensor(v) else batch[k] == v
    for k, v in keep_d.items():
        assert torch.equal(dst[k], v)
    # without a seed the keyword set of log_images is generate's of today
    want_kw = {"ddim_steps": 3, "use_ema": True, "unconditional_guidance_scale": 3., "unconditional_guidance_label": [""]}
    assert all(c[1] == want_kw for c in holder.model.calls)
    # the frames' conditioning is the reference loop's (app.py:298-300), chunk by chunk
    x = batch["smpl"].unsqueeze(0).repeat(9, 1, 1)
    pm = batch["person_mask"].unsqueeze(0).repeat(9, 1, 1, 1)
    for i, alpha in enumerate(np.array(alphas)):
        x[i] = alpha * x[i] + (1 - alpha) * dst["smpl"]
        pm[i] = inference.interp_mask(pm[i], dst["person_mask"].clone(), alpha)
    got_x = torch.cat([c[2]["smpl"] for c in holder.model.calls])
    got_m = torch.cat([c[2]["person_mask"] for c in holder.model.calls])
    assert torch.equal(got_x, x) and torch.equal(got_m, pm)
    assert holder.model.calls[0][2]["styles"].shape == (8, 9, 8) and holder.model.calls[1][2]["txt"] == ["a person"]
    # keyed: ids [0] * n (shared) or range(n) (independent), cut to the chunks
    for noise, ids in (("shared", [0] * 9), ("independent", list(range(9)))):
        holder = types.SimpleNamespace(device="cpu", model=_Model())
        InferenceModel.interpolate(holder, batch, dst, alphas, steps=3, sampler="dpmpp_2m", noise_seed=7, noise=noise)
        got = [c[1]["noise_keys"] for c in holder.model.calls]
        assert [k.ids for k in got] == [ids[:8], ids[8:]] and all(k.seed == 7 for k in got)
        assert all(c[1]["sampler"] == "dpmpp_2m" for c in holder.model.calls)
    for bad in (dict(alphas=[]), dict(alphas=[0.5, 1.5]), dict(alphas=[0.5], noise="same")):
        with pytest.raises(ValueError):
            InferenceModel.interpolate(holder, batch, dst, **bad)
    with pytest.raises(ValueError):
        InferenceModel.interpolate(holder, batch, {"smpl": dst["smpl"]}, [0.5])


def test_generate_keyword_set():
    holder = types.SimpleNamespace(device="cpu", model=_Model())
    InferenceModel.generate(holder, {"txt": ["a"]}, steps=7, use_ema=False)
    assert "noise_keys" not in holder.model.calls[0][1]
    InferenceModel.generate(holder, {"txt": ["a"]}, steps=7, noise_keys="K")
    assert holder.model.calls[1][1]["noise_keys"] == "K"


def test_load_pose_host_part(tmp_path):
    first, mask = ir.write_pose_folder(tmp_path / "a", hw=(260, 200))
    smpl, picture, got_mask = prepare.read_pose_folder(tmp_path / "a")
    assert smpl.shape == (1, 85) and smpl.dtype == np.float32
    assert np.array_equal(smpl[0, :72], first["pred_body_pose"][0]) and np.array_equal(smpl[0, 72:82], first["pred_betas"][0])
    assert np.array_equal(smpl[0, 82:], first["pred_camera"])
    assert picture.shape == (260, 200, 3) and picture.dtype == np.uint8
    assert Image.open(str(tmp_path / "a" / "pose_mask.png")).mode == "P"
    assert np.array_equal(got_mask, mask) and set(np.unique(got_mask)) == {0, 1}
    # exactly one file of each kind
    for missing in ("pose.p", "pose.jpg", "pose_mask.png"):
        ir.write_pose_folder(tmp_path / ("no_" + missing))
        os.remove(str(tmp_path / ("no_" + missing) / missing))
        with pytest.raises(ValueError, match="expected exactly one"):
            prepare.load_pose(tmp_path / ("no_" + missing))
    ir.write_pose_folder(tmp_path / "two")
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(tmp_path / "two" / "second.jpg"))
    with pytest.raises(ValueError, match="expected exactly one"):
        prepare.load_pose(tmp_path / "two")
    with pytest.raises(ValueError):
        prepare.load_pose(tmp_path / "nowhere")
    ir.write_pose_folder(tmp_path / "badp")
    with open(str(tmp_path / "badp" / "pose.p"), "wb") as f:
        pickle.dump([{"pred_betas": np.zeros((1, 10), np.float32)}], f)
    with pytest.raises(ValueError, match="pred_body_pose"):
        prepare.load_pose(tmp_path / "badp")


def test_run_interpolation_files_with_stubs(tmp_path):
    """File names, count, decoded sizes, the strip and the upscaled folder, with stub model objects."""
    calls = []

    class Im:
        def interpolate(self, batch, dst_pose, alphas, **kw):
            calls.append(kw)
            g = np.random.default_rng(0)
            return {"samples": g.random((len(alphas), 16, 12, 3)).astype(np.float32)}

    class Up:
        def upscale(self, pictures, styles, txt, steps=200, sampler="ddim"):
            calls.append((pictures.shape, pictures.dtype, txt, steps, sampler))
            return {"samples": np.repeat(np.repeat(pictures.astype(np.float32) / 255, 2, axis=1), 2, axis=2)}

    batch = {"styles": torch.zeros(9, 8), "txt": "a person"}
    alphas = [1.0, 0.8, 0.7, 0.6, 0.4, 0.3, 0.2, 0.1, 0.0]
    paths = evaluate.run_interpolation(Im(), batch, {}, alphas, tmp_path / "out", steps=5, sampler="dpmpp_2m", upscale=Up())
    assert calls[0] == {"steps": 5, "sampler": "dpmpp_2m", "noise_seed": 0}
    assert [os.path.relpath(str(p), str(tmp_path / "out")) for p in paths] == ["interp/interp_%d.jpg" % i for i in range(9)]
    assert sorted(os.listdir(str(tmp_path / "out" / "interp"))) == sorted("interp_%d.jpg" % i for i in range(9))
    for p in paths:
        assert Image.open(str(p)).size == (12, 16)
    assert Image.open(str(tmp_path / "out" / "interp_strip.jpg")).size == (9 * 12, 16)
    assert calls[1] == ((8, 16, 12, 3), np.uint8, "a person", 5, "dpmpp_2m") and calls[2][0] == (1, 16, 12, 3)
    assert sorted(os.listdir(str(tmp_path / "out" / "interp_upscaled"))) == sorted("interp_%d.png" % i for i in range(9))
    for i in range(9):
        up = Image.open(str(tmp_path / "out" / "interp_upscaled" / ("interp_%d.png" % i)))
        assert up.size == (24, 32)
    # PNG is lossless: the first upscaled picture is the doubled frame
    g = np.random.default_rng(0)
    frame0 = np.uint8(g.random((9, 16, 12, 3)).astype(np.float32)[0] * 255)
    want = np.uint8(np.repeat(np.repeat(frame0.astype(np.float32) / 255, 2, axis=0), 2, axis=1) * 255)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "out" / "interp_upscaled" / "interp_0.png"))), want)
