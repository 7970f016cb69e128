"""The plan caches of the modules (upgpt_amd/plancache.py, DESIGN.md "Plan caches") on a real MI355X, tiny model: a plan
evicted at the per-lane bound is rebuilt to the same bits, a lane evicts nothing of another lane, and a weight change
drops (and closes) the plans of the old weight set.  tests/test_lanes_gpu.py covers the UNet's lanes."""
import pytest
import torch

import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import synth
from upgpt_amd.ddim import DDIMSampler

pytestmark = pytest.mark.gpu
_cache = {}


def get_model():
    if "tiny" not in _cache:
        m = upgpt_amd.build_model("tiny")
        synth.fill_module_(m)
        _cache["tiny"] = m.cuda()
    return _cache["tiny"]


def lane0(plans):
    return [k for k in plans if k[-1] == 0]


def test_vae_decoder_eviction_bound_and_rebuilt_result():
    """Five latent sizes at B = 1 against the bound of four: 32x24 and 32x32 are the sizes of the decoder's tests
    (test_model_gpu.py), the others vary h and w over the same two lengths and one shorter.  The rebuilt plan of the
    first size gives the first result bit for bit (the decoder is bit-reproducible: the parent passes this test too)."""
    vae = get_model().first_stage_model
    vae._plans.clear()
    sizes = [(32, 24), (24, 32), (32, 32), (24, 24), (16, 24)]
    g = torch.Generator().manual_seed(11)
    zs = [torch.randn(1, 4, h, w, generator=g).cuda() for h, w in sizes]
    first = vae.decode(zs[0])
    key0 = next(iter(vae._plans))
    assert key0 == (1, 32, 24, 1.0, False, 0)
    outs = [vae.decode(z) for z in zs[1:]]
    assert all(o.shape == (1, 3, 8 * h, 8 * w) and torch.isfinite(o).all() for o, (h, w) in zip(outs, sizes[1:]))
    assert len(lane0(vae._plans)) <= 4 and key0 not in vae._plans
    assert [k[1:3] for k in vae._plans] == sizes[1:]
    assert torch.equal(vae.decode(zs[0]), first)
    assert list(vae._plans)[-1] == key0 and len(lane0(vae._plans)) == 4


def test_vae_encoder_eviction_bound_and_rebuilt_result():
    """Three picture sizes against the bound of four (pushing toward it at low cost): nothing is evicted, every size
    keeps its plan, and the first size encodes to the same bits again."""
    vae = get_model().first_stage_model
    vae._enc_plans.clear()
    sizes = [(256, 192), (192, 256), (192, 192)]
    g = torch.Generator().manual_seed(12)
    xs = [(torch.rand(1, 3, H, W, generator=g) * 2 - 1).cuda() for H, W in sizes]
    first = vae.encode(xs[0]).parameters
    plan0 = vae._enc_plans[(1, 256, 192, False, 0)]
    for x in xs[1:]:
        assert torch.isfinite(vae.encode(x).parameters).all()
    assert len(lane0(vae._enc_plans)) <= 4 and [k[1:3] for k in vae._enc_plans] == sizes
    assert torch.equal(vae.encode(xs[0]).parameters, first)
    assert vae._enc_plans[(1, 256, 192, False, 0)] is plan0


def test_clip_image_tower_eviction_bound_and_rebuilt_result():
    """Crop counts 1, 2, 3 against the bound of two."""
    from upgpt_amd.clip_image import FrozenClipImageEmbedder2
    enc = FrozenClipImageEmbedder2(width=256, layers=2, heads=4, output_dim=768)
    enc.load_state_dict({k: synth.synth_tensor("extra_cond_models.0." + k, tuple(v.shape))
                         for k, v in enc.state_dict().items()})
    enc = enc.cuda()
    tower = enc.model.visual
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn(1, n, 3, 224, 224, generator=g).cuda() for n in (1, 2, 3)]
    first = enc(xs[0])
    assert list(tower._plans) == [(1, False, 0)]
    for x in xs[1:]:
        assert torch.isfinite(enc(x)).all()
    assert list(tower._plans) == [(2, False, 0), (3, False, 0)]
    assert torch.equal(enc(xs[0]), first)
    assert list(tower._plans) == [(3, False, 0), (1, False, 0)]


def test_a_lane_evicts_nothing_of_another_lane():
    vae = get_model().first_stage_model
    vae._plans.clear()
    g = torch.Generator().manual_seed(14)
    sizes = [(32, 24), (24, 32), (32, 32), (24, 24)]
    zs = [torch.randn(1, 4, h, w, generator=g).cuda() for h, w in sizes]
    mine = [vae._decode_plan(1, h, w, 1.0) for h, w in sizes]  # lane 0 at its bound
    first = vae.decode(zs[0])
    with L.lane(1):
        theirs = vae._decode_plan(1, 32, 24, 1.0)
        other = vae.decode(zs[0])
    torch.cuda.synchronize()
    assert [vae._plans[k] for k in lane0(vae._plans)] == mine and len(mine) == 4
    assert [k for k in vae._plans if k[-1] == 1] == [(1, 32, 24, 1.0, False, 1)]
    assert theirs is not mine[0] and theirs.ctx is not mine[0].ctx  # own context: own workspace, own buffers
    assert all(p.ctx is mine[0].ctx for p in mine)
    assert torch.equal(other, first)


def test_weight_change_drops_and_closes_the_old_plans():
    model = get_model()
    unet, vae = model.model.diffusion_model, model.first_stage_model
    B, S = 1, 2
    inp = synth.synth_inputs(B, (32, 24), 4, 87, 768, seed=5, steps=S)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    z, _ = DDIMSampler(model).sample(S, B, (4, 32, 24), cond, eta=0.0, x_T=inp["x_T"].cuda(), verbose=False)
    key, old = next((k, p) for k, p in unet._plans.items() if k[0] == "live" and k[-1] == 0 and p.sampler_states)
    assert unet.plan(*key[1:7]) is old
    with torch.no_grad():
        next(unet.parameters()).mul_(1.0)  # (the same values under a new _version: the fingerprint changes)
    new = unet.plan(*key[1:7])
    assert new is not old and unet._plans[key] is new
    assert old.sampler_states == {}  # closed: its captured graphs went with it
    assert all(p is not old for p in unet._plans.values())
    z2, _ = DDIMSampler(model).sample(S, B, (4, 32, 24), cond, eta=0.0, x_T=inp["x_T"].cuda(), verbose=False)
    assert torch.equal(z2, z)

    before = vae.decode(z)
    old_plans = list(vae._plans.values())
    with torch.no_grad():
        next(vae.parameters()).mul_(1.0)
    after = vae.decode(z)
    assert torch.equal(after, before)
    assert all(p not in old_plans for p in vae._plans.values()) and len(vae._plans) == 1
