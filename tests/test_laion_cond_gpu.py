"""The CLIPTextImageCrossAtten conditioning stage on the GPU: the two entry points it adds to the C ABI
(upk_attention_fewkeys_f16, upk_gelu_f16) against fp64, the towers with hidden_act "gelu" and the transformers key
layout against the golden of transformers' CLIPModel, the stage against the golden's `c`, and the stage as the cond
stage of a LatentDiffusion built from the model block of inshop_laion_clip.yaml."""
import math
import os

import numpy as np
import pytest
import torch

import laion_cond_model as M
from upgpt_amd import _lib as L
from upgpt_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# Relative rms error of the stage's `c` against the golden: 2 x the error of the text tower alone.
# Yardstick: the parent commit's CLIP text tower against ITS transformers golden (test_clip_gpu.py
# test_clip_text_tower_vs_transformers_golden) measured mse 1.4503e-06 at rms(ref) 1.0093 (|ref| mean 0.8100), i.e.
# rel rms 1.1932e-03.  The stage stacks a second, deeper tower and four fp16 GEMM / attention stages on top of that tower.
# Measured for the stage on an MI355X: 7.949e-04.
TEXT_TOWER_REL = 1.1932e-03
STAGE_REL_BOUND = 2 * TEXT_TOWER_REL


@pytest.fixture(scope="module")
def ctx():
    return L.get_context(0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ---------------------------------------------------------------------------------------------- few-keys attention
def fewkeys_buffers(B, heads, n_q, n_kv, d, seed=0):
    """q / out with a NaN-filled pad of 8 / 16 columns, k and v two column slices of one [B, n_kv, 2 heads d + 8] buffer."""
    hd = heads * d
    q = torch.full((B, n_q, hd + 8), NAN, device=DEV, dtype=torch.float16)
    q[..., :hd] = rnd(B, n_q, hd, seed=seed).half()
    kv = rnd(B, n_kv, 2 * hd + 8, seed=seed + 1).half()
    out = torch.full((B, n_q, hd + 16), NAN, device=DEV, dtype=torch.float16)
    return q, kv, out


def run_fewkeys(ctx, q, kv, out, B, heads, n_q, n_kv, d, scale):
    hd = heads * d
    ctx.attention_fewkeys(q, q.shape[-1], n_q * q.shape[-1], kv, kv.shape[-1], n_kv * kv.shape[-1], kv[..., hd:],
                          kv.shape[-1], n_kv * kv.shape[-1], out, out.shape[-1], n_q * out.shape[-1], B, heads, n_q, n_kv,
                          d, scale)
    torch.cuda.synchronize()


def fewkeys_ref(q, kv, B, heads, n_q, n_kv, d, scale):
    hd = heads * d
    split = lambda t, n: t.double().view(B, n, heads, d).transpose(1, 2)
    qf, kf, vf = split(q[..., :hd], n_q), split(kv[..., :hd], n_kv), split(kv[..., hd:2 * hd], n_kv)
    ref = torch.softmax(qf @ kf.transpose(-1, -2) * scale, -1) @ vf
    return ref.transpose(1, 2).reshape(B, n_q, hd), vf


@pytest.mark.parametrize("B,heads,n_q,n_kv,d", [(2, 8, 77, 9, 96), (1, 3, 1, 1, 8), (3, 2, 65, 16, 128), (2, 1, 64, 5, 40)])
def test_attention_fewkeys_vs_fp64(ctx, B, heads, n_q, n_kv, d):
    """|got - ref| <= 2^-10 max|v|: half an fp16 ulp for the output rounding of a convex combination of v rows, plus as
    much again for the fp32 arithmetic."""
    hd, scale = heads * d, d ** -0.5
    q, kv, out = fewkeys_buffers(B, heads, n_q, n_kv, d)
    run_fewkeys(ctx, q, kv, out, B, heads, n_q, n_kv, d, scale)
    ref, vf = fewkeys_ref(q, kv, B, heads, n_q, n_kv, d, scale)
    got = out[..., :hd].double()
    assert torch.isfinite(got).all()
    err, bound = float((got - ref).abs().max()), 2.0 ** -10 * float(vf.abs().max())
    print("fewkeys B%d h%d nq%d nkv%d d%d: max err %.3e (bound %.3e)" % (B, heads, n_q, n_kv, d, err, bound))
    assert err <= bound
    assert torch.isnan(out[..., hd:]).all() and torch.isnan(q[..., hd:]).all()  # pads untouched


def test_attention_fewkeys_one_key_is_a_copy(ctx):
    B, heads, n_q, d = 2, 3, 70, 24
    q, kv, out = fewkeys_buffers(B, heads, n_q, 1, d, seed=5)
    run_fewkeys(ctx, q, kv, out, B, heads, n_q, 1, d, d ** -0.5)
    hd = heads * d
    assert torch.equal(out[..., :hd], kv[:, :1, hd:2 * hd].expand(B, n_q, hd))


def test_attention_fewkeys_large_scores(ctx):
    """Scores of magnitude 1e4 (one key aligned with q, the others opposite): the max subtraction keeps the softmax a
    one-hot, the output is that key's v row bit for bit."""
    B, heads, n_q, n_kv, d = 2, 8, 77, 9, 96
    hd, scale = heads * d, d ** -0.5
    q, kv, out = fewkeys_buffers(B, heads, n_q, n_kv, d, seed=9)
    g = torch.Generator(device="cpu").manual_seed(3)
    sign = (torch.randint(0, 2, (B, 1, heads, d), generator=g) * 2 - 1).to(DEV).half() * 32  # q k = 96 * 1024, * scale = 1.0e4
    q[..., :hd] = sign.expand(B, n_q, heads, d).reshape(B, n_q, hd)
    hit = (torch.arange(B)[:, None] + torch.arange(heads)[None, :]) % n_kv  # the aligned key of (sample, head)
    k = -sign.expand(B, n_kv, heads, d).clone()
    for b in range(B):
        for h in range(heads):
            k[b, hit[b, h], h] = sign[b, 0, h]
    kv[..., :hd] = k.reshape(B, n_kv, hd)
    assert abs(float((q[0, 0, :d].float() * kv[0, hit[0, 0], :d].float()).sum()) * scale) > 1e4
    run_fewkeys(ctx, q, kv, out, B, heads, n_q, n_kv, d, scale)
    v = kv[..., hd:2 * hd].view(B, n_kv, heads, d)
    want = torch.stack([torch.stack([v[b, hit[b, h], h] for h in range(heads)]) for b in range(B)])  # [B, heads, d]
    assert torch.isfinite(out[..., :hd]).all()
    assert torch.equal(out[..., :hd].view(B, n_q, heads, d), want[:, None].expand(B, n_q, heads, d))


@pytest.mark.parametrize("what", ["n_kv=0", "n_kv=17", "d=12", "d=136", "ld=100"])
def test_attention_fewkeys_refusals(ctx, what):
    B, heads, n_q, n_kv, d = 1, 1, 8, 4, 96
    q = torch.zeros(B, n_q, 256, device=DEV, dtype=torch.float16)
    kv = torch.zeros(B, 17, 512, device=DEV, dtype=torch.float16)
    out = torch.full((B, n_q, 256), 7.0, device=DEV, dtype=torch.float16)
    ldq = 256
    if what.startswith("n_kv"):
        n_kv = int(what[5:])
    elif what.startswith("d="):
        d = int(what[2:])
    else:
        ldq = 100
    with pytest.raises(RuntimeError, match="UPK_ESHAPE"):
        ctx.attention_fewkeys(q, ldq, n_q * 256, kv, 512, 17 * 512, kv[..., 256:], 512, 17 * 512, out, 256, n_q * 256, B,
                              heads, n_q, n_kv, d, 0.1)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---------------------------------------------------------------------------------------------- GELU
def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def check_gelu(got, x):
    """|got - ref64| <= 2^-10 |ref64| + 1e-6 (the absolute term: 1 + erf cancels in fp32 for x <~ -4, as in torch's own
    fp32 GELU)."""
    ref = gelu64(x)
    excess = (got.double() - ref).abs() - (2.0 ** -10 * ref.abs() + 1e-6)
    print("gelu: max err %.3e, worst excess over the bound %.3e" % (float((got.double() - ref).abs().max()), float(excess.max())))
    assert torch.isfinite(got).all() and float(excess.max()) <= 0.0


def test_gelu_small_with_pad(ctx):
    buf = torch.full((5, 40), NAN, device=DEV, dtype=torch.float16)
    x = rnd(5, 24, seed=2, scale=2.0).half()
    buf[:, :24] = x
    ctx.gelu(buf, 40, 5, 24)
    torch.cuda.synchronize()
    check_gelu(buf[:, :24], x)
    assert torch.isnan(buf[:, 24:]).all()
    with pytest.raises(RuntimeError, match="UPK_ESHAPE"):
        ctx.gelu(buf, 40, 5, 20)  # cols not a multiple of 8


def test_gelu_range(ctx):
    rows, cols = 154, 3072
    x = torch.linspace(-12.0, 12.0, rows * cols, device=DEV).view(rows, cols).half()
    special = torch.tensor([0.0, 6e-5, -6e-5, 65504.0, -65504.0], device=DEV).half()
    x[0, :5], x[77, 100:105], x[153, -5:] = special, special, special
    buf = x.clone()
    ctx.gelu(buf, cols, rows, cols)
    torch.cuda.synchronize()
    check_gelu(buf, x)
    assert float(buf[0, 3]) == 65504.0 and float(buf[0, 4]) == 0.0 and float(buf[0, 0]) == 0.0


def test_gemm_then_gelu_equals_the_geglu_epilogue(ctx):
    """The same pre-activations through both activations: operands on a coarse binary grid, so every dot product is exact
    in fp32 AND representable in fp16 (the plain GEMM's fp16 output is the GEGLU epilogue's fp32 accumulator); the GEGLU
    value half is weight 0, bias 1."""
    Mr, K, inner = 96, 32, 64
    g = torch.Generator(device="cpu").manual_seed(4)
    a = (torch.randint(-8, 9, (Mr, K), generator=g).float() / 4).to(DEV).half()
    w = (torch.randint(-8, 9, (inner, K), generator=g).float() / 8).to(DEV)  # |sum| <= 64, multiples of 1 / 32
    pre = a.float() @ w.t()
    assert torch.equal(pre.half().float(), pre) and float(pre.abs().max()) > 4
    wp, n_pad = ctx.pack_weight(w.contiguous())
    y = torch.zeros(Mr, inner, device=DEV, dtype=torch.float16)
    ctx.gemm(a, K, Mr, K, wp, inner, n_pad, torch.zeros(n_pad, device=DEV), None, 0, y, inner, 0)
    torch.cuda.synchronize()
    assert torch.equal(y.float(), pre)
    ctx.gelu(y, inner, Mr, inner)
    j = torch.arange(2 * inner)
    blk, r = j // 64, j % 64
    rm = torch.where(r < 32, blk * 32 + r, inner + blk * 32 + (r - 32)).int().to(DEV)  # [32 value | 32 gate] per 64 rows
    w2 = torch.cat([torch.zeros(inner, K, device=DEV), w]).contiguous()
    wp2, n_pad2 = ctx.pack_weight(w2, row_map=rm)
    b2 = torch.cat([torch.ones(inner, device=DEV), torch.zeros(inner, device=DEV)])[rm.long()].contiguous()
    y2 = torch.zeros(Mr, inner, device=DEV, dtype=torch.float16)
    ctx.gemm(a, K, Mr, K, wp2, inner, n_pad2, b2, None, 0, y2, inner, L.F_GEGLU)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    check_gelu(y, pre)


# ---------------------------------------------------------------------------------------------- towers
def test_default_tower_paths_have_not_moved():
    """hidden_act left at its default: the three tower classes of the parent commit give these bits on these weights
    (tests/golden/clip_default_path.npz was written by the parent's classes on an MI355X)."""
    import zlib
    from upgpt_amd.clip_image import CLIPVisual
    from upgpt_amd.clip_text import CLIPTextTower, CLIPTextTransformer
    g = np.load(os.path.join(M.G, "clip_default_path.npz"))
    text = dict(vocab_size=1000, hidden_size=256, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4)
    gen = torch.Generator(device="cpu").manual_seed(99)
    torch.randint(0, 1000, (2, 77), generator=gen)
    crops = torch.randn(3, 3, 224, 224, generator=gen)
    assert (zlib.crc32(crops.numpy().tobytes()) & 0xFFFFFFFF) == int(g["crops_crc"]), "torch.randn stream changed"
    ids = torch.as_tensor(g["ids"]).long()

    def fill(m, prefix):
        m.load_state_dict({k: synth.synth_tensor(prefix + k, tuple(v.shape)) for k, v in m.state_dict().items()})
        return m.cuda()
    z = fill(CLIPTextTransformer(**text), "default_path.text.")(input_ids=ids).last_hidden_state
    assert torch.equal(z.cpu(), torch.as_tensor(g["text_hf"]).float())
    z = fill(CLIPTextTower(**text), "default_path.textproj.").encode_text(ids)
    assert torch.equal(z.cpu(), torch.as_tensor(g["text_openai"]))
    vis = fill(CLIPVisual(width=256, layers=2, heads=4, output_dim=768), "default_path.visual.")
    assert torch.equal(vis(crops.cuda()).cpu(), torch.as_tensor(g["visual"]))
    # the explicit spelling of the default is the default
    again = fill(CLIPVisual(width=256, layers=2, heads=4, output_dim=768, hidden_act="quick_gelu"), "default_path.visual.")
    assert torch.equal(again(crops.cuda()).cpu(), torch.as_tensor(g["visual"]))


@pytest.fixture(scope="module")
def model():
    """LatentDiffusion from the model block of inshop_laion_clip.yaml with recipe weights, on the GPU."""
    m = M.build_model()
    synth.fill_module_(m, prefixes=("model.diffusion_model.", "first_stage_model.", "extra_cond_models.", "cond_stage_model."))
    return m.cuda()


@pytest.fixture(scope="module")
def stage(model):
    return model.cond_stage_model


@pytest.fixture(scope="module")
def gold():
    g = M.golden()
    ids, styles = M.golden_inputs(g)
    return g, ids, styles.cuda()


@pytest.fixture(scope="module")
def c_stage(stage, gold):
    _, ids, styles = gold
    return stage(ids, styles)


def test_towers_with_gelu_vs_golden(stage, gold):
    """The bounds of the quick_gelu towers' own golden tests (test_clip_gpu.py): the activation is the only difference,
    and its error (1.5e-7) is far below the fp16 rounding behind it."""
    g, ids, styles = gold
    x = stage.get_text_emb(ids)
    assert x.shape == (2, 77, 768) and x.dtype == torch.float32 and torch.isfinite(x).all()
    err = (x[:, g["text_rows"].tolist()].cpu() - torch.as_tensor(g["last_hidden_state"])).abs()
    print("laion text tower vs golden: mse %.3e, max err %.3e, rel rms %.3e" % (
        float((err ** 2).mean()), float(err.max()), M.rel_rms(x[:, g["text_rows"].tolist()], torch.as_tensor(g["last_hidden_state"]))))
    assert float((err ** 2).mean()) < 1e-4 and float(err.max()) < 6e-2
    f = stage.forward_image(styles)
    ref = torch.as_tensor(g["image_features"])
    assert f.shape == (2, 9, 768) and torch.isfinite(f).all()
    err = (f.cpu() - ref).abs()
    rel = float(err.max()) / float(ref.abs().max())
    print("laion image tower vs golden: mse %.3e, max err %.3e, max rel %.3e, rel rms %.3e" % (
        float((err ** 2).mean()), float(err.max()), rel, M.rel_rms(f, ref)))
    assert float((err ** 2).mean()) < 1e-3 and rel < 3e-2


# ---------------------------------------------------------------------------------------------- the stage
def test_stage_vs_golden(stage, gold, c_stage):
    g, ids, styles = gold
    c = c_stage
    assert c.shape == (2, 77, 768) and c.dtype == torch.float32 and c.is_cuda and torch.isfinite(c).all()
    rel = M.rel_rms(c[:, g["c_rows"].tolist()], torch.as_tensor(g["c"]))
    print("stage vs golden c: rel rms %.4e (bound %.4e = 2 x %.4e)" % (rel, STAGE_REL_BOUND, TEXT_TOWER_REL))
    assert rel <= STAGE_REL_BOUND
    assert torch.equal(stage(ids, styles), c)  # deterministic
    assert torch.equal(stage(txt=ids.cuda(), styles=styles), c)  # ids on either side
    # style_encode=None: the text embedding unchanged
    stage.style_encode = None
    try:
        assert torch.equal(stage(ids, styles), stage.get_text_emb(ids))
    finally:
        stage.style_encode = "image"


def test_stage_is_invariant_to_the_order_of_the_crops(stage, gold, c_stage):
    g, ids, styles = gold
    perm = torch.tensor([4, 0, 8, 2, 7, 1, 6, 3, 5], device=DEV)
    c2 = stage(ids, styles[:, perm])
    rel = M.rel_rms(c2, c_stage)
    print("stage, crops permuted: rel rms %.4e against the unpermuted call" % rel)
    assert rel <= STAGE_REL_BOUND
    assert M.rel_rms(c2[:, g["c_rows"].tolist()], torch.as_tensor(g["c"])) <= STAGE_REL_BOUND
    c3 = stage(ids, styles.flip(0))  # the other sample's styles: a different conditioning
    assert M.rel_rms(c3, c_stage) > 10 * STAGE_REL_BOUND


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def batch(gold):
    _, ids, styles = gold
    g0 = torch.Generator().manual_seed(5)
    return {"image": torch.rand(2, 256, 192, 3, generator=g0) * 2 - 1, "txt": ids, "styles": styles,
            "smpl": 0.5 * torch.randn(2, 1, 85, generator=g0), "person_mask": synth.person_mask(2, 32, 24)}


def test_log_images_through_the_stage(model, batch, c_stage):
    out = model.get_input(batch, model.first_stage_key, force_c_encode=True)
    c = out[1]["c_crossattn"]
    assert c.shape == (2, 78, 768) and torch.equal(c[:, :77], c_stage)
    log = model.log_images(batch, N=2, ddim_steps=2, ddim_eta=0., seed=3)
    assert log["samples"].shape == (2, 3, 256, 192) and torch.isfinite(log["samples"]).all()
    # the twin: the same model with DummyModel as its cond stage, fed the stage's precomputed c
    from upgpt_amd.poses import DummyModel
    keep = (model.cond_stage_model, model.cond_stage_key_2, model.cond_stage_trainable)
    model.cond_stage_model, model.cond_stage_key_2, model.cond_stage_trainable = DummyModel(), None, False
    try:
        twin = model.log_images(dict(batch, txt=c_stage), N=2, ddim_steps=2, ddim_eta=0., seed=3)
    finally:
        model.cond_stage_model, model.cond_stage_key_2, model.cond_stage_trainable = keep
    assert torch.equal(twin["samples"], log["samples"])


def test_shared_step_through_the_stage(model, batch):
    torch.manual_seed(11)
    loss, loss_dict = model.shared_step(batch)
    assert torch.isfinite(loss).all() and float(loss) > 0
    assert all(torch.isfinite(v).all() for v in loss_dict.values())
