"""CLIP image tower of the style-conditioning stage on the HIP kernels (second half).

The reference's `FrozenClipImageEmbedder2` (ldm/modules/encoders/modules.py:234-256) holds OpenAI's `clip` package model
`ViT-L/14` (a third-party dependency, git main, weights downloaded at run time) and calls `model.encode_image` on
[b, n, 3, 224, 224] pre-processed crops -> [b, n, 768].  `clip.model.VisionTransformer`: Conv2d(3, 1024, 14, stride 14,
bias=False) patch embedding -> [class token ; 256 patches] + positional embedding -> ln_pre -> 24 pre-LN residual blocks
(16 heads of 64, fused in_proj q|k|v, MLP 1024 -> 4096 -> 1024 with QuickGELU) -> ln_post on the class token -> @ proj
[1024, 768].

* `CLIPVisual` holds the weights under the package's own names (`conv1.weight`, `class_embedding`,
  `positional_embedding`, `transformer.resblocks.N.attn.in_proj_weight`, `...mlp.c_fc.weight`, `ln_post.*`, `proj`), so a
  checkpoint's `extra_cond_models.*.model.visual.*` entries load with `load_state_dict` (the text half of the CLIP model
  is never used by this stage and is not held).
* Compute: `upk_patchify_nchw_f32_f16` + GEMM, `upk_vit_assemble_f16`, `upk_layernorm_f16` (ln_pre / ln_post), per block
  LayerNorm folded into the q|k|v projection and into c_fc (`upk_conv_desc.ln_colsum`), `upk_attention_f16`,
  `UPK_F_QUICKGELU`, residual epilogues; the final projection is a GEMM over the class-token rows.
"""
import torch
from torch import nn

from . import _lib as L
from . import knobs as K
from .clip_text import hidden_act
from .engine import Act, Emitter, PW, Packer, Program, _rup
from .packing import SharedPacks
from .params import ParamTree, weights_fingerprint
from .plancache import PlanCache

CLIP_L14_VISION = dict(width=1024, layers=24, heads=16, patch_size=14, image_size=224, output_dim=768, eps=1e-5,
                       hidden_act="quick_gelu")

# weight names of the two layouts the tower is stored under: the `clip` package's VisionTransformer (fused in_proj,
# `proj` stored [width, output_dim]) and the vision half of transformers' CLIPModel (separate q / k / v projections,
# `visual_projection.weight` stored [output_dim, width], i.e. `proj` transposed; "pre_layrnorm" is the library's spelling)
OPENAI_NAMES = dict(conv="conv1.weight", cls="class_embedding", pos="positional_embedding", ln_pre="ln_pre",
                    layer="transformer.resblocks.%d.", qkv="attn.in_proj", ln1="ln_1", out="attn.out_proj", ln2="ln_2",
                    fc1="mlp.c_fc", fc2="mlp.c_proj", ln_post="ln_post", proj="proj", proj_transposed=False)
HF_NAMES = dict(conv="vision_model.embeddings.patch_embedding.weight", cls="vision_model.embeddings.class_embedding",
                pos="vision_model.embeddings.position_embedding.weight", ln_pre="vision_model.pre_layrnorm",
                layer="vision_model.encoder.layers.%d.", qkv=["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"],
                ln1="layer_norm1", out="self_attn.out_proj", ln2="layer_norm2", fc1="mlp.fc1", fc2="mlp.fc2",
                ln_post="vision_model.post_layernorm", proj="visual_projection.weight", proj_transposed=True)


def visual_param_shapes(cfg):
    d, p = cfg["width"], cfg["patch_size"]
    n = (cfg["image_size"] // p) ** 2 + 1
    s = {"class_embedding": (d,), "positional_embedding": (n, d), "proj": (d, cfg["output_dim"]),
         "conv1.weight": (d, 3, p, p), "ln_pre.weight": (d,), "ln_pre.bias": (d,), "ln_post.weight": (d,),
         "ln_post.bias": (d,)}
    for i in range(cfg["layers"]):
        b = "transformer.resblocks.%d." % i
        s[b + "attn.in_proj_weight"], s[b + "attn.in_proj_bias"] = (3 * d, d), (3 * d,)
        s[b + "attn.out_proj.weight"], s[b + "attn.out_proj.bias"] = (d, d), (d,)
        s[b + "ln_1.weight"], s[b + "ln_1.bias"] = (d,), (d,)
        s[b + "mlp.c_fc.weight"], s[b + "mlp.c_fc.bias"] = (4 * d, d), (4 * d,)
        s[b + "mlp.c_proj.weight"], s[b + "mlp.c_proj.bias"] = (d, 4 * d), (d,)
        s[b + "ln_2.weight"], s[b + "ln_2.bias"] = (d,), (d,)
    return s


def hf_vision_param_shapes(cfg):
    """Vision half of transformers' CLIPModel: `vision_model.*` and `visual_projection.weight`."""
    d, p = cfg["width"], cfg["patch_size"]
    n, f = (cfg["image_size"] // p) ** 2 + 1, cfg.get("intermediate_size", 4 * cfg["width"])
    e = "vision_model.embeddings."
    s = {e + "class_embedding": (d,), e + "patch_embedding.weight": (d, 3, p, p), e + "position_embedding.weight": (n, d),
         "vision_model.pre_layrnorm.weight": (d,), "vision_model.pre_layrnorm.bias": (d,)}
    for i in range(cfg["layers"]):
        b = "vision_model.encoder.layers.%d." % i
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[b + "self_attn.%s.weight" % proj], s[b + "self_attn.%s.bias" % proj] = (d, d), (d,)
        for ln in ("layer_norm1", "layer_norm2"):
            s[b + ln + ".weight"], s[b + ln + ".bias"] = (d,), (d,)
        s[b + "mlp.fc1.weight"], s[b + "mlp.fc1.bias"] = (f, d), (f,)
        s[b + "mlp.fc2.weight"], s[b + "mlp.fc2.bias"] = (d, f), (d,)
    s["vision_model.post_layernorm.weight"], s["vision_model.post_layernorm.bias"] = (d,), (d,)
    s["visual_projection.weight"] = (cfg["output_dim"], d)
    return s


class _VisualPlan(Emitter):
    """Launch program of the image tower for N images."""

    def __init__(self, ctx, cfg, get, N, shared=None, names=OPENAI_NAMES):
        super().__init__(ctx)
        self.cfg, self.N = cfg, N
        nm = names
        d, heads, p, img = cfg["width"], cfg["heads"], cfg["patch_size"], cfg["image_size"]
        dh = d // heads
        if dh not in (32, 64, 128) or d % 32:
            raise NotImplementedError("CLIP image tower with head dim %d / width %d" % (dh, d))
        eps = float(cfg["eps"])
        erf_gelu = hidden_act(cfg) == "gelu"
        g = img // p
        npatch, S = g * g, g * g + 1
        kp = _rup(3 * p * p, 32)
        chk, h = self._chk, self.hctx
        P = self.prog = Program(ctx)

        # names in the packer's "<name>.weight / .bias" convention on top of the stored keys
        def lookup(n):
            if n.endswith("attn.in_proj.weight"):
                return get(n.replace("in_proj.weight", "in_proj_weight"))
            if n.endswith("attn.in_proj.bias"):
                return get(n.replace("in_proj.bias", "in_proj_bias"))
            if n == "conv1_flat.weight":
                return get(nm["conv"]).reshape(d, 3 * p * p)
            if n == "proj_t.weight":  # (the Linear layout [output_dim, width])
                return get(nm["proj"]) if nm["proj_transposed"] else get(nm["proj"]).t().contiguous()
            return get(n)

        pk = Packer(ctx, lookup)
        if shared is not None:  # (the packed tower is shared by every lane's plan: 0.6 GB once, not once per lane)
            pk = shared.wrap(pk)
        self.x = self.alloc(N, 3, img, img, dtype=torch.float32)
        patches = Act(self.alloc(N * npatch, kp), N, npatch, 1, kp)
        fn_p = self.lib.upk_patchify_nchw_f32_f16
        ap = (self.x.data_ptr(), N, 3, img, img, p, patches.t.data_ptr(), kp)
        P.add(lambda s: chk(fn_p(h, *ap, s)), self.x, patches, cls="other")
        pe = self.conv(P, patches, pk.pack("conv1_flat", cin_packed=kp, bias=False))
        cls_e, pos_e = pk.vec(nm["cls"]), pk.vec(nm["pos"])
        tok = Act(self.alloc(N * S, d), N, S, 1, d)
        fn_v = self.lib.upk_vit_assemble_f16
        av = (pe.t.data_ptr(), pe.ld, cls_e.data_ptr(), pos_e.data_ptr(), N, npatch, d, tok.t.data_ptr(), tok.ld)
        P.add(lambda s: chk(fn_v(h, *av, s)), pe, cls_e, pos_e, tok, cls="other")
        x = Act(self.alloc(N * S, d), N, S, 1, d)
        self._ln(P, tok, pk.vec(nm["ln_pre"] + ".weight"), pk.vec(nm["ln_pre"] + ".bias"), eps, x, N * S)
        vt_ld = _rup(S, 32)
        M = N * S
        for i in range(cfg["layers"]):
            b = nm["layer"] % i
            qkv = [b + q for q in nm["qkv"]] if isinstance(nm["qkv"], list) else b + nm["qkv"]  # (rows q | k | v either way)
            wqkv = pk.pack(qkv, n_out=2 * d, ln=b + nm["ln1"])
            qk = Act(self.alloc(M, 2 * d), N, S, 1, 2 * d)
            vt = self.alloc(N, heads, dh, vt_ld, zero=True)
            self.conv(P, x, wqkv, out=qk, ln_eps=eps,
                      vt=dict(t=vt, heads=heads, dhead=dh, ld=vt_ld, tokens=S, **{"from": 2 * d}))
            att = Act(self.alloc(M, d), N, S, 1, d)
            # (Emitter.attention: upk_attention_f16 with these seventeen arguments, and the launch recorded in P.attn)
            self.attention(P, qk.t, 2 * d, S * 2 * d, qk.t[:, d:], 2 * d, S * 2 * d, vt, vt_ld, att.t, d, S * d, N, heads, S, S,
                           dh, dh ** -0.5)
            x = self.conv(P, att, pk.pack(b + nm["out"]), residual=x)
            if erf_gelu:  # (hidden_act "gelu": a plain fc1 launch, then the exact GELU in place)
                hmid = self.gelu(P, self.conv(P, x, pk.pack(b + nm["fc1"], ln=b + nm["ln2"]), ln_eps=eps))
            else:
                hmid = self.conv(P, x, pk.pack(b + nm["fc1"], ln=b + nm["ln2"]), ln_eps=eps, flags=L.F_QUICKGELU)
            x = self.conv(P, hmid, pk.pack(b + nm["fc2"]), residual=x)
        # ln_post on the class tokens (row n*S of x: a [N, d] view with leading dimension S*d), then @ proj
        cls_rows = Act(self.alloc(N, d), N, 1, 1, d)
        self._ln(P, x, pk.vec(nm["ln_post"] + ".weight"), pk.vec(nm["ln_post"] + ".bias"), eps, cls_rows, N, ldx=S * x.ld)
        self.out = self.alloc(N, cfg["output_dim"], dtype=torch.float32)
        self.conv(P, cls_rows, pk.pack("proj_t", bias=False), out_f32=self.out)
        self.out16 = None
        self.apply_tuning(tune_missing=K.autotune_missing())

    def _ln(self, P, x, gamma, beta, eps, y, rows, ldx=None):
        fn, h, chk = self.lib.upk_layernorm_f16, self.hctx, self._chk
        a = (x.t.data_ptr(), x.ld if ldx is None else ldx, rows, x.C, gamma.data_ptr(), beta.data_ptr(), eps,
             y.t.data_ptr(), y.ld)
        P.add(lambda s: chk(fn(h, *a, s)), x, gamma, beta, y, cls="layernorm")

    def f16_features(self):
        """The features once more as an fp16 activation [N, output_dim] for a consumer on the device (the k | v
        projection of clip_cross.py): one upk_f32_to_f16 launch appended to the program on first request."""
        if self.out16 is None:
            od = self.cfg["output_dim"]
            if od % 32:
                raise NotImplementedError("fp16 image features need output_dim %% 32 == 0, got %d" % od)
            o16 = self.out16 = Act(self.alloc(self.N, od), self.N, 1, 1, od)
            fn, h, chk, o32, N = self.lib.upk_f32_to_f16, self.hctx, self._chk, self.out, self.N
            self.prog.add(lambda s: chk(fn(h, o32.data_ptr(), N, od, o16.t.data_ptr(), o16.ld, s)), o32, o16, cls="other")
        return self.out16

    def upload(self, images):
        """The only host -> device step of the tower (bracketed by _lib.host_io when the crops come from the host)."""
        img = self.cfg["image_size"]
        if tuple(images.shape) != (self.N, 3, img, img):
            raise ValueError("images must be [%d, 3, %d, %d], got %s" % (self.N, img, img, tuple(images.shape)))
        self.x.copy_(images.to(self.dev, torch.float32))

    def execute(self):
        self.prog.run()
        return self.out.clone()

    def run(self, images):
        self.upload(images)
        return self.execute()


class _VisionTower(ParamTree):
    """Weights of one storage layout + the per-crop-count launch programs ([N, 3, 224, 224] -> [N, 768])."""
    NAMES = OPENAI_NAMES

    def __init__(self, shapes, config):
        super().__init__()
        self.config = config
        self.add_params(shapes)
        self._plans = PlanCache(2)
        self._fp = None

    def _plan(self, N):
        """The launch program for N crops of the calling thread's lane (built on first use)."""
        p = next(self.parameters())
        if p.device.type != "cuda":
            raise RuntimeError("upgpt_amd.%s computes only through the HIP kernels on an MI355X: move it to 'cuda' "
                               "first. There is no CPU fallback." % type(self).__name__)
        with L.PLAN_LOCK:  # (execution lanes: a plan — buffers and packed weights — per (crop count, tuning table, lane))
            fp = weights_fingerprint(self)
            if fp != self._fp:
                self._plans.drop(device=p.device)
                self._fp, self._packs = fp, SharedPacks()

            def build():
                params = dict(self.named_parameters())
                plan = _VisualPlan(L.get_context(p.device), self.config, lambda n: params[n].data, N,
                                   shared=self._packs, names=self.NAMES)
                if self._packs.take_fresh():
                    torch.cuda.current_stream(p.device).synchronize()  # (packed on this lane's stream, read from every lane's)
                return plan
            return self._plans.get((N,), build, p.device)

    def forward(self, images):
        plan = self._plan(int(images.shape[0]))
        p = next(self.parameters())
        from ._lib import host_io
        with torch.cuda.device(p.device), host_io():
            # the whole tower stays serialised against the other lanes' graph captures: with only the upload under the lock
            #  the secondary bench hit "capturing stream has unjoined work" once in five sessions — a tower's first
            # eager launches set function attributes and allocate while another lane captures.  Packed weights are shared.
            plan.upload(images)
            return plan.execute()


class CLIPVisual(_VisionTower):
    """`clip.model.VisionTransformer` weights + forward ([N, 3, 224, 224] -> [N, 768])."""

    def __init__(self, **config):
        cfg = dict(CLIP_L14_VISION, **config)
        super().__init__(visual_param_shapes(cfg), cfg)


class CLIPVisionHF(_VisionTower):
    """The vision half of transformers' `CLIPModel` under its key names (`vision_model.*`, `visual_projection.weight`);
    forward = `CLIPModel.get_image_features` ([N, 3, 224, 224] -> [N, 768])."""
    NAMES = HF_NAMES

    def __init__(self, **config):
        cfg = dict(CLIP_L14_VISION, **config)
        super().__init__(hf_vision_param_shapes(cfg), cfg)


class _CLIPModelShell(nn.Module):
    """The part of `clip.model.CLIP` this stage touches: `.visual` and `.encode_image`."""

    def __init__(self, **config):
        super().__init__()
        self.visual = CLIPVisual(**config)

    def encode_image(self, image):
        return self.visual(image)


class FrozenClipImageEmbedder2(nn.Module):
    """Drop-in for ldm.modules.encoders.modules.FrozenClipImageEmbedder2 (modules.py:234-256): [b, n, 3, 224, 224]
    pre-processed crops -> [b, n, 768]; state-dict keys `model.visual.*` as in the reference's checkpoints."""

    def __init__(self, model="ViT-L/14", jit=False, device="cuda", **config):
        super().__init__()
        if model != "ViT-L/14" and not config:
            raise NotImplementedError("only the ViT-L/14 image tower of the reference configs is described here; pass the "
                                      "VisionTransformer dimensions as keyword arguments for another one")
        self.model = _CLIPModelShell(**config).eval()
        for p in self.parameters():
            p.requires_grad = False

    @torch.no_grad()
    def forward(self, x):
        b, n, c, h, w = x.shape
        ret = self.model.encode_image(x.reshape(b * n, c, h, w))
        return ret.reshape(b, n, -1)

    def encode(self, x):
        return self(x)
