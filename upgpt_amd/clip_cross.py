"""The CLIPTextImageCrossAtten conditioning stage on the HIP kernels.

The reference's `CLIPTextImageCrossAtten` (ldm/modules/encoders/modules.py:259-323, the cond stage of
configs/deepfashion/inshop_laion_clip.yaml) holds transformers' `CLIPModel("laion/CLIP-ViT-L-14-laion2B-s32B-b82K")` and
a `CrossAttention(768, 768, heads=8, dim_head=96)`:

    x      = model.text_model(tokens).last_hidden_state            [B, 77, 768]
    styles = model.get_image_features(the n crops of each sample)  [B, n, 768]
    c      = cross_att(x, styles)                                  [B, 77, 768]   (no residual, no norm)

* `CLIPModelHF` holds the weights under `CLIPModel`'s key names (`text_model.*`, `vision_model.*`,
  `visual_projection.weight`, and the unused `text_projection.weight` / `logit_scale`), so a checkpoint's
  `cond_stage_model.model.*` entries load with `load_state_dict`.  The laion model's hidden_act is the exact GELU
  (`upk_gelu_f16` behind each fc1), unlike the quick_gelu of OpenAI's towers.
* Compute: the two tower programs (clip_text.py, clip_image.py) leave fp16 activations on the device; `_CrossPlan` reads
  them in place: `to_q` GEMM over the text rows, ONE `to_k | to_v` GEMM over the B * n feature rows,
  `upk_attention_fewkeys_f16` (8 heads of 96 over n <= 16 keys, k and v two column slices of that GEMM's output), and
  the `to_out` GEMM with its bias into fp32.  No torch op computes anything and nothing visits the host in between.
"""
import torch
from torch import nn

from . import knobs as K
from .clip_image import CLIPVisionHF
from .clip_text import CLIPTextTransformer
from .engine import Act, Emitter, Packer, Program
from .params import ParamTree, weights_fingerprint
from .plancache import PlanCache

LAION_L14 = "laion/CLIP-ViT-L-14-laion2B-s32B-b82K"
MAX_STYLES = 16  # keys of upk_attention_fewkeys_f16


class CLIPModelHF(ParamTree):
    """Parameters of transformers' `CLIPModel` under its own key names.  The two towers are the HIP-kernel ones; their
    parameter subtrees hang directly under this module (`text_model`, `vision_model`, `visual_projection`), so the keys
    carry no extra level.  `text_projection.weight` and `logit_scale` are held for the checkpoint and never read.

    config: `hidden_act` and `projection_dim` for both towers, `text=dict(...)` / `vision=dict(...)` for one of them
    (the keys of clip_text.CLIP_L14_TEXT / clip_image.CLIP_L14_VISION)."""

    def __init__(self, hidden_act="gelu", projection_dim=768, text=None, vision=None):
        super().__init__()
        text_t = CLIPTextTransformer(**dict(dict(hidden_act=hidden_act), **(text or {})))
        vision_t = CLIPVisionHF(**dict(dict(hidden_act=hidden_act, output_dim=projection_dim), **(vision or {})))
        for tower in (text_t, vision_t):
            for name, child in tower.named_children():
                self.add_module(name, child)
        # (the tower objects themselves stay outside the module tree: their parameters are the ones registered above)
        self.__dict__["towers"] = (text_t, vision_t)
        self.add_params({"text_projection.weight": (projection_dim, text_t.config["hidden_size"]), "logit_scale": ()})

    @property
    def text_tower(self):
        return self.towers[0]

    @property
    def vision_tower(self):
        return self.towers[1]

    def get_image_features(self, pixel_values):
        return self.vision_tower(pixel_values)


class _CrossPlan(Emitter):
    """Launches behind the two towers for one (text plan, image plan) pair: q, k | v, attention, to_out."""

    def __init__(self, ctx, get, text_plan, image_plan, B, n, heads, dim_head):
        super().__init__(ctx)
        x, f = text_plan.out, image_plan.f16_features()
        S, inner = x.M // B, heads * dim_head
        pk = Packer(ctx, get)
        P = self.prog = Program(ctx)
        q = self.conv(P, x, pk.pack("to_q", bias=False))
        kv = self.conv(P, f, pk.pack(["to_k", "to_v"], bias=False))  # rows k | v: one launch over the B * n features
        att = Act(self.alloc(x.M, inner), B, S, 1, inner)
        fn, h, chk = self.lib.upk_attention_fewkeys_f16, self.hctx, self._chk
        a = (q.t.data_ptr(), q.ld, S * q.ld, kv.t.data_ptr(), kv.ld, n * kv.ld, kv.t[:, inner:].data_ptr(), kv.ld,
             n * kv.ld, att.t.data_ptr(), att.ld, S * att.ld, B, heads, S, n, dim_head, float(dim_head ** -0.5))
        P.add(lambda s: chk(fn(h, *a, s)), q, kv, att, cls="attention",
              label="attn fewkeys B%d h%d nq%d nkv%d d%d" % (B, heads, S, n, dim_head))
        self.out = self.alloc(x.M, get("to_out.0.weight").shape[0], dtype=torch.float32)
        self.conv(P, att, pk.pack("to_out.0"), out_f32=self.out)
        self.shape = (B, S, self.out.shape[1])
        self.apply_tuning(tune_missing=K.autotune_missing())


class CLIPTextImageCrossAtten(nn.Module):
    """Drop-in for ldm.modules.encoders.modules.CLIPTextImageCrossAtten (modules.py:259-323).  State-dict keys:
    `model.*` as transformers' CLIPModel, `cross_att.to_q / to_k / to_v.weight`, `cross_att.to_out.0.weight / .bias`.

    forward(txt, styles): txt a list of B strings (needs the hub model's tokenizer files on disk, or `tokenizer=`) or,
    as this package's extension, an int tensor [B, max_length] of token ids; styles [B, n, 3, 224, 224] pre-processed
    crops, n <= 16.  Returns fp32 [B, max_length, 768].  There is deliberately no `encode`: LatentDiffusion.
    get_learned_conditioning then calls the stage with the {txt, styles} dict as keyword arguments, as the reference
    does.  `tower_config` goes to CLIPModelHF (tests use small towers)."""

    def __init__(self, version=LAION_L14, max_length=77, device="cuda", style_encode="image", tokenizer=None,
                 heads=8, dim_head=96, **tower_config):
        super().__init__()
        if style_encode not in ("image", "text", None):
            raise ValueError("style_encode must be 'image', 'text' or None, got %r" % (style_encode,))
        self.version, self.max_length, self.device, self.style_encode = version, max_length, device, style_encode
        if style_encode == "text":
            self.get_text_outputs(None)  # (NotImplementedError with the reason: refused up front, not at the first batch)
        self.tokenizer = tokenizer
        self.heads, self.dim_head = heads, dim_head
        if max_length != 77 and "text" not in tower_config:
            tower_config["text"] = dict(max_position_embeddings=max_length)
        self.model = CLIPModelHF(**tower_config)
        self.freeze()
        width, inner = self.model.text_tower.config["hidden_size"], heads * dim_head
        if self.model.vision_tower.config["output_dim"] != width:
            raise ValueError("the image features (%d) and the text states (%d) must have one width: the reference's "
                             "CrossAttention takes both as 768" % (self.model.vision_tower.config["output_dim"], width))
        # CrossAttention(query_dim, context_dim, heads, dim_head): to_q / to_k / to_v without bias, to_out.0 with
        # (attention.py:152-168; its Dropout `to_out.1` has no parameters)
        self.cross_att = ParamTree({"to_q.weight": (inner, width), "to_k.weight": (inner, width),
                                    "to_v.weight": (inner, width), "to_out.0.weight": (width, inner),
                                    "to_out.0.bias": (width,)})
        self._plans, self._fp = PlanCache(2), None

    def freeze(self):
        """modules.py:320-323: the CLIP model is frozen, the cross-attention stays trainable."""
        self.model = self.model.eval()
        for param in self.model.parameters():
            param.requires_grad = False

    # ---- text
    def _tokenizer(self):
        if self.tokenizer is None:
            try:
                from transformers import CLIPTokenizer
                tok = CLIPTokenizer.from_pretrained(self.version, local_files_only=True)
                if len(tok) < self.model.text_tower.config["vocab_size"] - 2:
                    # (transformers 5.x hands back an EMPTY tokenizer instead of failing when the files are missing)
                    raise FileNotFoundError("tokenizer of %r has %d entries" % (self.version, len(tok)))
                self.tokenizer = tok
            except Exception as e:  # no hub access: the vocabulary files have to be on disk
                raise RuntimeError(
                    "CLIPTextImageCrossAtten needs the CLIP tokenizer files of %r on disk (no network): pass "
                    "tokenizer=..., or give txt as an int tensor [B, %d] of token ids" % (self.version, self.max_length)) from e
        return self.tokenizer

    def _tokens(self, text):
        if torch.is_tensor(text):
            if text.is_floating_point() or text.dim() != 2:
                raise ValueError("txt as a tensor must be int token ids [B, %d], got %s %s" % (
                    self.max_length, text.dtype, tuple(text.shape)))
            return text
        enc = self._tokenizer()(text, truncation=True, max_length=self.max_length, return_length=True,
                                return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
        return enc["input_ids"]

    def get_text_emb(self, text):
        """modules.py:294-296: last_hidden_state of the text tower, fp32 [B, max_length, 768]."""
        return self.model.text_tower(input_ids=self._tokens(text)).last_hidden_state

    def get_text_outputs(self, texts):
        raise NotImplementedError(
            "style_encode='text' (the pooled text outputs of 9 style captions as the styles, modules.py:298-305) is not "
            "built: no config of the reference uses it; style_encode='image' is the cond stage of inshop_laion_clip.yaml")

    # ---- image
    @torch.no_grad()
    def forward_image(self, image):
        """modules.py:280-285: [b, n, 3, 224, 224] -> get_image_features -> [b, n, 768]."""
        b, n, c, h, w = image.shape
        return self.model.get_image_features(image.reshape(b * n, c, h, w)).reshape(b, n, -1)

    # ---- the stage
    def _plan(self, B, n):
        from ._lib import PLAN_LOCK, get_context
        text_plan, image_plan = self.model.text_tower._plan(B), self.model.vision_tower._plan(B * n)
        p = self.cross_att.to_q.weight
        with PLAN_LOCK:
            fp = weights_fingerprint(self.cross_att)
            if fp != self._fp:
                self._plans.drop(device=p.device)
                self._fp = fp

            def build():
                params = dict(self.cross_att.named_parameters())
                plan = _CrossPlan(get_context(p.device), lambda name: params[name].data, text_plan, image_plan, B, n,
                                  self.heads, self.dim_head)
                torch.cuda.current_stream(p.device).synchronize()  # (weights packed on this lane's stream)
                return text_plan, image_plan, plan
            # (not valid: a tower rebuilt or evicted its plan)
            return self._plans.get((B, n), build, p.device, lambda e: e[0] is text_plan and e[1] is image_plan)

    def forward(self, txt, styles, use_text_style=False):
        if self.style_encode is None:
            return self.get_text_emb(txt)
        ids = self._tokens(txt)
        p = self.cross_att.to_q.weight
        if p.device.type != "cuda" or next(self.model.parameters()).device != p.device:
            raise RuntimeError("upgpt_amd.CLIPTextImageCrossAtten computes only through the HIP kernels on an MI355X: move it "
                               "to 'cuda' first. There is no CPU fallback.")
        if styles.dim() != 5 or styles.shape[0] != ids.shape[0] or not 1 <= styles.shape[1] <= MAX_STYLES:
            raise ValueError("styles must be [%d, n <= %d, 3, H, W] crops, got %s" % (ids.shape[0], MAX_STYLES,
                                                                                       tuple(styles.shape)))
        B, n = int(styles.shape[0]), int(styles.shape[1])
        from ._lib import host_io
        text_plan, image_plan, plan = self._plan(B, n)
        with torch.cuda.device(p.device):
            text_plan.check(ids)
            with host_io():  # (token ids come from the host; the towers' eager launches stay under the lock: clip_image.py)
                text_plan.upload(ids)
                image_plan.upload(styles.reshape(B * n, *styles.shape[2:]))
                text_plan.prog.run()
                image_plan.prog.run()
                plan.prog.run()
                return plan.out.clone().view(plan.shape)
