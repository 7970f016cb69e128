"""Golden vectors for the CLIPTextImageCrossAtten conditioning stage.  The reference's class
(ldm/modules/encoders/modules.py:259-323) is transformers' `CLIPModel` (laion/CLIP-ViT-L-14-laion2B-s32B-b82K: the
ViT-L/14 pair with hidden_act "gelu") plus its own `ldm.modules.attention.CrossAttention(768, 768, heads=8, dim_head=96)`.
This script builds THAT pair — transformers as installed, random init, and CrossAttention imported from the reference
tree given as the argument — loads recipe weights (upgpt_amd/synth.py: a pure function of key name and shape) under the
checkpoint's `cond_stage_model.*` names, runs it on CPU fp32 on seeded inputs and stores inputs + outputs.  Only data is
committed: laion_cond.npz and the list of state-dict names laion_cond_keys.txt.

    python tests/golden/make_laion_cond_golden.py <path of the reference tree>

To stay within the size of clip_text.npz the fp32 outputs are kept for a SUBSET of the 77 tokens (`c_rows`, `text_rows`:
both ends, both sides of the 64-query tile seam of the attention kernel, both sides of the end-of-text position); the
image features are kept whole.
"""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1])
spec = importlib.util.spec_from_file_location("synth", os.path.join(ROOT, "upgpt_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)

import transformers  # noqa: E402
from transformers import CLIPConfig, CLIPModel  # noqa: E402

# `ldm` must resolve to the reference here: the repository's own `ldm/` alias package would shadow it
sys.path[:] = [REF] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
ref_util = types.ModuleType("ldm.modules.diffusionmodules.util")  # (attention.py imports `checkpoint` from it; unused here)
ref_util.checkpoint = lambda func, inputs, params, flag: func(*inputs)
sys.modules.setdefault("ldm.modules.diffusionmodules.util", ref_util)
from ldm.modules.attention import CrossAttention  # noqa: E402
import ldm.modules.attention as ref_attention  # noqa: E402
assert os.path.abspath(ref_attention.__file__).startswith(REF)

PREFIX = "cond_stage_model."
C_ROWS = [0, 1, 2, 5, 9, 14, 19, 20, 21, 31, 40, 47, 55, 62, 63, 64, 70, 76]
TEXT_ROWS = [0, 1, 19, 20, 40, 63, 64, 76]
torch.manual_seed(0)
cfg = CLIPConfig(
    text_config=dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                     max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=768),
    vision_config=dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                       patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=768),
    projection_dim=768)
model = CLIPModel(cfg).eval()
cross = CrossAttention(query_dim=768, context_dim=768, heads=8, dim_head=96).eval()

keys = {}
for owner, mod in (("model.", model), ("cross_att.", cross)):
    new = {}
    for k, v in mod.state_dict().items():
        if v.dtype.is_floating_point:
            new[k] = synth.synth_tensor(PREFIX + owner + k, tuple(v.shape))
            keys[owner + k] = tuple(v.shape)
    missing, unexpected = mod.load_state_dict(new, strict=False)
    assert not unexpected and not [m for m in missing if "position_ids" not in m], (missing, unexpected)

g = torch.Generator(device="cpu").manual_seed(2424)
ids = torch.randint(0, 49408, (2, 77), generator=g)
ids[:, 0] = 49406                           # <|startoftext|>
ids[0, 20:], ids[1, 41:] = 49407, 49407    # <|endoftext|> padding, as the tokenizer produces
styles = torch.randn(2, 9, 3, 224, 224, generator=g)  # [B, 9 crops, 3, 224, 224], already "pre-processed"
with torch.no_grad():
    x = model.text_model(input_ids=ids).last_hidden_state
    f = model.get_image_features(pixel_values=styles.reshape(18, 3, 224, 224))
    f = getattr(f, "pooler_output", f).reshape(2, 9, 768)
    c = cross(x, f)
np.savez_compressed(
    os.path.join(HERE, "laion_cond.npz"), ids=ids.numpy().astype(np.int32),
    styles_crc=np.uint32(zlib.crc32(styles.numpy().tobytes()) & 0xFFFFFFFF), c_rows=np.int32(C_ROWS),
    text_rows=np.int32(TEXT_ROWS), last_hidden_state=x[:, TEXT_ROWS].numpy().astype(np.float32),
    image_features=f.numpy().astype(np.float32), c=c[:, C_ROWS].numpy().astype(np.float32),
    c_rms=np.float32(c.pow(2).mean().sqrt()), text_rms=np.float32(x.pow(2).mean().sqrt()),
    features_rms=np.float32(f.pow(2).mean().sqrt()), transformers_version=np.bytes_(transformers.__version__),
    n_keys=np.int32(len(keys)))
with open(os.path.join(HERE, "laion_cond_keys.txt"), "w") as fh:
    fh.write("".join("%s\n" % k for k in sorted(keys)))
print("wrote laion_cond.npz: text rms %.4f, features rms %.4f, c rms %.4f, %d keys, transformers %s" % (
    x.pow(2).mean().sqrt(), f.pow(2).mean().sqrt(), c.pow(2).mean().sqrt(), len(keys), transformers.__version__))
