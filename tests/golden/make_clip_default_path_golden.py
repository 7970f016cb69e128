"""Pinned outputs of the CLIP towers' DEFAULT code path (hidden_act "quick_gelu": the OpenAI-layout image tower, the text
tower under both key layouts), small towers with recipe weights, computed on an MI355X.  The committed
tests/golden/clip_default_path.npz was written from the classes of the commit BEFORE the hidden_act switch and the second
image-tower key layout were added (the same run compared them with the new classes: equal bit for bit);
tests/test_laion_cond_gpu.py::test_default_tower_paths_have_not_moved holds every later commit to those bits.  Regenerate only
when a kernel on that path is changed on purpose.  Needs the GPU.

    python tests/golden/make_clip_default_path_golden.py     ->  tests/golden/clip_default_path.npz
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from upgpt_amd import synth  # noqa: E402
from upgpt_amd.clip_image import CLIPVisual  # noqa: E402
from upgpt_amd.clip_text import CLIPTextTower, CLIPTextTransformer  # noqa: E402

TEXT = dict(vocab_size=1000, hidden_size=256, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4)
VISION = dict(width=256, layers=2, heads=4, output_dim=768)


def fill(m, prefix):
    m.load_state_dict({k: synth.synth_tensor(prefix + k, tuple(v.shape)) for k, v in m.state_dict().items()})
    return m.cuda()


g = torch.Generator(device="cpu").manual_seed(99)
ids = torch.randint(0, 1000, (2, 77), generator=g)
crops = torch.randn(3, 3, 224, 224, generator=g)
hf = fill(CLIPTextTransformer(**TEXT), "default_path.text.")(input_ids=ids).last_hidden_state.cpu()
assert torch.equal(hf, hf.half().float())  # (the tower's fp16 result widened: stored as fp16 without loss)
np.savez_compressed(
    os.path.join(HERE, "clip_default_path.npz"), text_hf=hf.numpy().astype(np.float16),
    text_openai=fill(CLIPTextTower(**TEXT), "default_path.textproj.").encode_text(ids).cpu().numpy(),
    visual=fill(CLIPVisual(**VISION), "default_path.visual.")(crops.cuda()).cpu().numpy(), ids=ids.numpy().astype(np.int32),
    crops_crc=np.uint32(zlib.crc32(crops.numpy().tobytes()) & 0xFFFFFFFF))
print("wrote clip_default_path.npz")
