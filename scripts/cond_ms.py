"""Time of the CLIPTextImageCrossAtten conditioning stage for --n samples of 77 tokens and 9 style crops,
full-size towers with recipe weights, in one process:
  (a) the stage per call: text tower, image tower over 9 n crops, to_q, to_k | to_v, upk_attention_fewkeys_f16, to_out;
      HIP events around the call (token ids and crops already on the device); launches from upk_kernel_launches;
  (b) the few-keys attention launch alone, on buffers of the stage's shape;
  (c) the conditioning pair of bbox.yaml on the same inputs, as the baseline: FrozenCLIPEmbedder (text tower, quick_gelu)
      and FrozenClipImageEmbedder2 (image tower, quick_gelu), whose outputs are concatenated along the tokens.
Medians over --rounds after --warmup.  One JSON line at the end.  This is a record, not a gate: no threshold, this is not a
bench path."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from upgpt_amd import _lib, synth  # noqa: E402
from upgpt_amd.clip_cross import CLIPTextImageCrossAtten  # noqa: E402
from upgpt_amd.clip_image import FrozenClipImageEmbedder2  # noqa: E402
from upgpt_amd.clip_text import FrozenCLIPEmbedder  # noqa: E402


def fill(module, prefix):
    module.load_state_dict({k: synth.synth_tensor(prefix + k, tuple(v.shape)) for k, v in module.state_dict().items()})
    return module.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of the kernels"
    assert a.rounds >= 20, "the median of at least 20 runs"
    B, n, S, heads, d = a.n, 9, 77, 8, 96
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, 49408, (B, S), generator=g).cuda()
    crops = torch.randn(B, n, 3, 224, 224, generator=g).cuda()
    stage = fill(CLIPTextImageCrossAtten(), "cond_stage_model.")
    text, image = fill(FrozenCLIPEmbedder(), "cond_stage_model."), fill(FrozenClipImageEmbedder2(), "extra_cond_models.0.")
    ctx = _lib.get_context(ids.device)
    hd = heads * d
    q = torch.randn(B, S, hd, device="cuda").half()
    kv = torch.randn(B, n, 2 * hd, device="cuda").half()
    o = torch.empty(B, S, hd, device="cuda", dtype=torch.float16)

    def attention():
        ctx.attention_fewkeys(q, hd, S * hd, kv, 2 * hd, n * 2 * hd, kv[..., hd:], 2 * hd, n * 2 * hd, o, hd, S * hd, B, heads,
                              S, n, d, d ** -0.5)

    def pair():
        return torch.cat((text.encode_tokens(ids), image(crops)), 1)

    def launches(fn):
        ctx.lib.upk_kernel_launches(ctx.h, 1)
        fn()
        return int(ctx.lib.upk_kernel_launches(ctx.h, 0))

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    runs = {"stage": lambda: stage(ids, crops), "attention_fewkeys": attention, "bbox_pair": pair}
    out = dict(n=B, crops=n, tokens=S, rounds=a.rounds)
    for name, fn in runs.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        nl = launches(fn)
        t = [event_ms(fn) for _ in range(a.rounds)]
        out[name] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), launches=nl)
        print("  %-18s %.4f ms between HIP events (min %.4f, max %.4f), %d launches" % (name, statistics.median(t), min(t),
                                                                                       max(t), nl))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
