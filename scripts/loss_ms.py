"""Wall time of the loss layer around the UNet forward at the bench batch (B = 8, latent 4 x 32 x 24) and at the
upscale latent (B = 4, 3 x 128 x 96), inputs and results on the device:
  (a) upk_q_sample_f32 (into the fp16 NHWC stem input) + upk_p_losses_f32: 3 launches
  (b) the same arithmetic as torch element-wise ops and .mean() on the device, what the package would otherwise use
      (extract_into_tensor, q_sample, the layout kernel for the stem input, get_loss, the weighting and the means of
      ddpm.py:1101-1121); it is not part of the code under test
and of one validation_step (two forwards: live and EMA weights) of --model on a DeepFashion-shaped batch of 8.
A call of (a) or (b) is tens of microseconds, so a timed window is --iters calls behind one synchronise; the two alternate
within each of --rounds rounds after --warmup rounds of both; median, min and max per call are printed, the launches of
(a) from upk_kernel_launches and of (b) from torch's profiler, and one JSON line at the end.  The results of (a) and (b)
are compared first.  No threshold: this is not a bench path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import upgpt_amd  # noqa: E402
from upgpt_amd import _lib, synth  # noqa: E402
from upgpt_amd.schedule import extract_into_tensor  # noqa: E402

SHAPES = {"bench B=8 4x32x24": (8, 4, 32, 24), "upscale B=4 3x128x96": (4, 3, 128, 96)}


def make_case(model, shape, dev):
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    case = dict(x0=r(*shape), noise=r(*shape), pred=r(*shape), w=0.5 + torch.rand(B, 1, H, W, generator=g, device=dev),
                t=torch.randint(0, 1000, (B,), generator=g, device=dev), shape=shape,
                xin=torch.zeros(B * H * W, 32, dtype=torch.float16, device=dev), out=torch.empty(4 + 2 * B, device=dev),
                logvar=torch.zeros(1000, device=dev))
    case["t32"] = case["t"].int()
    ctx = _lib.get_context(dev)
    case["ws"] = torch.empty(ctx.p_losses_ws_bytes(B, C, H * W), dtype=torch.uint8, device=dev)
    return case


def hip_way(model, ctx, c):
    B, C, H, W = c["shape"]
    ctx.q_sample(c["x0"], c["noise"], c["t32"], model.sqrt_alphas_cumprod, model.sqrt_one_minus_alphas_cumprod, 1000, None,
                 c["xin"], 32, B, C, H * W)
    ctx.p_losses(c["pred"], c["noise"], c["w"], 1, c["t32"], c["logvar"], model.lvlb_weights, 1000, _lib.LOSS_L2, 1.0, 0.0,
                 c["out"], B, C, H * W, c["ws"], c["ws"].numel())
    return c["out"]


def torch_way(model, ctx, c):
    B, C, H, W = c["shape"]
    x0, noise, t = c["x0"], c["noise"], c["t"]
    x_noisy = (extract_into_tensor(model.sqrt_alphas_cumprod, t, x0.shape) * x0 +
               extract_into_tensor(model.sqrt_one_minus_alphas_cumprod, t, x0.shape) * noise)
    ctx.nchw_to_nhwc(x_noisy, B, C, H * W, c["xin"], 32, 0, 0, 1.0)
    e = (noise - c["pred"]) ** 2
    simple = (c["w"] * e).mean([1, 2, 3])
    logvar_t = c["logvar"][t]
    gamma = (simple / torch.exp(logvar_t) + logvar_t).mean()
    vlb = (model.lvlb_weights[t] * e.mean([1, 2, 3])).mean()
    return torch.stack([1.0 * gamma + 0.0 * vlb, simple.mean(), gamma, vlb])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bbox")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--val_rounds", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    dev = torch.device("cuda", 0)
    model = upgpt_amd.build_model(a.model)
    synth.fill_module_(model)
    synth.fill_ema_(model, salt=1)
    model = model.cuda()
    ctx = _lib.get_context(dev)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    result = {}
    for label, shape in SHAPES.items():
        c = make_case(model, shape, dev)
        variants = [("a upk_q_sample_f32 + upk_p_losses_f32", lambda: hip_way(model, ctx, c)),
                    ("b torch element-wise ops and .mean()", lambda: torch_way(model, ctx, c))]
        ra, rb = variants[0][1]()[:4].double().cpu(), variants[1][1]().double().cpu()
        diff = float(((ra - rb).abs() / rb.abs().clamp_min(1e-30)).max())
        print("%s: max relative |a - b| of {loss, loss_simple, loss_gamma, loss_vlb}: %.2e" % (label, diff))
        assert diff < 1e-5
        ctx.lib.upk_kernel_launches(ctx.h, 1)
        variants[0][1]()
        upk_launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            variants[1][1]()
            torch.cuda.synchronize()
        torch_launches = int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
        for _ in range(a.warmup):
            for _, fn in variants:
                timed(fn, a.iters)
        ms = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                ms[name].append(timed(fn, a.iters)[0])
        res = {}
        for name, _ in variants:
            v = ms[name]
            res[name] = dict(median=statistics.median(v), min=min(v), max=max(v))
            print("  %-42s %8.4f ms per call (min %.4f, max %.4f over %d rounds of %d calls)" % (
                name, res[name]["median"], min(v), max(v), len(v), a.iters))
        print("  launches per call: (a) %d, (b) %d" % (upk_launches, torch_launches))
        result[label] = dict(ms=res, upk_launches=upk_launches, torch_launches=torch_launches, max_rel_diff=diff)

    B = 8
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1, "txt": torch.randn(B, 77, 768, generator=g0),
             "styles": 0.45 * torch.randn(B, 9, 768, generator=g0), "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0),
             "person_mask": synth.person_mask(B, 32, 24), "loss_w": 0.5 + torch.rand(B, 1, 32, 24, generator=g0)}
    batch = {k: v.cuda() for k, v in batch.items()}
    step = lambda: model.validation_step(batch, 0)
    for _ in range(a.warmup):
        timed(step, 1)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    step()
    val_launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
    v = [timed(step, 1)[0] for _ in range(a.val_rounds)]
    d = step()
    print("validation_step (%s, B = %d): %.3f ms (min %.3f, max %.3f over %d calls), %d upk launches; %s" % (
        a.model, B, statistics.median(v), min(v), max(v), len(v), val_launches, {k: round(float(x), 5) for k, x in d.items()}))
    result["validation_step"] = dict(model=a.model, batch=B, median=statistics.median(v), min=min(v), max=max(v),
                                     upk_launches=val_launches)
    print(json.dumps(dict(iters=a.iters, rounds=a.rounds, results=result)))


if __name__ == "__main__":
    main()
