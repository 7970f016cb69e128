"""Wall time of MS-SSIM (plus SSIM, which is its level 0) of --n picture pairs of 256 x 176, uint8 pictures
on the device -> [n] results on the device:
  (a) metrics.ssim_levels: upk_ssim_u8, 2 * 5 launches, then the 30-number tail per image
  (b) the same algorithm as torch ops on the device (depthwise F.conv2d per axis and moment, F.avg_pool2d between the
      levels, element-wise maps, means): what the reference runs through pytorch_msssim (scripts/eval_metrics.py:110-111,
      which calls ssim and ms_ssim separately; here level 0 is shared, in its favour)
The two alternate within each of --rounds rounds after --warmup rounds of both; median, min and max are printed, the
launches of (a) from upk_kernel_launches and of (b) from torch's profiler, and one JSON line at the end.  The results of
(a) and (b) are compared first.  No threshold: this is not a bench path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from upgpt_amd import _lib, metrics  # noqa: E402

C1, C2 = 0.01 ** 2, 0.03 ** 2


def torch_way(a, b):
    """uint8 [N, H, W, 3] device tensors -> (SSIM [N], MS-SSIM [N]) with torch ops, fp32 as the reference."""
    x = a.permute(0, 3, 1, 2).float() / 255
    y = b.permute(0, 3, 1, 2).float() / 255
    c = torch.arange(11, dtype=torch.float32, device=a.device) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).view(1, 1, 11).repeat(3, 1, 1)

    def blur(t):
        t = F.conv2d(t, g.view(3, 1, 11, 1), groups=3)
        return F.conv2d(t, g.view(3, 1, 1, 11), groups=3)

    vals = []
    for l in range(5):
        mu1, mu2 = blur(x), blur(y)
        s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        ssim_c, cs_c = ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)
        if l == 0:
            ssim0 = ssim_c.mean(1)
        vals.append(torch.relu(cs_c if l < 4 else ssim_c))
        if l < 4:
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    wt = torch.tensor(metrics.MS_WEIGHTS, device=a.device).view(-1, 1, 1)
    return ssim0, (torch.stack(vals, 0) ** wt).prod(0).mean(1)


def hip_way(a, b):
    lv = metrics.ssim_levels(a, b, 5)
    return metrics.ssim_from_levels(lv).float(), metrics.ms_ssim_from_levels(lv).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    H, W = 256, 176
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(yy[None, :, :, None] / 7.0 + rng.uniform(0, 6.28, (a.n, 1, 1, 3))) * np.cos(xx[None, :, :, None] / 5.0)
    gt = torch.from_numpy(np.clip(np.rint(base), 0, 255).astype(np.uint8)).cuda()
    smp = torch.from_numpy(np.clip(np.rint(base + 12 * rng.standard_normal(base.shape)), 0, 255).astype(np.uint8)).cuda()
    variants = [("a upk_ssim_u8 (metrics.ssim_levels)", lambda: hip_way(smp, gt)),
                ("b torch ops on the device (the reference's way)", lambda: torch_way(smp, gt))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    (_, ra), (_, rb) = timed(variants[0][1]), timed(variants[1][1])
    diff = [float((x.double() - y.double()).abs().max()) for x, y in zip(ra, rb)]
    print("max |a - b|: SSIM %.2e, MS-SSIM %.2e" % tuple(diff))
    assert max(diff) < 1e-3
    ctx = _lib.get_context(smp.device)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    variants[0][1]()
    upk_launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        variants[1][1]()
        torch.cuda.synchronize()
    torch_launches = int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
    for _ in range(a.warmup):
        for _, fn in variants:
            timed(fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(timed(fn)[0])
    res = {}
    for name, _ in variants:
        v = ms[name]
        res[name] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print("%-50s %8.3f ms (min %.3f, max %.3f over %d rounds)" % (name, res[name]["median"], min(v), max(v), len(v)))
    print("launches: upk_ssim_u8 %d (plus the torch ops of the 30-number tail), torch ops %d" % (upk_launches, torch_launches))
    print(json.dumps(dict(n=a.n, h=H, w=W, rounds=a.rounds, ms=res, upk_launches=upk_launches, torch_launches=torch_launches,
                          max_abs_diff=dict(ssim=diff[0], ms_ssim=diff[1]))))


if __name__ == "__main__":
    main()
