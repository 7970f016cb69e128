"""Wall time of LPIPS (VGG16) of --n picture pairs of 256 x 176, uint8 pictures on the device -> [n, 5] layer
values on the device, with synthetic weights (synth.synthetic_lpips_state): LPIPS.pairs_u8, i.e. per pass of
--pairs_per_pass pairs 2 input launches, 13 convolutions per pair, 13 ReLU (+ pool) passes and 5 x 2 tap launches.
Prints per-pair time (median, min, max over --rounds after --warmup), the launches of one call from upk_kernel_launches,
and the share of the time spent in the 13 ReLU passes, measured by running the plans' programs with and without them
(Program.run(skip_idx=...): an ablation, its results are garbage) — the number that decides whether a ReLU epilogue flag in
upk_conv2d_nhwc_f16 is worth a later change.  One JSON line at the end.  No threshold: this is not a bench path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from upgpt_amd import _lib, synth  # noqa: E402
from upgpt_amd.lpips import LPIPS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--pairs_per_pass", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    H, W = 256, 176
    rng = np.random.RandomState(0)
    gt = torch.from_numpy(rng.randint(0, 256, (a.n, H, W, 3)).astype(np.uint8)).cuda()
    smp = torch.from_numpy(np.clip(gt.cpu().numpy().astype(np.int32) + rng.randint(-20, 21, (a.n, H, W, 3)), 0, 255).astype(np.uint8)).cuda()
    net = LPIPS(pairs_per_pass=a.pairs_per_pass)
    net.load_state_dict(synth.synthetic_lpips_state(0))
    net = net.cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    _, lv = timed(lambda: net.pairs_u8(smp, gt))  # builds the plans
    assert bool(torch.isfinite(lv).all())
    ctx = _lib.get_context(smp.device)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    net.pairs_u8(smp, gt)
    launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
    for _ in range(a.warmup):
        timed(lambda: net.pairs_u8(smp, gt))
    ms = [timed(lambda: net.pairs_u8(smp, gt))[0] for _ in range(a.rounds)]

    # the programs alone (no input launches, no result copy), with and without their ReLU passes
    plans = [net._plan(min(a.pairs_per_pass, a.n - i), H, W) for i in range(0, a.n, a.pairs_per_pass)]
    relu_idx = [[i for i, lab in enumerate(p.prog.labels) if lab.startswith("relu")] for p in plans]
    assert all(len(r) == 13 for r in relu_idx)

    def programs(skip):
        for p, r in zip(plans, relu_idx):
            p.prog.run(skip_idx=r if skip else ())

    full, bare = [], []
    for _ in range(a.warmup + a.rounds):
        full.append(timed(lambda: programs(False))[0])
        bare.append(timed(lambda: programs(True))[0])
    full, bare = full[a.warmup:], bare[a.warmup:]
    share = 1.0 - statistics.median(bare) / statistics.median(full)
    med = statistics.median(ms)
    print("%d pairs of %d x %d, %d per pass: %.3f ms (min %.3f, max %.3f over %d rounds) = %.3f ms per pair, %d launches" % (
        a.n, H, W, a.pairs_per_pass, med, min(ms), max(ms), len(ms), med / a.n, launches))
    print("programs alone: %.3f ms, without the 13 ReLU passes %.3f ms: share %.1f %%" % (
        statistics.median(full), statistics.median(bare), 100 * share))
    print(json.dumps(dict(n=a.n, h=H, w=W, pairs_per_pass=a.pairs_per_pass, rounds=a.rounds, ms=dict(median=med, min=min(ms), max=max(ms)),
                          ms_per_pair=med / a.n, launches=launches, programs_ms=statistics.median(full),
                          programs_without_relu_ms=statistics.median(bare), relu_share=share)))


if __name__ == "__main__":
    main()
