"""Wall time of the FID features (InceptionV3) of --n pictures of 256 x 176, uint8 pictures on the device ->
[n, 2048] on the device, with synthetic weights (synth.synthetic_fid_state): FIDInception.features_u8, i.e. per pass of
--pictures_per_pass pictures one input launch (bilinear resize to 299 x 299), 94 convolutions, 13 pools and the global mean.
Synchronised at each end.  Prints the time (median, min, max over --rounds after --warmup) for every --n, the launches of one
call from upk_kernel_launches and the convolutions' share of the algorithmic FLOPs per second; one JSON line at the end.
No threshold: this is not a bench path."""
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
from upgpt_amd.fid import FIDInception  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[32, 100])
    ap.add_argument("--pictures_per_pass", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    H, W = 256, 176
    rng = np.random.RandomState(0)
    net = FIDInception(pictures_per_pass=a.pictures_per_pass)
    net.load_state_dict(synth.synthetic_fid_state(0))
    net = net.cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    results = []
    for n in a.n:
        x = torch.from_numpy(rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)).cuda()
        _, f = timed(lambda: net.features_u8(x))  # builds the plans
        assert tuple(f.shape) == (n, 2048) and bool(torch.isfinite(f).all())
        ctx = _lib.get_context(x.device)
        ctx.lib.upk_kernel_launches(ctx.h, 1)
        net.features_u8(x)
        launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
        for _ in range(a.warmup):
            timed(lambda: net.features_u8(x))
        ms = [timed(lambda: net.features_u8(x))[0] for _ in range(a.rounds)]
        med = statistics.median(ms)
        flops = sum(net._plan(min(a.pictures_per_pass, n - i), H, W, True).prog.igemm_flops for i in range(0, n, a.pictures_per_pass))
        print("%d pictures of %d x %d, %d per pass: %.3f ms (min %.3f, max %.3f over %d rounds) = %.3f ms per picture, %d launches, "
              "%.1f TFLOP/s over the whole call" % (n, H, W, a.pictures_per_pass, med, min(ms), max(ms), len(ms), med / n, launches,
                                                   flops / med * 1e-9))
        results.append(dict(n=n, h=H, w=W, pictures_per_pass=a.pictures_per_pass, rounds=a.rounds, ms=dict(median=med, min=min(ms), max=max(ms)),
                            ms_per_picture=med / n, launches=launches, conv_flops=flops, tflops=flops / med * 1e-9))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
