"""Time of building the conditioning of a pose interpolation for n = 9 and n = 64 frames at 32 x 24, d = 85,
two ways in one process, on the same commit and from the same device-resident inputs:
  (a) prepare.interp_pose: the alphas' upload and one upk_pose_interp_f32 launch; wall clock around the call ending in a
      synchronise, and the launch alone between HIP events (the alphas already on the device);
  (b) the host loop of the reference's demo (app.py:298-300) as a user of this package would type it:
      inference.interp_mask per frame (two .cpu() round trips, a numpy rectangle, an upload) and the torch blend
      alpha * x + (1 - alpha) * y on device tensors; wall clock, synchronised at the end.
The two rounds alternate.  Medians over --rounds after --warmup.  The two results are compared bit for bit before anything
is timed.  One JSON line at the end.  This is a record, not a gate: no threshold, this is not a bench path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from upgpt_amd import _lib, inference, prepare  # noqa: E402

H, W, D = 32, 24, 85


def inputs():
    g = torch.Generator().manual_seed(0)
    src, dst = torch.full((1, H, W), inference.MASK_BG), torch.full((1, H, W), inference.MASK_BG)
    src[0, 3:29, 4:21] = inference.MASK_FG
    dst[0, 3:32, 9:24] = inference.MASK_FG
    return [t.cuda() for t in (src, dst, torch.randn(1, D, generator=g), torch.randn(1, D, generator=g))]


def host_loop(src, dst, x, y, alphas):
    n = len(alphas)
    smpl = x.unsqueeze(0).repeat(n, 1, 1)
    mask = src.unsqueeze(0).repeat(n, 1, 1, 1)
    for i, alpha in enumerate(alphas):
        smpl[i] = alpha * smpl[i] + (1 - alpha) * y
        mask[i] = inference.interp_mask(mask[i], dst, alpha)
    return {"smpl": smpl, "person_mask": mask}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[9, 64])
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of the kernel"
    assert a.rounds >= 20, "the median of at least 20 runs"
    src, dst, x, y = inputs()
    ctx = _lib.get_context(torch.device("cuda", torch.cuda.current_device()))
    med = statistics.median
    result = []
    for n in a.frames:
        alphas = np.linspace(1.0, 0.0, n)
        got, want = prepare.interp_pose(src, dst, x, y, alphas), host_loop(src, dst, x, y, alphas)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), "the two paths differ in %s" % k
        ctx.lib.upk_kernel_launches(ctx.h, 1)
        prepare.interp_pose(src, dst, x, y, alphas)
        launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
        at = torch.from_numpy(alphas).cuda()
        mo, so = torch.empty(n, 1, H, W, device="cuda"), torch.empty(n, 1, D, device="cuda")

        def event_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.pose_interp(src, dst, H, W, x, y, D, at, n, mo, so)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def wall_ms(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        dev_fn, host_fn = (lambda: prepare.interp_pose(src, dst, x, y, alphas)), (lambda: host_loop(src, dst, x, y, alphas))
        for _ in range(a.warmup):
            event_ms(), wall_ms(dev_fn), wall_ms(host_fn)
        k, dw, hw = [], [], []
        for _ in range(a.rounds):  # (alternating: both see the same neighbours on a shared host)
            k.append(event_ms()), dw.append(wall_ms(dev_fn)), hw.append(wall_ms(host_fn))
        print("n = %d frames at %d x %d, d = %d" % (n, H, W, D))
        print("  device: interp_pose (upload of the alphas + %d launch) %.4f ms wall (min %.4f, max %.4f); the launch alone %.4f ms "
              "between HIP events (min %.4f, max %.4f)" % (launches, med(dw), min(dw), max(dw), med(k), min(k), max(k)))
        print("  host:   the demo's loop (interp_mask + torch blend per frame) %.3f ms wall (min %.3f, max %.3f)" % (
            med(hw), min(hw), max(hw)))
        result.append(dict(n=n, h=H, w=W, d=D, rounds=a.rounds, launches=launches,
                           device_wall_ms=dict(median=med(dw), min=min(dw), max=max(dw)),
                           device_event_ms=dict(median=med(k), min=min(k), max=max(k)),
                           host_wall_ms=dict(median=med(hw), min=min(hw), max=max(hw))))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
