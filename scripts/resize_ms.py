"""Time of the low-resolution conditioning for --n pictures of 256 x 176 with pad (8, 0) to 128 x 96, two ways
in one process:
  (a) prepare.lr_transform on uint8 pictures that are already on the device (where upk_image_finish_u8 leaves them):
      one upk_resize_bilinear_u8 launch, timed with HIP events around the call; the launch count is read from
      upk_kernel_launches;
  (b) the reference's path for the same bytes on the host: np.pad(mode='edge'), PIL's resize(BILINEAR), the ToTensor
      arithmetic in numpy (u / 255 * 2 - 1, CHW), the upload of the fp32 batch; wall clock, synchronised at the end.
      The pictures start on the host here; the device -> host copy a caller of (b) pays first is timed separately.
Medians over --rounds after --warmup.  The two results are compared bit for bit before anything is timed.  One JSON line
at the end.  Data of this size is launch-bound: no threshold, this is not a bench path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from upgpt_amd import _lib, prepare  # noqa: E402


def pillow_path(pics, size, pad):
    out = []
    for p in pics:
        padded = np.pad(p, ((pad[1], pad[1]), (pad[0], pad[0]), (0, 0)), mode="edge")
        u8 = np.asarray(Image.fromarray(padded).resize((size[1], size[0]), Image.BILINEAR))
        out.append((u8.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)).transpose(2, 0, 1))
    return torch.from_numpy(np.stack(out)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of the kernel"
    assert a.rounds >= 20, "the median of at least 20 runs"
    H, W, size, pad = 256, 176, [128, 96], (8, 0)
    pics = np.random.default_rng(0).integers(0, 256, (a.n, H, W, 3), dtype=np.uint8)
    dev = torch.from_numpy(pics).cuda()
    lr, _ = prepare.lr_transform(dev, size, pad)  # (uploads the tables)
    host = pillow_path(pics, size, pad)
    torch.cuda.synchronize()
    assert torch.equal(lr.view(torch.int32), host.view(torch.int32)), "the two paths differ"
    ctx = _lib.get_context(dev.device)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    prepare.lr_transform(dev, size, pad)
    launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))

    def device_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        prepare.lr_transform(dev, size, pad)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        device_ms(), wall_ms(lambda: pillow_path(pics, size, pad))
    k = [device_ms() for _ in range(a.rounds)]
    kw = [wall_ms(lambda: prepare.lr_transform(dev, size, pad)) for _ in range(a.rounds)]
    p = [wall_ms(lambda: pillow_path(pics, size, pad)) for _ in range(a.rounds)]
    d2h = [wall_ms(lambda: dev.cpu()) for _ in range(a.rounds)]
    med = statistics.median
    print("%d pictures of %d x %d, pad %s -> %d x %d" % (a.n, H, W, pad, size[0], size[1]))
    print("  device: lr_transform %.4f ms between HIP events (min %.4f, max %.4f), %.4f ms wall with a synchronise, %d launch(es)"
          % (med(k), min(k), max(k), med(kw), launches))
    print("  host:   pad + PIL resize + numpy ToTensor arithmetic + upload %.3f ms wall (min %.3f, max %.3f); the device -> "
          "host copy of the pictures in front of it %.3f ms" % (med(p), min(p), max(p), med(d2h)))
    print(json.dumps(dict(n=a.n, h=H, w=W, pad=list(pad), size=size, rounds=a.rounds, launches=launches,
                          device_event_ms=dict(median=med(k), min=min(k), max=max(k)), device_wall_ms=med(kw),
                          pillow_wall_ms=dict(median=med(p), min=min(p), max=max(p)), d2h_ms=med(d2h))))


if __name__ == "__main__":
    main()
