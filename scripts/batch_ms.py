"""Time of assembling one test batch of --n samples at 256 x 192 with the decoding left out, two ways in one
process, from the same decoded bytes (pictures, 9 style crops per sample of which 8 exist, a 256 x 256 smpl picture, a
256 x 256 mask, a label map, 85 smpl parameters):
  (a) the device path of upgpt_amd/data.py: the bytes packed into one pinned buffer, one upload, then image / src_image /
      smpl_image (upk_resize_bilinear_u8 with both passes skipped), styles (upk_clip_normalize_u8), person_mask in 'bbox' mode
      (upk_cond_bbox_u8), loss_w (upk_cond_gather_u8) and the one device -> host copy of the boxes; wall clock around the
      whole of it, and the launches alone between HIP events on bytes that are already on the device;
  (b) the reference's per-sample host work on the same bytes, restated with numpy / PIL / torch CPU as tests/batch_ref.py does
      (ToTensor and x * 2 - 1, get_bbox, PIL's NEAREST resize, the CLIP normalisation of nine crops, get_mask), the collate and
      the upload of the fp32 batch; wall clock, synchronised at the end.  One process does all samples in turn: the
      reference spreads them over DataLoader workers, which this does not model.
Medians over --rounds after --warmup.  The two results are compared bit for bit before anything is timed.  One JSON line at
the end.  This is a record, not a gate: no threshold, this is not a bench path."""
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

from upgpt_amd import _lib, data, prepare  # noqa: E402
from upgpt_amd.inference import CLIP_MEAN, CLIP_STD  # noqa: E402

H, W, LATENT, MASK, SLOTS = 256, 192, (32, 24), 256, 9
WEIGHTS = {"face": 8.0, "background": 0.5}


def decoded(n):
    rng = np.random.default_rng(0)
    d = dict(image=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), src=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8),
             smpl_pic=rng.integers(0, 256, (n, MASK, MASK, 3), dtype=np.uint8),
             crops=rng.integers(0, 256, (n * SLOTS, 224, 224, 3), dtype=np.uint8), mask=np.zeros((n, MASK, MASK), dtype=np.uint8),
             segm=rng.integers(0, 24, (n, H, W), dtype=np.uint8), smpl=rng.standard_normal((n, 1, 85)).astype(np.float32))
    for i in range(n):
        d["mask"][i, 20 + i:230 - i, 60 + 2 * i:200 - i] = 255
    d["valid"] = np.array(([1] * (SLOTS - 1) + [0]) * n, dtype=np.int32)
    return d


def device_launches(up):
    out = {"image": prepare.lr_transform(up["image"], [H, W])[1], "src_image": prepare.lr_transform(up["src"], [H, W])[1]}
    left = (MASK - W) // 2
    out["smpl_image"] = prepare.lr_transform(up["smpl_pic"][:, :, left:left + W], [H, W])[1]
    out["styles"] = data.clip_normalize(up["crops"], up["valid"][0]).view(-1, SLOTS, 3, 224, 224)
    out["person_mask"], boxes = data.person_mask(up["mask"], LATENT, 'bbox', return_boxes=True)
    out["loss_w"] = data.loss_weight(up["segm"], LATENT, WEIGHTS, 'mm')
    out["smpl"] = up["smpl"]
    return out, boxes


def device_path(d):
    pack = data._Pack()
    for k in ("image", "src", "smpl_pic", "crops", "mask", "segm", "smpl"):
        pack.add(k, list(d[k]))
    pack.add("valid", [d["valid"]])
    out, boxes = device_launches(pack.upload(torch.device("cuda")))
    assert int(boxes.cpu().min()) >= 0
    return out


def host_path(d):
    mean = np.array(CLIP_MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.array(CLIP_STD, dtype=np.float32).reshape(3, 1, 1)
    lut_ids = {"face": 14, "background": 0}
    left = (MASK - W) // 2
    samples = []
    for i in range(len(d["image"])):
        s = {}
        for key, arr in (("image", d["image"][i]), ("src_image", d["src"][i]), ("smpl_image", d["smpl_pic"][i][:, left:left + W])):
            s[key] = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).to(torch.float32).div(255).mul(2.).sub(1.).permute(1, 2, 0)
        crops = []
        for j in range(SLOTS):
            u8 = d["crops"][i * SLOTS + j] if d["valid"][i * SLOTS + j] else np.zeros((224, 224, 3), dtype=np.uint8)
            crops.append(torch.from_numpy((u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std))
        s["styles"] = torch.stack(crops)
        m = d["mask"][i]
        r, c = np.nonzero(np.mean(m, 1))[0], np.nonzero(np.mean(m, 0))[0]
        bbox = np.zeros_like(m, np.uint8)
        bbox[r[0]:r[-1] + 1, c[0]:c[-1] + 1] = 1
        small = np.asarray(Image.fromarray(bbox).resize((LATENT[1], LATENT[0]), Image.NEAREST))
        s["person_mask"] = torch.from_numpy(small.copy())[None].to(torch.float32).div(255) * 2. - 1.
        w = np.full(d["segm"][i].shape, 1.0, dtype=np.float32)
        for label, value in WEIGHTS.items():
            w[d["segm"][i] == lut_ids[label]] = value
        s["loss_w"] = torch.from_numpy(np.asarray(Image.fromarray(w).resize((LATENT[1], LATENT[0]), Image.NEAREST)).copy())[None]
        s["smpl"] = torch.from_numpy(d["smpl"][i])
        samples.append(s)
    return {k: torch.stack([s[k] for s in samples]).cuda() for k in samples[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of the kernels"
    assert a.rounds >= 20, "the median of at least 20 runs"
    d = decoded(a.n)
    got, want = device_path(d), host_path(d)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), "the two paths differ in %s" % k
    up = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    up["valid"] = up["valid"][None]
    ctx = _lib.get_context(torch.device("cuda", torch.cuda.current_device()))
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    device_launches(up)
    launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))

    def event_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_launches(up)
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
        event_ms(), wall_ms(lambda: device_path(d)), wall_ms(lambda: host_path(d))
    k = [event_ms() for _ in range(a.rounds)]
    dw = [wall_ms(lambda: device_path(d)) for _ in range(a.rounds)]
    hw = [wall_ms(lambda: host_path(d)) for _ in range(a.rounds)]
    med = statistics.median
    mb = sum(v.nbytes for v in d.values()) / 1e6
    print("a batch of %d at %d x %d, %d crops (%d stored), %.1f MB of decoded bytes" % (a.n, H, W, a.n * SLOTS, int(d["valid"].sum()), mb))
    print("  device: pack + upload + %d launches + the boxes' copy %.3f ms wall (min %.3f, max %.3f); the launches alone %.4f ms "
          "between HIP events (min %.4f, max %.4f)" % (launches, med(dw), min(dw), max(dw), med(k), min(k), max(k)))
    print("  host:   the reference's per-sample arithmetic + collate + upload %.2f ms wall (min %.2f, max %.2f)" % (
        med(hw), min(hw), max(hw)))
    print(json.dumps(dict(n=a.n, h=H, w=W, crops=a.n * SLOTS, decoded_mb=mb, rounds=a.rounds, launches=launches,
                          device_wall_ms=dict(median=med(dw), min=min(dw), max=max(dw)),
                          device_event_ms=dict(median=med(k), min=min(k), max=max(k)),
                          host_wall_ms=dict(median=med(hw), min=min(hw), max=max(hw)))))


if __name__ == "__main__":
    main()
