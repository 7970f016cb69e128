"""Time of the style crops for --n pictures of 256 x 176 with the LIP groups (8 groups, 9 slots), two ways in
one process:
  (a) styles.style_crops on uint8 pictures and label maps that are already on the device: upk_segm_boxes_u8 and
      upk_style_crops_u8, timed with HIP events around the call; the launch count is read from upk_kernel_launches;
  (b) the reference's loop for the same data on the host: per picture and group the mask, the two torch.sum scans of
      get_mask_range, the masked fill or the cut and zero pad, PIL's resize(BILINEAR) and centre crop, then the
      ToTensor / Normalize arithmetic in numpy and the upload of the fp32 batch; wall clock, synchronised at the end.
      (The reference also writes every crop as a JPEG and reads it back; that is left out here, in its favour.)
Medians over --rounds after --warmup.  The two results are compared bit for bit before anything is timed.  One JSON line
at the end.  This is a record, not a gate: no threshold, this is not a bench path."""
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

from upgpt_amd import _lib, styles  # noqa: E402
from upgpt_amd.inference import CLIP_MEAN, CLIP_STD, style_names  # noqa: E402


def label_maps(n, h, w):
    """A person-shaped arrangement of the LIP labels, shifted a little from picture to picture."""
    L = styles.LIP.label2id
    out = np.zeros((n, h, w), dtype=np.uint8)
    for i, s in enumerate(out):
        d = i % 5
        s[10 + d:30 + d, 70:110] = L['hair']
        s[4 + d:12 + d, 72:108] = L['hat']
        s[26 + d:60 + d, 74:106] = L['face']
        s[36 + d:42 + d, 78:102] = L['eyeglass']
        s[62 + d:140, 50 + d:126] = L['top']
        s[62 + d:150, 40:56 + d] = L['coat']
        s[140:228, 56:120 - d] = L['pants']
        s[228:250, 56:84] = L['left-shoe']
        s[228:250, 92:120 - d] = L['right-shoe']
    return out


def host_path(pics, segm, seg):
    mean = np.array(CLIP_MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.array(CLIP_STD, dtype=np.float32).reshape(3, 1, 1)
    out = np.zeros((len(pics), len(style_names), 224, 224, 3), dtype=np.uint8)
    for b, (pic, s) in enumerate(zip(pics, segm)):
        h, w = s.shape
        for name, ids in seg.group_ids.items():
            mask = np.isin(s, ids)
            m = torch.from_numpy(mask)
            cols, rows = torch.sum(m.to(torch.float32), dim=0).numpy(), torch.sum(m.to(torch.float32), dim=1).numpy()
            cn, rn = np.nonzero(cols > 0.1)[0], np.nonzero(rows > 0.1)[0]
            left, right, top, bottom = (int(cn[0]), int(cn[-1]), int(rn[0]), int(rn[-1])) if cn.size else (0, w, 0, h)
            if name == 'background':
                if not mask.any():
                    continue
                fill = [int(pic[..., c][mask].astype(np.int64).sum()) // int(mask.sum()) for c in range(3)]
                x = np.where(mask[..., None], pic, np.array(fill, dtype=np.uint8))
            else:
                x = (pic * mask[..., None] if name != 'face' else pic)[top:bottom, left:right]
                ch, cw = x.shape[:2]
                if ch <= 0 or cw <= 0 or (name == 'face' and ch > 128):
                    continue
                p = (ch - cw) // 2
                x = np.pad(x, ((max(-p, 0),) * 2, (max(p, 0),) * 2, (0, 0)))
            ph, pw = x.shape[:2]
            oh, ow = (int(224 * ph / pw), 224) if pw <= ph else (224, int(224 * pw / ph))
            if (oh, ow) != (ph, pw):
                x = np.asarray(Image.fromarray(np.ascontiguousarray(x)).resize((ow, oh), Image.BILINEAR))
            t, l = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
            out[b, style_names.index(name)] = x[t:t + 224, l:l + 224]
    f = (out.transpose(0, 1, 4, 2, 3).astype(np.float32) / np.float32(255) - mean) / std
    return torch.from_numpy(np.ascontiguousarray(f)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of the kernels"
    assert a.rounds >= 20, "the median of at least 20 runs"
    H, W, seg = 256, 176, styles.LIP
    pics = np.random.default_rng(0).integers(0, 256, (a.n, H, W, 3), dtype=np.uint8)
    segm = label_maps(a.n, H, W)
    dp, ds = torch.from_numpy(pics).cuda(), torch.from_numpy(segm).cuda()
    got, valid, _ = styles.style_crops(dp, ds, seg)
    host = host_path(pics, segm, seg)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), host.view(torch.int32)), "the two paths differ"
    ctx = _lib.get_context(dp.device)
    ctx.lib.upk_kernel_launches(ctx.h, 1)
    styles.style_crops(dp, ds, seg)
    launches = int(ctx.lib.upk_kernel_launches(ctx.h, 0))

    def device_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        styles.style_crops(dp, ds, seg)
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
        device_ms(), wall_ms(lambda: host_path(pics, segm, seg))
    k = [device_ms() for _ in range(a.rounds)]
    kw = [wall_ms(lambda: styles.style_crops(dp, ds, seg)) for _ in range(a.rounds)]
    p = [wall_ms(lambda: host_path(pics, segm, seg)) for _ in range(a.rounds)]
    med = statistics.median
    print("%d pictures of %d x %d, LIP groups, %d valid crops of %d slots" % (a.n, H, W, int(valid.sum()), valid.numel()))
    print("  device: style_crops %.4f ms between HIP events (min %.4f, max %.4f), %.4f ms wall with a synchronise, %d launch(es)"
          % (med(k), min(k), max(k), med(kw), launches))
    print("  host:   mask + range + cut / fill + pad + PIL resize + crop + normalise + upload %.2f ms wall (min %.2f, max %.2f)"
          % (med(p), min(p), max(p)))
    print(json.dumps(dict(n=a.n, h=H, w=W, segmenter="lip", valid=int(valid.sum()), slots=int(valid.numel()), rounds=a.rounds,
                          launches=launches, device_event_ms=dict(median=med(k), min=min(k), max=max(k)), device_wall_ms=med(kw),
                          host_wall_ms=dict(median=med(p), min=min(p), max=max(p)))))


if __name__ == "__main__":
    main()
