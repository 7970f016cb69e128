"""Wall time of test_step's image finishing: B = 8, 256 x 192 -> crop [256, 176], --styles crops of
224 x 224 per sample.  From the call to host-side uint8 arrays:
  (a) evaluate.finished_arrays: upk_image_finish_u8 launches into one uint8 device buffer, one copy, one synchronise
  (b) the reference's way (ddpm.py:1352-1377): the fp32 images copied to the host, crop / clamp / rescale /
      de-normalise / concat / mul(255).byte() with torch ops there
The samples and the reconstruction start on the device (where log_images leaves them), the batch on the host (where a
data loader leaves it) in both.  The two alternate within each of --rounds rounds after --warmup rounds of both;
median, min and max are printed, and one JSON line at the end.  The arrays of (a) and (b) are compared first."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from upgpt_amd import evaluate  # noqa: E402


def reference_way(log, batch, crop):
    """The reference's expressions on host tensors (torchvision's CenterCrop / Normalize / ToPILImage written out)."""
    def cc(x):
        top, left, ch, cw = evaluate.center_crop_window(x.shape[-2], x.shape[-1], crop)
        return x[..., top:top + ch, left:left + cw]

    u8 = lambda t: t.mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    out = {}
    for k, name in (("samples", "samples"), ("reconstruction", "recon")):
        out[name] = (torch.clamp(cc(log[k].detach().cpu()), -1., 1.) + 1.0) / 2.0
    for k, name in (("image", "gt"), ("src_image", "src"), ("smpl_image", "smpl")):
        out[name] = cc((batch[k].permute(0, 3, 1, 2) + 1.0) / 2.0)
    n = out["samples"].shape[0]
    out["concats"] = torch.cat([out[k][:n] for k in evaluate.CONCAT_ORDER], 3)
    d = torch.tensor([float(v) for v in evaluate.DENORM_D]).view(3, 1, 1)
    m = torch.tensor([float(v) for v in evaluate.DENORM_M]).view(3, 1, 1)
    st = batch["styles"]
    out["styles"] = torch.cat([st[:, s].sub(0.).div(d).sub(m).div(1.) for s in range(st.shape[1])], 3)
    return {k: u8(v[:n] if k != "styles" else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--styles", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    B, H, W, crop = a.bs, 256, 192, [256, 176]
    g = torch.Generator().manual_seed(0)
    model = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), crop_size=crop)
    log = {k: (0.8 * torch.randn(B, 3, H, W, generator=g)).cuda() for k in ("samples", "reconstruction")}
    batch = {k: torch.rand(B, H, W, 3, generator=g) * 2 - 1 for k in ("image", "src_image", "smpl_image")}
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 1, 3, 1, 1)
    batch["styles"] = (torch.rand(B, a.styles, 3, 224, 224, generator=g) - mean) / std
    variants = [("a device finishing (finished_arrays)", lambda: evaluate.finished_arrays(model, batch, log)),
                ("b host finishing (the reference's way)", lambda: reference_way(log, batch, crop))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    (_, ra), (_, rb) = timed(variants[0][1]), timed(variants[1][1])
    same = all(np.array_equal(ra[k], rb[k]) for k in rb)
    print("arrays of (a) and (b) identical:", same)
    assert same
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
        print("%-42s %8.3f ms (min %.3f, max %.3f over %d rounds)" % (name, res[name]["median"], min(v), max(v), len(v)))
    out_bytes = int(sum(v.size for v in ra.values()))
    print(json.dumps(dict(bs=B, styles=a.styles, rounds=a.rounds, uint8_bytes=out_bytes, ms=res)))


if __name__ == "__main__":
    main()
