"""Times of region-locked editing on the MI355X.  A record, not a gate: no threshold.

  1. The two launches alone, upk_region_mask_u8 (mask, keep and cells) and upk_composite_u8 (out and alpha), at
     [8, 256, 192] and [4, 512, 384], at the defaults (dilate 8, feather 4) and at the largest windows (dilate 32,
     feather 16): --burst launches back to back between two HIP events, divided by their number, so the figure is the
     launch in a stream that is kept busy; median (min .. max) over --rounds bursts after --warmup.
  2. InferenceModel.edit_region against InferenceModel.generate per call at the benchmark's shape (bbox model, 8 pictures
     of 256 x 192, --steps sampler steps), wall clock from entry to return (both end in a synchronise and a copy to the
     host), alternating in ONE process after a warm-up of both; median (min .. max) over --call-rounds.  generate samples
     the plain chain, edit_region encodes the picture and samples the masked chain: the difference is the masked chain's,
     the two launches above are a small part of it.
One JSON line at the end; --out also writes it to a file.  Needs a GPU; nothing here falls back."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import upgpt_amd  # noqa: E402
from upgpt_amd import _lib, edit, synth  # noqa: E402
from upgpt_amd.inference import InferenceModel  # noqa: E402
from upgpt_amd.rng import NoiseKeys  # noqa: E402
from upgpt_amd.styles import LIP  # noqa: E402

SHAPES = [(8, 256, 192), (4, 512, 384)]
WINDOWS = [(8, 4), (32, 16)]  # (dilate, feather)


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def show(r, unit="ms", fmt="%.4f"):
    return (fmt + " %s (" + fmt + " .. " + fmt + ")") % (r["median"], unit, r["min"], r["max"])


def label_maps(b, h, w):
    """A person-like map: a torso rectangle of `top` over `pants`, hair above, background around."""
    segm = np.zeros((b, h, w), dtype=np.uint8)
    segm[:, h // 16:h // 6, 3 * w // 8:5 * w // 8] = LIP.label2id['hair']
    segm[:, h // 5:h // 2, w // 4:3 * w // 4] = LIP.label2id['top']
    segm[:, h // 2:7 * h // 8, w // 3:2 * w // 3] = LIP.label2id['pants']
    return segm


def burst_ms(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / burst


def launches(a):
    ctx = _lib.get_context(torch.device("cuda", torch.cuda.current_device()))
    labels = edit.region_labels("top")
    rng = np.random.default_rng(0)
    out = []
    for b, h, w in SHAPES:
        segm = torch.from_numpy(label_maps(b, h, w)).cuda()
        orig, gen = (torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).cuda() for _ in range(2))
        mask = torch.empty((b, h, w), dtype=torch.uint8, device="cuda")
        keep = torch.empty((b, 1, h // 8, w // 8), device="cuda")
        cells = torch.empty((b,), dtype=torch.int32, device="cuda")
        res, alpha = torch.empty_like(orig), torch.empty_like(mask)
        for dilate, feather in WINDOWS:
            region = lambda: ctx.region_mask(segm, w, h * w, b, h, w, labels, dilate, 8, mask, w, h * w, keep, cells)
            comp = lambda: ctx.composite(orig, 3 * w, 3 * h * w, gen, 3 * w, 3 * h * w, mask, w, h * w, b, h, w, feather, res,
                                         3 * w, 3 * h * w, alpha, w, h * w)
            for _ in range(a.warmup):
                burst_ms(region, a.burst), burst_ms(comp, a.burst)
            rm, cm = [], []
            for _ in range(a.rounds):
                rm.append(burst_ms(region, a.burst)), cm.append(burst_ms(comp, a.burst))
            r = dict(batch=b, h=h, w=w, dilate=dilate, feather=feather, burst=a.burst, rounds=a.rounds, cells=cells.tolist(),
                     region_mask_ms=summary(rm), composite_ms=summary(cm))
            print("[%d, %d, %d] dilate %2d feather %2d: region_mask %s, composite %s per launch" % (
                b, h, w, dilate, feather, show(r["region_mask_ms"]), show(r["composite_ms"])))
            out.append(r)
    return out


def calls(a):
    with contextlib.redirect_stdout(io.StringIO()):
        model = upgpt_amd.build_model("bbox")
    synth.fill_module_(model)
    im = object.__new__(InferenceModel)  # (without the two CLIP towers of __init__: the batch carries embeddings)
    im.device, im.model = "cuda", model.cuda()
    b, (lh, lw) = 8, model.image_size
    f = 2 ** int(model.num_downs)
    h, w = f * lh, f * lw
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(1)
    picture = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).cuda()
    segm = torch.from_numpy(label_maps(b, h, w)).cuda()
    person = torch.full((b, 1, lh, lw), -1.0)
    person[:, :, 3:lh - 3, 4:lw - 3] = -0.99215686
    batch = {"txt": torch.randn(b, 77, 768, generator=g).cuda(), "styles": (0.45 * torch.randn(b, 9, 768, generator=g)).cuda(),
             "smpl": (0.5 * torch.randn(b, 1, 85, generator=g)).cuda(), "person_mask": person.cuda()}
    full = dict(batch, image=picture.float() / 127.5 - 1.0)
    keys = NoiseKeys(7, range(b), device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = {"generate": lambda: im.generate(full, a.steps, sampler=a.sampler, noise_keys=keys),
                "edit_region": lambda: im.edit_region(picture, segm, "top", batch, steps=a.steps, sampler=a.sampler, noise_keys=keys)}
    for _ in range(a.call_warmup):
        for fn in variants.values():
            timed(fn)
    ms = {k: [] for k in variants}
    for _ in range(a.call_rounds):  # (alternating: both see the same neighbours on a shared host)
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    out = dict(what="ms per call, bbox model, %d pictures of %d x %d, %d %s steps" % (b, h, w, a.steps, a.sampler),
               rounds=a.call_rounds, warmup=a.call_warmup, generate_ms=summary(ms["generate"]), edit_region_ms=summary(ms["edit_region"]))
    print(out["what"])
    for k in variants:
        print("  %-12s %s" % (k, show(out[k + "_ms"], fmt="%.2f")))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sampler", default="ddim")
    ap.add_argument("--call-rounds", type=int, default=8)
    ap.add_argument("--call-warmup", type=int, default=2)
    ap.add_argument("--skip-calls", action="store_true", help="the two launches only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_ms.py measures on the GPU: none is visible")
    out = {"device": torch.cuda.get_device_name(0), "launches": launches(a)}
    if not a.skip_calls:
        out["calls"] = calls(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
