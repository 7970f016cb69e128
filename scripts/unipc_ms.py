"""Call time of DPM-Solver++(2M) at 20 steps against UniPC at the step counts under discussion (12, 15, 20)
on the MI355X, at the benchmark's shape: bbox model, bs 8, 32x32 latent, sample() on the captured-graph fast path +
decode_first_stage, from entry to a device synchronise.  All run in ONE process and alternate within each of --rounds
rounds after a warm-up of all (plans, graphs, tables); median, min and max of the call time, the pictures per second at the
median and the time per step ((median - decode_only) / steps) are printed, then one JSON line.  No threshold: the only
expectation is that a UniPC step costs what a 2M step costs next to a UNet forward — compare the per-step figures of this
run.  Needs a GPU; nothing here falls back."""
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
import torch  # noqa: E402

import upgpt_amd  # noqa: E402
from upgpt_amd import synth  # noqa: E402
from upgpt_amd.dpm_solver import DPMSolverSampler  # noqa: E402
from upgpt_amd.unipc import UniPCSampler  # noqa: E402


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(32, 32))
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--unipc-steps", type=int, nargs="+", default=(12, 15, 20))
    ap.add_argument("--order", type=int, default=3, help="UniPC order at fewer steps than --dpm-steps; order 2 at as many")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="bbox")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unipc_ms.py measures on the GPU: none is visible")
    B, hw = a.bs, tuple(a.hw)
    with quiet():
        model = upgpt_amd.build_model(a.model)
    synth.fill_module_(model)
    model = model.cuda()
    inp = synth.synth_inputs(B, hw, 4, 87, 768, seed=0)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    x_T = inp["x_T"].cuda()
    kw = dict(x_T=x_T, verbose=False, log_every_t=10 ** 6)
    dpm = DPMSolverSampler(model)
    steps = {"dpmpp_2m_%d" % a.dpm_steps: a.dpm_steps}
    variants = [("dpmpp_2m_%d" % a.dpm_steps, lambda: dpm.sample(a.dpm_steps, B, (4,) + hw, cond, **kw)[0])]
    for S in a.unipc_steps:
        order = 2 if S >= a.dpm_steps else a.order
        name = "unipc%d_%d" % (order, S)
        steps[name] = S
        # (a sampler per step count: each keeps its schedule between calls, as a caller's would)
        variants.append((name, lambda S=S, order=order, s=UniPCSampler(model): s.sample(S, B, (4,) + hw, cond, order=order, **kw)[0]))
    variants.append(("decode_only", None))
    z_held = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with quiet(), model.ema_scope():
            z = fn() if fn is not None else z_held["z"]
            img = model.decode_first_stage(z)
        torch.cuda.synchronize()
        z_held["z"] = z
        assert bool(torch.isfinite(img).all()), name
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        for name, fn in variants:
            timed(name, fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(timed(name, fn))
    out = {"what": "sample() + decode_first_stage, ms per call of bs %d at %dx%d (%s model)" % (B, hw[0], hw[1], a.model),
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    decode = statistics.median(ms["decode_only"])
    for name, v in ms.items():
        r = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        tail = ""
        if name != "decode_only":
            r["images_per_s"] = B / (r["median_ms"] * 1e-3)
            r["ms_per_step"] = (r["median_ms"] - decode) / steps[name]
            tail = "  %7.2f images/s  %6.3f ms/step" % (r["images_per_s"], r["ms_per_step"])
        out[name] = r
        print("%-14s median %8.2f ms  min %8.2f  max %8.2f%s" % (name, r["median_ms"], r["min_ms"], r["max_ms"], tail))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
