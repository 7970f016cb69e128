"""Times of SDE-DPM-Solver++(2M) on the MI355X.  A record, not a gate: no threshold.

  1. The step kernel alone, upk_dpmpp_2m_sde_step_f32 without noise and mask, with noise, with noise and mask, against
     upk_dpmpp_2m_step_f32, at [8, 4, 32x24] and [4, 3, 128x96] (a second-order row, xin refreshed): --burst launches back to
     back between two HIP events, divided by their number; median (min .. max) over --rounds bursts after --warmup.
  2. sample() + decode_first_stage of the bbox model, 8 pictures at the model's latent size, guidance 3, keyed noise, on the
     captured path: the solver at --steps (20, 30) against DDIM eta = 1 at --ddim-steps (50, 200).
  3. The masked chain, LatentDiffusion.edit_images with 8 pictures as InferenceModel.edit_region calls it (its guidance
     arguments included, as log_images takes them): the solver at 20 steps on the captured path against sampler="dpmpp_2m"
     at 20 steps (its masked chains run step by step from Python) and masked DDIM at 50.
  2. and 3.: wall clock from entry to a device synchronise, all variants alternating in ONE process within each of
  --call-rounds rounds after a warm-up of all; median (min .. max).
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
from upgpt_amd import _lib, synth  # noqa: E402
from upgpt_amd.ddim import DDIMSampler  # noqa: E402
from upgpt_amd.dpm_sde import DPMSolverSDESampler  # noqa: E402
from upgpt_amd.rng import NoiseKeys  # noqa: E402
from upgpt_amd.schedule import dpm_coefficient_table, dpm_sde_coefficient_table  # noqa: E402

SHAPES = [(8, 4, 32 * 24), (4, 3, 128 * 96)]


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def show(r, fmt="%.4f"):
    return (fmt + " ms (" + fmt + " .. " + fmt + ")") % (r["median"], r["min"], r["max"])


def burst_ms(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / burst


def launches(a, acp):
    ctx = _lib.get_context(torch.device("cuda", torch.cuda.current_device()))
    from upgpt_amd.schedule import make_logsnr_timesteps
    node = make_logsnr_timesteps(acp, 20)
    alphas, alphas_prev = acp[node[1:]], acp[node[:-1]]
    ode, sde = dpm_coefficient_table(alphas, alphas_prev).cuda(), dpm_sde_coefficient_table(alphas, alphas_prev, 1.0).cuda()
    row = torch.tensor([5], dtype=torch.int32, device="cuda")  # a second-order row; no auto-advance: every launch reads it
    out = []
    for b, c, hw in SHAPES:
        n = b * c * hw
        rn = lambda *s: torch.randn(*s, device="cuda")
        x, eps, old, pred, plain = rn(n), rn(n), rn(n), rn(n), rn(n)
        noise, keep, mask = rn(20, n), rn(20, n), (rn(n) > 0).float()
        xin = torch.zeros(b * hw, 32, dtype=torch.float16, device="cuda")
        variants = {
            "dpmpp_2m": lambda: ctx.dpmpp_2m_step(x, eps, ode, row, old, pred, xin, 32, b, c, hw),
            "sde": lambda: ctx.dpmpp_2m_sde_step(x, eps, sde, None, None, None, 0, row, old, pred, None, xin, 32, b, c, hw),
            "sde_noise": lambda: ctx.dpmpp_2m_sde_step(x, eps, sde, noise, None, None, 0, row, old, pred, None, xin, 32, b, c, hw),
            "sde_noise_mask": lambda: ctx.dpmpp_2m_sde_step(x, eps, sde, noise, keep, mask, 20, row, old, pred, plain, xin, 32,
                                                            b, c, hw)}
        ms = {k: [] for k in variants}
        for r in range(a.warmup + a.rounds):
            for k, fn in variants.items():
                x.normal_()  # (the update is in place: keep the operands at unit scale)
                t = burst_ms(fn, a.burst)
                if r >= a.warmup:
                    ms[k].append(t)
        rec = dict(batch=b, c=c, hw=hw, burst=a.burst, rounds=a.rounds, **{k + "_ms": summary(v) for k, v in ms.items()})
        print("[%d, %d, %d] per launch: %s" % (b, c, hw, ", ".join("%s %s" % (k, show(rec[k + "_ms"])) for k in variants)))
        out.append(rec)
    return out


def calls(a, model):
    b, (lh, lw) = 8, model.image_size
    shape = (model.channels, lh, lw)
    inp = synth.synth_inputs(b, (lh, lw), model.channels, 87, 768, seed=0)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    keys = NoiseKeys(7, range(b), device="cuda")
    kw = dict(verbose=False, log_every_t=10 ** 6, unconditional_guidance_scale=3.0, unconditional_conditioning=uc, noise_keys=keys)
    variants = {}
    for S in a.steps:  # (a sampler per step count: each keeps its schedule between calls, as a caller's would)
        variants["sde_%d" % S] = lambda S=S, s=DPMSolverSDESampler(model): s.sample(S, b, shape, cond, eta=1.0, **kw)[0]
    for S in a.ddim_steps:
        variants["ddim_eta1_%d" % S] = lambda S=S, s=DDIMSampler(model): s.sample(S, b, shape, cond, eta=1.0, **kw)[0]

    f = 2 ** int(model.num_downs)
    g = torch.Generator().manual_seed(0)
    person = torch.full((b, 1, lh, lw), -1.0)
    person[:, :, 3:lh - 3, 4:lw - 3] = -0.99215686
    batch = {"image": (torch.rand(b, f * lh, f * lw, 3, generator=g) * 2 - 1).cuda(), "txt": torch.randn(b, 77, 768, generator=g).cuda(),
             "styles": (0.45 * torch.randn(b, 9, 768, generator=g)).cuda(), "smpl": (0.5 * torch.randn(b, 1, 85, generator=g)).cuda(),
             "person_mask": person.cuda()}
    keep = torch.ones(b, 1, lh, lw, device="cuda")
    keep[:, :, lh // 5:lh // 2, lw // 4:3 * lw // 4] = 0.0
    ekw = dict(N=b, noise_keys=keys, use_ema=True, unconditional_guidance_scale=3., unconditional_guidance_label=[""])
    edits = {"edit_sde_20": lambda: model.edit_images(batch, keep, ddim_steps=20, sampler="dpmpp_2m_sde", **ekw),
             "edit_dpmpp_2m_20": lambda: model.edit_images(batch, keep, ddim_steps=20, sampler="dpmpp_2m", **ekw),
             "edit_ddim_50": lambda: model.edit_images(batch, keep, ddim_steps=50, **ekw)}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with quiet(), torch.no_grad():
            if name.startswith("edit_"):
                img = fn()["samples"]
            else:
                with model.ema_scope():
                    img = model.decode_first_stage(fn())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img).all()), name
        return (time.perf_counter() - t0) * 1e3

    variants.update(edits)
    for _ in range(a.call_warmup):
        for name, fn in variants.items():
            timed(name, fn)
    ms = {name: [] for name in variants}
    for _ in range(a.call_rounds):  # (alternating: all see the same neighbours on a shared host)
        for name, fn in variants.items():
            ms[name].append(timed(name, fn))
    out = dict(what="ms per call, bbox model, %d pictures, latent %dx%d: sample() at guidance 3 + decode_first_stage; edit_images" % (
        b, lh, lw), rounds=a.call_rounds, warmup=a.call_warmup)
    for name, v in ms.items():
        out[name + "_ms"] = summary(v)
        print("  %-18s %s" % (name, show(out[name + "_ms"], "%.2f")))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, nargs="+", default=(20, 30))
    ap.add_argument("--ddim-steps", type=int, nargs="+", default=(50, 200))
    ap.add_argument("--call-rounds", type=int, default=5)
    ap.add_argument("--call-warmup", type=int, default=2)
    ap.add_argument("--skip-calls", action="store_true", help="the step kernel only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_sde_ms.py measures on the GPU: none is visible")
    with quiet():
        model = upgpt_amd.build_model("bbox")
    synth.fill_module_(model)
    model = model.cuda()
    out = {"device": torch.cuda.get_device_name(0), "launches": launches(a, model.alphas_cumprod.detach().cpu())}
    if not a.skip_calls:
        out["calls"] = calls(a, model)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
