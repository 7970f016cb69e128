"""ms per DDIM step of the editing calls against plain generation: bbox model, bs 8, 32x24 latent,
50 steps, eta 0.  One sample() call, from entry to a device synchronise, divided by its steps:
  (a) plain generation on the captured-graph path
  (b) sample(mask=, x0=), unguided, on the captured-graph path
  (c) the same, guided at scale 3 (dict conditioning)
  (d) sample(mask=, x0=), unguided, on the step-by-step general path (DDIMSampler._fast_ok forced to False: the path
      every masked call took before upk_ddim_step_edit_f32)
  (e) decode(x, cond, 25) on the captured-graph path, per step of its 25
The variants alternate within each of --rounds rounds after a warm-up of every variant; median, min and max over the
rounds are printed, and one JSON line at the end."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import upgpt_amd  # noqa: E402
from upgpt_amd import synth  # noqa: E402
from upgpt_amd.ddim import DDIMSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="bbox")
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    B, S, hw = a.bs, a.steps, (32, 24)
    with contextlib.redirect_stdout(io.StringIO()):
        model = upgpt_amd.build_model(a.kind)
    synth.fill_module_(model)
    model = model.cuda()
    inp = synth.synth_inputs(B, hw, 4, 87, 768, seed=0, steps=S)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    x_T = inp["x_T"].cuda()
    x0 = (0.7 * synth.synth_inputs(B, hw, 4, 87, 768, seed=1)["x_T"]).cuda()
    mask = torch.ones(B, 1, *hw, device="cuda")
    mask[:, :, hw[0] // 4:3 * hw[0] // 4, hw[1] // 4:3 * hw[1] // 4] = 0.
    sampler = DDIMSampler(model)
    kw = dict(eta=0.0, x_T=x_T, verbose=False, log_every_t=10 ** 6)
    guided = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    fast_ok = DDIMSampler._fast_ok

    def general():
        DDIMSampler._fast_ok = lambda self, *args, **k: False
        try:
            return sampler.sample(S, B, (4,) + hw, cond, mask=mask, x0=x0, **kw)[0]
        finally:
            DDIMSampler._fast_ok = fast_ok

    variants = [
        ("a plain, graph path", S, lambda: sampler.sample(S, B, (4,) + hw, cond, **kw)[0]),
        ("b masked, graph path", S, lambda: sampler.sample(S, B, (4,) + hw, cond, mask=mask, x0=x0, **kw)[0]),
        ("c masked guided 3.0, graph path", S, lambda: sampler.sample(S, B, (4,) + hw, cond, mask=mask, x0=x0, **guided,
                                                                      **kw)[0]),
        ("d masked, general path", S, general),
        ("e decode from the middle, graph path", S // 2, lambda: sampler.decode(x_T, cond, S // 2)),
    ]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()), model.ema_scope():
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(a.warmup):
        for _, _, fn in variants:
            timed(fn)
    ms = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, n, fn in variants:
            t, _ = timed(fn)
            ms[name].append(t / n)
    res = {}
    for name, _, _ in variants:
        v = ms[name]
        res[name] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print("%-40s %8.3f ms/step (min %.3f, max %.3f over %d rounds)" % (name, res[name]["median"], min(v), max(v), len(v)))
    med = lambda k: res[k]["median"]
    res["b/a"] = med("b masked, graph path") / med("a plain, graph path")
    res["d/b"] = med("d masked, general path") / med("b masked, graph path")
    print("b/a = %.3f   d/b = %.2f" % (res["b/a"], res["d/b"]))
    print(json.dumps(dict(kind=a.kind, bs=B, steps=S, rounds=a.rounds, ms_per_step=res)))


if __name__ == "__main__":
    main()
