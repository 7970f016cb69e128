"""What a caller can observe of every sampler chain, as records that two commits can be compared by.

Tiny model, seeded inputs, B = 2, 32 x 24, S = 6 (T = 6 for DDPM), log_every_t = 2.  Each case runs three times on one
sampler: without callbacks, with recording callbacks, and once more warm.  A record holds the SHA-256 of the final latent
and of every intermediate, the callbacks' arguments (tensors hashed) in call order, the printed lines, the bytes of
torch.cuda.get_rng_state() after the call, the upk_kernel_launches of the call and the sorted graph keys of every sampler
state; an exception is recorded by type and text.

    python scripts/chain_records.py --out a.json      # in a fresh process, at each commit
    python scripts/chain_records.py --compare a.json b.json

--compare prints the records that differ and exits non-zero when any does.  The paths run the same kernels in the same
order on the same bits, so no tolerance applies.  Needs a GPU; nothing here falls back."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HW, S = 2, (32, 24), 6
SHAPE = (4,) + HW


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(repr((str(t.dtype), tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


def hashed(v):
    import torch
    if torch.is_tensor(v):
        return sha(v)
    if isinstance(v, dict):
        return {k: hashed(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [hashed(x) for x in v]
    return v


class PassThrough:
    """A score corrector that returns its input: the chain takes the general path and computes the same."""
    def modify_score(self, model, e_t, x, t, c, **kw):
        return e_t


def cases(model):
    import torch
    from upgpt_amd import rng, synth
    from upgpt_amd.ddim import DDIMSampler
    from upgpt_amd.dpm_solver import DPMSolverSampler
    from upgpt_amd.plms import PLMSSampler
    from upgpt_amd.unipc import UniPCSampler
    inp = synth.synth_inputs(B, HW, 4, 87, 768, seed=7, steps=S)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    uc = {"c_crossattn": torch.zeros_like(cond["c_crossattn"]), "c_concat": cond["c_concat"]}
    x_T = inp["x_T"].cuda()
    x0 = (0.7 * synth.synth_inputs(B, HW, 4, 87, 768, seed=8)["x_T"]).cuda()
    mask = torch.zeros(B, 1, *HW, device="cuda")
    mask[:, :, 4:28, 6:18] = 1.
    keys = lambda: rng.NoiseKeys(11, range(B), device="cuda")
    guided = dict(unconditional_guidance_scale=3., unconditional_conditioning=uc)
    masked = dict(mask=mask, x0=x0)
    out = []

    def sampler_cases(name, cls, variants, **fixed):
        for tag, kw in variants:
            s = cls(model)
            out.append(("%s %s" % (name, tag), lambda cb, s=s, kw=kw: s.sample(
                S, B, SHAPE, cond, verbose=False, log_every_t=2, **dict(fixed, **kw), **cb)))

    def prepared(cls, **kw):  # a sampler whose schedule stands, for the calls below sample()
        s = cls(model)
        with contextlib.redirect_stdout(io.StringIO()):
            s.make_schedule(S, verbose=False, **kw)
        return s

    sampler_cases("ddim", DDIMSampler, [
        ("eta0 drawn", dict(eta=0.)), ("eta0 given", dict(eta=0., x_T=x_T)), ("eta1 drawn", dict(eta=1.)),
        ("eta1 given", dict(eta=1., x_T=x_T)), ("guided eta0", dict(eta=0., x_T=x_T, **guided)),
        ("guided eta1", dict(eta=1., x_T=x_T, **guided)), ("masked", dict(eta=1., x_T=x_T, **masked)),
        ("masked guided", dict(eta=1., x_T=x_T, **masked, **guided)), ("keyed", dict(eta=1., noise_keys=keys())),
        ("keyed masked", dict(eta=1., noise_keys=keys(), **masked))])
    s = prepared(DDIMSampler, ddim_eta=1.)
    out.append(("ddim decode", lambda cb, s=s: (s.decode(x_T, cond, 4), None)))
    out.append(("ddim decode guided", lambda cb, s=s: (s.decode(x_T, cond, 4, **guided), None)))
    out.append(("ddim timesteps=4", lambda cb, s=s: s.ddim_sampling(cond, (B,) + SHAPE, x_T=x_T, timesteps=4,
                                                                    log_every_t=2, **cb)))
    sampler_cases("plms", PLMSSampler, [("plain", dict(x_T=x_T)), ("guided", dict(x_T=x_T, **guided)),
                                        ("keyed", dict(noise_keys=keys()))])
    loop = lambda **kw: lambda cb: model.p_sample_loop(cond, (B,) + SHAPE, return_intermediates=True, timesteps=S,
                                                       log_every_t=2, **kw, **cb)
    out.append(("ddpm plain", loop()))
    out.append(("ddpm masked", loop(x_T=x_T, **masked)))
    out.append(("ddpm keyed", loop(noise_keys=keys())))
    out.append(("ddpm progressive", lambda cb: model.progressive_denoising(cond, (B,) + SHAPE, x_T=x_T, start_T=S,
                                                                           log_every_t=2, **cb)))
    corrected = dict(x_T=x_T, score_corrector=PassThrough())
    sampler_cases("dpm", DPMSolverSampler, [
        ("plain", dict(x_T=x_T)), ("guided", dict(x_T=x_T, **guided)), ("keyed", dict(noise_keys=keys())),
        ("order1", dict(x_T=x_T, order=1)), ("masked", dict(x_T=x_T, **masked)),
        ("masked keyed", dict(noise_keys=keys(), **masked)), ("corrector", corrected)])
    s = prepared(DPMSolverSampler)
    out.append(("dpm decode", lambda cb, s=s: (s.decode(x_T, cond, 4), None)))
    out.append(("dpm timesteps=4", lambda cb, s=s: s.dpm_sampling(cond, (B,) + SHAPE, x_T=x_T, timesteps=4, log_every_t=2,
                                                                  **cb)))
    sampler_cases("unipc", UniPCSampler, [
        ("order2", dict(x_T=x_T, order=2)), ("order3", dict(x_T=x_T, order=3)),
        ("guided order2", dict(x_T=x_T, order=2, **guided)), ("guided order3", dict(x_T=x_T, order=3, **guided)),
        ("keyed order2", dict(noise_keys=keys(), order=2)), ("keyed order3", dict(noise_keys=keys(), order=3)),
        ("order1", dict(x_T=x_T, order=1)), ("bh1", dict(x_T=x_T, variant="bh1")),
        ("no corrector", dict(x_T=x_T, corrector=False)), ("corrector", corrected),
        ("masked refusal", dict(x_T=x_T, **masked))])
    s = prepared(UniPCSampler, order=3)
    out.append(("unipc decode", lambda cb, s=s: (s.decode(x_T, cond, 4), None)))
    out.append(("unipc timesteps=4", lambda cb, s=s: s.unipc_sampling(cond, (B,) + SHAPE, x_T=x_T, timesteps=4,
                                                                      log_every_t=2, **cb)))
    return out


def record(model, ctx, fn, with_callbacks):
    import torch
    calls = []
    cb = {}
    if with_callbacks:
        cb = dict(callback=lambda i: calls.append(["callback", int(i)]),
                  img_callback=lambda x, i: calls.append(["img_callback", sha(x), int(i)]))
    torch.manual_seed(1234)
    n0 = int(ctx.lib.upk_kernel_launches(ctx.h, 0))
    text = io.StringIO()
    rec = {}
    try:
        with contextlib.redirect_stdout(text):
            z, inter = fn(cb)
        torch.cuda.synchronize()
        rec.update(final=sha(z), intermediates=hashed(inter))
    except Exception as e:  # (what a refused call raises is part of what a caller observes)
        rec.update(raised=type(e).__name__, message=str(e))
    rec.update(callbacks=calls, stdout=text.getvalue().splitlines(),
               rng_state=bytes(torch.cuda.get_rng_state().tolist()).hex(),
               launches=int(ctx.lib.upk_kernel_launches(ctx.h, 0)) - n0,
               graphs=sorted(repr((key[1:], kind, sorted(map(repr, st.graphs))))
                             for key, plan in model.model.diffusion_model._plans.items()
                             for kind, st in plan.sampler_states.items()))
    return rec


def run(out):
    import torch
    import upgpt_amd
    from upgpt_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("chain_records.py records on the GPU: none is visible")
    with contextlib.redirect_stdout(io.StringIO()):
        model = upgpt_amd.build_model("tiny")
    synth.fill_module_(model)
    model = model.cuda()
    ctx = _lib.get_context(0)
    records = {}
    for name, fn in cases(model):
        for run_name, with_callbacks in (("plain", False), ("callbacks", True), ("warm", False)):
            records["%s / %s" % (name, run_name)] = record(model, ctx, fn, with_callbacks)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
    print("%d records -> %s" % (len(records), out))


def compare(a, b):
    with open(a) as f:
        ra = json.load(f)
    with open(b) as f:
        rb = json.load(f)
    bad = 0
    for name in sorted(set(ra) | set(rb)):
        x, y = ra.get(name), rb.get(name)
        if x != y:
            bad += 1
            fields = sorted(k for k in set(x or {}) | set(y or {}) if (x or {}).get(k) != (y or {}).get(k))
            print("DIFFERS %s: %s" % (name, "missing on one side" if x is None or y is None else ", ".join(fields)))
            for k in fields if x is not None and y is not None else []:
                print("    %s: %r\n    %s  %r" % (k, x.get(k), " " * len(k), y.get(k)))
    print("%d of %d records identical" % (len(set(ra) | set(rb)) - bad, len(set(ra) | set(rb))))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="chain_records.json")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else run(a.out))
