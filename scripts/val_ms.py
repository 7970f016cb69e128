"""Wall clock of the keyed validation path against the generator path it stands beside, in one process:
  (a) one validation_step of --model on a DeepFashion-shaped batch of 8 on the device (two forwards: live and EMA):
      unkeyed (torch.randint + randn_like + upk_q_sample_f32, the posterior from the generator) against keyed
      (upk_q_sample_keyed_f32, the posterior from upk_randn_keyed_f32), alternating within each of --rounds rounds;
  (b) evaluate.run_validation of the tiny model over a synthetic tree (tests/batch_ref.make_tree, --pairs pairs at
      256 x 192, batch_size --bs; PIL decodes every picture): the serial generator path (seed=) against noise_seed= at
      lanes 1, 2 and 4, alternating within each round after one warm-up run of each.
Median, min and max per variant, and one JSON line at the end.  A record, not a gate: no threshold, not a bench path."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import upgpt_amd  # noqa: E402
from upgpt_amd import data, evaluate, rng, synth  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(variants, rounds, warmup):
    for _ in range(warmup):
        for _, fn in variants:
            timed(fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            ms[name].append(timed(fn)[0])
    out = {}
    for name, v in ms.items():
        out[name] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print("  %-44s %9.3f ms (min %.3f, max %.3f over %d)" % (name, out[name]["median"], min(v), max(v), len(v)))
    return out


class WithEmbeddings:
    """txt and the style embeddings of the tiny model (its text stage is a pass-through), on the device."""

    def __init__(self, ds):
        self.ds = ds

    def batches(self, batch_size, batch_start=0, batch_step=1):
        for k, b in enumerate(self.ds.batches(batch_size, batch_start=batch_start, batch_step=batch_step)):
            n = len(b["fname"])
            g = torch.Generator().manual_seed(100 + batch_start + k * batch_step)
            yield dict(b, txt=torch.randn(n, 77, 768, generator=g).cuda(),
                       style_emb=(0.45 * torch.randn(n, 9, 768, generator=g)).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bbox")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--bs", type=int, default=4)
    ap.add_argument("--run_rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    result = {}

    model = upgpt_amd.build_model(a.model)
    synth.fill_module_(model)
    synth.fill_ema_(model, salt=1)
    model = model.cuda()
    B = 8
    g0 = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1, "txt": torch.randn(B, 77, 768, generator=g0),
             "styles": 0.45 * torch.randn(B, 9, 768, generator=g0), "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0),
             "person_mask": synth.person_mask(B, 32, 24), "loss_w": 0.5 + torch.rand(B, 1, 32, 24, generator=g0)}
    batch = {k: v.cuda() for k, v in batch.items()}
    keys = rng.NoiseKeys(7, range(B), device="cuda")
    keys.keys
    print("validation_step (%s, B = %d):" % (a.model, B))
    result["validation_step"] = alternate([("unkeyed (generator, upk_q_sample_f32)", lambda: model.validation_step(batch, 0)),
                                           ("keyed (upk_q_sample_keyed_f32)",
                                            lambda: model.validation_step(batch, 0, noise_keys=keys))], a.rounds, a.warmup)
    del model
    torch.cuda.empty_cache()

    import batch_ref as br
    extra = upgpt_amd.model_params("tiny")["extra_cond_stages"]
    extra["style_cond"] = dict(extra["style_cond"], cond_stage_key="style_emb")
    tiny = upgpt_amd.build_model("tiny", overrides={"extra_cond_stages": extra})
    synth.fill_module_(tiny)
    synth.fill_ema_(tiny, salt=1)
    tiny = tiny.cuda()
    with tempfile.TemporaryDirectory() as tmp:
        pairs = tuple((i % 6, (i + 1) % 6) for i in range(a.pairs))
        ds = data.DeepFashionPair(**dict(br.make_tree(tmp, pairs=pairs, pic=(256, 192), mask=(256, 256)),
                                         input_mask_type="bbox"))
        src = WithEmbeddings(ds)
        print("run_validation (tiny, %d samples, batch_size %d):" % (len(ds), a.bs))
        variants = [("serial, torch generator (seed=)", lambda: evaluate.run_validation(tiny, src, batch_size=a.bs, seed=5))]
        for lanes in (1, 2, 4):
            variants.append(("noise_seed=, lanes = %d" % lanes, (lambda n: lambda: evaluate.run_validation(
                tiny, src, batch_size=a.bs, noise_seed=7, lanes=n))(lanes)))
        result["run_validation"] = dict(samples=len(ds), batch_size=a.bs, ms=alternate(variants, a.run_rounds, 1))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
