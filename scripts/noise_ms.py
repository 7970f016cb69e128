"""What keyed noise costs and buys on the MI355X:
  (1) one sample() call at the reference's operating point — bbox model, bs 8, 32x24 latent, 200 DDIM steps, eta 1 — from
      entry to a device synchronise, with noise_keys (one upk_randn_keyed_f32 launch for the table) against the
      torch-generator path of the same tree (200 torch.randn calls, 200 row copies, one mul_).  The two alternate
      within each of --rounds rounds after a warm-up of both; median, min and max are printed.  The part in front of the
      first graph launch (draws, tables) is timed separately with a synchronise of its own in a second pass.
  (2) evaluate.run_split over a synthetic tree of --pairs pairs (tests/batch_ref.make_tree) on the tiny model with
      style embeddings, noise_seed set, lanes=1 against lanes=--lanes: wall time of the whole call, files written included.
      Both take the lanes' tuning table (_lib.shared_chip), so the comparison is lanes against no lanes and not table
      against table.  One warm-up call of each builds plans and graphs.
One JSON line at the end."""
import argparse
import contextlib
import io
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
from upgpt_amd import _lib, data, evaluate, rng, synth  # noqa: E402
from upgpt_amd.ddim import DDIMSampler  # noqa: E402


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def sample_ms(a):
    B, S, hw = a.bs, a.steps, (32, 24)
    with quiet():
        model = upgpt_amd.build_model("bbox")
    synth.fill_module_(model)
    model = model.cuda()
    inp = synth.synth_inputs(B, hw, 4, 87, 768, seed=0)
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    keys = rng.NoiseKeys(1, range(B), device="cuda")
    keys.keys
    sampler = DDIMSampler(model)
    kw = dict(eta=1.0, verbose=False, log_every_t=10 ** 6)
    variants = [("keyed", lambda: sampler.sample(S, B, (4,) + hw, cond, noise_keys=keys, **kw)[0]),
                ("torch generator", lambda: sampler.sample(S, B, (4,) + hw, cond, **kw)[0])]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with quiet(), model.ema_scope():
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        for _, fn in variants:
            timed(fn)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(timed(fn))
    # the part in front of the loop: the same call with the graph launches taken out (SamplerState.launch is a no-op)
    from upgpt_amd import engine
    launch = engine.SamplerState.launch
    engine.SamplerState.launch = lambda self, *args, **k: None
    pre = {name: [] for name, _ in variants}
    try:
        for _ in range(a.rounds):
            for name, fn in variants:
                pre[name].append(timed(fn))
    finally:
        engine.SamplerState.launch = launch
    res = {}
    for name, _ in variants:
        res[name] = dict(call_ms=stats(ms[name]), before_loop_ms=stats(pre[name]))
        print("%-16s sample() %8.2f ms (min %.2f, max %.2f over %d rounds); before the loop %6.3f ms (min %.3f, max %.3f)" % (
            name, res[name]["call_ms"]["median"], min(ms[name]), max(ms[name]), a.rounds, res[name]["before_loop_ms"]["median"],
            min(pre[name]), max(pre[name])))
    return res


class WithEmbeddings:
    """txt / style embeddings for the tiny model (pass-through stages), made with the batch and already on the device."""

    def __init__(self, ds):
        self.ds = ds

    def batches(self, batch_size):
        for i, b in enumerate(self.ds.batches(batch_size)):
            g = torch.Generator().manual_seed(i)
            n = len(b["fname"])
            yield dict(b, txt=torch.randn(n, 77, 768, generator=g).cuda(),
                       style_emb=(0.45 * torch.randn(n, 9, 768, generator=g)).cuda())


def split_s(a):
    import batch_ref as br
    extra = upgpt_amd.model_params("tiny")["extra_cond_stages"]
    extra["style_cond"] = dict(extra["style_cond"], cond_stage_key="style_emb")
    with quiet():
        model = upgpt_amd.build_model("tiny", overrides={"extra_cond_stages": extra})
    synth.fill_module_(model)
    synth.fill_ema_(model, salt=1)
    model = model.cuda()
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        n_img = a.pairs + 1
        kw = dict(br.make_tree(os.path.join(tmp, "data"), n_images=n_img, pairs=tuple((i, i + 1) for i in range(a.pairs)),
                               pic=(256, 192), mask=(256, 256)), input_mask_type="mask")  # (the tree's masks shrink with the
        # image index and are empty past image 27: 'bbox' would refuse them)
        ds = data.DeepFashionPair(**kw)
        assert len(ds) == a.pairs

        def run(lanes, tag):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with quiet(), _lib.shared_chip(a.lanes):
                evaluate.run_split(model, WithEmbeddings(ds), os.path.join(tmp, tag), batch_size=a.bs, lanes=lanes,
                                   noise_seed=7, ddim_steps=a.split_steps, ddim_eta=1.0)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for lanes in (1, a.lanes):
            run(lanes, "warm%d" % lanes)
        t = {1: [], a.lanes: []}
        for r in range(a.split_rounds):
            for lanes in (1, a.lanes):
                t[lanes].append(run(lanes, "r%d_%d" % (r, lanes)))
        for lanes in (1, a.lanes):
            res["lanes=%d" % lanes] = dict(stats(t[lanes]), images_per_s=a.pairs / statistics.median(t[lanes]))
            print("run_split lanes=%d: %7.2f s (min %.2f, max %.2f over %d rounds), %.1f pairs/s" % (
                lanes, statistics.median(t[lanes]), min(t[lanes]), max(t[lanes]), a.split_rounds,
                a.pairs / statistics.median(t[lanes])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--split-steps", type=int, default=50)
    ap.add_argument("--split-rounds", type=int, default=3)
    ap.add_argument("--only", choices=("sample", "split"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    out = {}
    if a.only in (None, "sample"):
        out["sample"] = sample_ms(a)
    if a.only in (None, "split"):
        out["run_split"] = split_s(a)
    print(json.dumps(dict(out, bs=a.bs, steps=a.steps, pairs=a.pairs, lanes=a.lanes, split_steps=a.split_steps)))


if __name__ == "__main__":
    main()
