#!/usr/bin/env python
"""Generates tests/golden/loss.npz: the reference's LatentDiffusion.p_losses (ddpm.py:1083-1123) run on CPU with the
recipe weights and recipe inputs, and the schedule tables it reads.

    python tests/golden/make_loss_golden.py

Recipe `tiny`, EMA shadow = its own recipe draw (fill_ema_(model, salt=1)), B = 2, latent 4 x 32 x 24, 87 context tokens.
x_start = 0.18215 * 4 * x_T, noise = row 0 of the noise table, both of synth_inputs(seed=SEED, steps=1); t = [999, 3]; the
loss weight map [B, 1, 32, 24] is 2.0 on rows 0-7, 1.0 on rows 8-19 and 0.5 on rows 20-31.  Stored: model_output with the
live and with the EMA weights (fp32), the loss_dict values (and the per-call total) of the three cases `w` (loss_w given),
`none` (loss_w=None) and `l1` (loss_type='l1', loss_w given) for both weight sets, lvlb_weights and the two q_sample
tables.  Inputs are not stored: the tests regenerate them from upgpt_amd/synth.py.  The stubs and the model builder come
from make_goldens.py, which is imported, not copied.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)  # installs the stubs and puts the reference's `ldm` on sys.path

synth = mg.synth
HW, C, NTOK, B, SEED = (32, 24), 4, 87, 2, 40
T = (999, 3)


def loss_inputs():
    """(x_start, noise, t, loss_w, cond) of the fixture; tests/test_loss_gpu.py builds the same from synth."""
    inp = synth.synth_inputs(B, HW, C, NTOK, 768, seed=SEED, steps=1)
    loss_w = torch.ones(B, 1, *HW)
    loss_w[:, :, 0:8] = 2.0
    loss_w[:, :, 20:32] = 0.5
    cond = {"c_crossattn": inp["c_crossattn"], "c_concat": [inp["c_concat"]]}
    return 0.18215 * 4.0 * inp["x_T"], inp["noise"][0], torch.tensor(T, dtype=torch.long), loss_w, cond


def main(out):
    model, _ = mg.build_reference("tiny")
    synth.fill_ema_(model, salt=1)
    assert not model.training and not model.learn_logvar
    x_start, noise, t, loss_w, cond = loss_inputs()
    g = {"lvlb_weights": model.lvlb_weights.numpy(), "sqrt_alphas_cumprod": model.sqrt_alphas_cumprod.numpy(),
         "sqrt_one_minus_alphas_cumprod": model.sqrt_one_minus_alphas_cumprod.numpy(),
         "t": np.asarray(T, dtype=np.int32), "seed": np.asarray(SEED)}
    taps = []
    apply_model = model.apply_model

    def tapped(*a, **k):
        taps.append(apply_model(*a, **k))
        return taps[-1]

    model.apply_model = tapped
    for weights in ("live", "ema"):
        for case, ltype, w in (("w", "l2", loss_w), ("none", "l2", None), ("l1", "l1", loss_w)):
            model.loss_type = ltype
            del taps[:]
            if weights == "ema":
                with model.ema_scope():
                    loss, d = model.p_losses(x_start, cond, t, noise=noise, loss_w=w)
            else:
                loss, d = model.p_losses(x_start, cond, t, noise=noise, loss_w=w)
            assert sorted(d) == ["val/loss", "val/loss_simple", "val/loss_vlb"], sorted(d)
            for k, v in d.items():
                g["%s/%s/%s" % (weights, case, k[4:])] = np.asarray(float(v), dtype=np.float64)
            g["%s/%s/total" % (weights, case)] = np.asarray(float(loss), dtype=np.float64)
            if case == "w":
                g["%s/model_output" % weights] = taps[0].numpy()
            print(weights, case, {k: "%.6g" % float(v) for k, v in d.items()}, flush=True)
    model.loss_type = "l2"
    assert float(np.abs(g["live/model_output"] - g["ema/model_output"]).max()) > 1e-3
    np.savez_compressed(out, **g)
    print("loss ->", out, {k: v.shape for k, v in g.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "loss.npz"))
    ap.add_argument("--seed", type=int, default=SEED)
    args = ap.parse_args()
    SEED = args.seed
    main(args.out)
