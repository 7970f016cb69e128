#!/usr/bin/env python
"""Generates tests/golden/ddpm.npz: the reference's DDPM ancestral sampler (ddpm.py:1125-1310) and the DDPM /
plotting branches of its log_images (ddpm.py:1380-1499), run on CPU with the recipe weights and recipe noise.

    python tests/golden/make_ddpm_golden.py [--jobs 4]

Only outputs are stored, never the noise: the GPU tests regenerate it from upgpt_amd/synth.py (a 1000-step table is
about 24 MB).  Final latents are stored at full resolution; the logged intermediates 2x2 average-pooled, to keep the
file small.  The posterior noise of every step (ddpm.noise_like) and the q_sample noise of the masked loop
(torch.randn_like inside q_sample) are fed from those tables in the reference's draw order.  The stubs, the model
builder and the feeds come from make_goldens.py, which is imported, not copied.
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
import ldm.models.diffusion.ddpm as ref_ddpm  # noqa: E402

synth = mg.synth
HW, C, NTOK = (32, 24), 4, 87


class RandnLikeFeed:
    """torch.randn_like(x) (the q_sample noise of ddpm.py:282) returns the next slice of `noise`."""

    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def __enter__(self):
        self.orig = torch.randn_like
        feed = self

        def randn_like(x, *a, **k):
            n = feed.noise[feed.i].to(x.dtype)
            assert n.shape == x.shape, (n.shape, x.shape)
            feed.i += 1
            return n

        torch.randn_like = randn_like
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.orig


def pool2(inter):
    """[n, B, C, H, W] list of intermediates -> 2x2 average-pooled fp32 array."""
    x = torch.stack(inter)
    return torch.nn.functional.avg_pool2d(x.flatten(0, 1), 2).reshape(*x.shape[:3], x.shape[3] // 2, -1).numpy()


def _inputs(B, seed, T):
    inp = synth.synth_inputs(B, HW, C, NTOK, 768, seed=seed, steps=T)
    cond = {"c_crossattn": inp["c_crossattn"], "c_concat": [inp["c_concat"]]}
    return inp, cond


def item_chain(g):
    """1. tiny, B = 2, the full 1000-step p_sample_loop, log_every_t = 200."""
    model, _ = mg.build_reference("tiny")
    inp, cond = _inputs(2, 40, 1000)
    ref_ddpm.noise_like = mg.NoiseFeed(inp["noise"])
    z, inter = model.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].clone(),
                                   verbose=False, log_every_t=200)
    assert ref_ddpm.noise_like.i == 1000
    g["chain/z"] = z.numpy()
    g["chain/inter_pool2"] = pool2(inter)


def item_progressive(g):
    """2. tiny, B = 2, progressive_denoising(start_T=200, temperature=0.7, log_every_t=50): the x0 intermediates."""
    model, _ = mg.build_reference("tiny")
    inp, cond = _inputs(2, 41, 200)
    ref_ddpm.noise_like = mg.NoiseFeed(inp["noise"])
    z, inter = model.progressive_denoising(cond, (C,) + HW, verbose=False, batch_size=2, x_T=inp["x_T"].clone(),
                                           start_T=200, temperature=0.7, log_every_t=50)
    assert ref_ddpm.noise_like.i == 200
    g["prog/z"] = z.numpy()
    g["prog/inter_pool2"] = pool2(inter)


def item_mask(g):
    """3. tiny, B = 2, p_sample_loop(timesteps=200) with the centre-square mask of log_images and x0."""
    model, _ = mg.build_reference("tiny")
    inp, cond = _inputs(2, 42, 200)
    q = synth.synth_inputs(2, HW, C, NTOK, 768, seed=43, steps=200)
    x0 = 0.18215 * 4.0 * q["x_T"]
    mask = torch.ones(2, *HW)
    h, w = HW
    mask[:, h // 4:3 * h // 4, w // 4:3 * w // 4] = 0.
    mask = mask[:, None]
    ref_ddpm.noise_like = mg.NoiseFeed(inp["noise"])
    with RandnLikeFeed(q["noise"]) as feed:
        z, inter = model.p_sample_loop(cond, (2, C) + HW, return_intermediates=True, x_T=inp["x_T"].clone(),
                                       verbose=False, timesteps=200, mask=mask, x0=x0, log_every_t=50)
    assert ref_ddpm.noise_like.i == 200 and feed.i == 200
    g["mask/z"] = z.numpy()
    g["mask/inter_pool2"] = pool2(inter)


def item_bbox(g):
    """4. bbox, B = 1, p_sample_loop(timesteps=100)."""
    model, _ = mg.build_reference("bbox")
    inp, cond = _inputs(1, 44, 100)
    ref_ddpm.noise_like = mg.NoiseFeed(inp["noise"])
    z, inter = model.p_sample_loop(cond, (1, C) + HW, return_intermediates=True, x_T=inp["x_T"].clone(),
                                   verbose=False, timesteps=100)
    g["bbox/z"] = z.numpy()
    g["bbox/inter_pool2"] = pool2(inter)


def item_log_images(g):
    """5. tiny log_images (EMA shadow != live weights, the a15 batch):
    a. ddim_steps=None (DDPM, timesteps=50 forwarded to sample()), seeded x_T, fed posterior noise;
    b. DDIM 5 steps with inpaint, plot_diffusion_rows and plot_denoise_rows, zero DDIM noise: the key set, the shapes
       of every make_grid input and the denoise-row stack.
    The posterior sample z of get_input is not pinned: the denoise stack and the DDPM samples do not depend on it, and
    the values of the inpainting / outpainting samples and of the diffusion row are not stored (they also depend on x_T
    and noise the reference draws inside those runs), only the key set and the grid shapes."""
    model, _ = mg.build_reference("tiny")
    synth.fill_ema_(model, salt=1)
    B = 2
    batch = mg.a15_batch(B)
    x_T = synth.synth_inputs(1, HW, C, NTOK, 768, seed=11)["x_T"]
    noise = synth.synth_inputs(B, HW, C, NTOK, 768, seed=45, steps=50)["noise"]
    torch.manual_seed(1234)
    ref_ddpm.noise_like = mg.NoiseFeed(noise)
    with mg.RandnFeed(x_T) as feed:
        log = model.log_images(batch, N=B, ddim_steps=None, seed=11, timesteps=50)
    assert feed.hits == 1 and ref_ddpm.noise_like.i == 50
    g["log_ddpm/keys"] = np.asarray(sorted(log))
    g["log_ddpm/samples_pool8"] = mg.pool8(log["samples"])
    z, c = model.get_input(batch, "image", force_c_encode=True, bs=B)[:2]
    ref_ddpm.noise_like = mg.NoiseFeed(noise)
    with model.ema_scope():
        zs, inter = model.sample_log(cond=c, batch_size=B, ddim=False, ddim_steps=None, x_T=x_T.repeat(B, 1, 1, 1),
                                     timesteps=50)
    g["log_ddpm/samples_z"] = zs.numpy()
    g["log_ddpm/n_inter"] = np.asarray(len(inter))

    grids = []

    def make_grid(t, nrow=8, **k):
        grids.append((tuple(t.shape), int(nrow), t.clone()))
        return torch.zeros(3, 4, 4)

    ref_ddpm.make_grid = make_grid
    mg.ref_ddim.noise_like = mg.NoiseFeed(None)
    torch.manual_seed(1234)
    with mg.RandnFeed(x_T):
        log = model.log_images(batch, N=B, ddim_steps=5, seed=11, inpaint=True, plot_diffusion_rows=True,
                               plot_denoise_rows=True)
    g["log_ddim/keys"] = np.asarray(sorted(log))
    g["log_ddim/mask"] = log["mask"].numpy()
    g["log_ddim/grid_shapes"] = np.asarray([s for s, _, _ in grids])
    g["log_ddim/grid_nrow"] = np.asarray([n for _, n, _ in grids])
    g["log_ddim/denoise_stack_pool8"] = mg.pool8(grids[1][2]).astype(np.float16)


def item_table(g):
    """The per-step scalars of p_sample and q_sample from the reference model's buffers, combined as ddpm.py does in
    fp32, timesteps 999 ... 0: the rows of upk_ddpm_step_f32."""
    model, _ = mg.build_reference("tiny")
    t = torch.arange(model.num_timesteps - 1, -1, -1)
    ex = lambda buf: ref_ddpm.extract_into_tensor(buf, t, (t.shape[0], 1)).reshape(-1)
    nonzero = 1 - (t == 0).float()
    g["table"] = torch.stack([ex(model.sqrt_recip_alphas_cumprod), ex(model.sqrt_recipm1_alphas_cumprod),
                              ex(model.posterior_mean_coef1), ex(model.posterior_mean_coef2),
                              nonzero * (0.5 * ex(model.posterior_log_variance_clipped)).exp(),
                              ex(model.sqrt_alphas_cumprod), ex(model.sqrt_one_minus_alphas_cumprod),
                              torch.zeros(t.shape[0])], dim=1).numpy()


ITEMS = (item_chain, item_progressive, item_mask, item_bbox, item_log_images, item_table)


def _run(i):
    torch.set_num_threads(max(1, int(os.environ.get("DDPM_GOLDEN_THREADS", "2"))))
    g = {}
    ITEMS[i](g)
    print("done:", ITEMS[i].__name__, flush=True)
    return g


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(HERE, "ddpm.npz"))
    ap.add_argument("--only", nargs="*", help="regenerate these items (item_* names without the prefix) into --out")
    args = ap.parse_args()
    todo = [i for i, f in enumerate(ITEMS) if not args.only or f.__name__[5:] in args.only]
    if args.jobs > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(args.jobs) as pool:
            parts = pool.map(_run, todo, chunksize=1)
    else:
        parts = [_run(i) for i in todo]
    g = dict(np.load(args.out)) if args.only else {}
    g.update({k: v for p in parts for k, v in p.items()})
    g = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in g.items()}
    np.savez_compressed(args.out, **g)
    print("ddpm ->", args.out, {k: v.shape for k, v in g.items()})
