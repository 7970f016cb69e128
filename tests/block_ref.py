"""Per-block, per-sample criterion for the UNet and the VAE as the engine wires them (tests/test_unet_blocks_gpu.py runs it
on the device, tests/test_unet_blocks_host.py shows on the CPU what it catches and recomputes its bounds).

Reference: the live oracle in fp64 on recipe weights.  Two measures per tap and per sample, over that sample's C*H*W values:
    rel_mse = mean((got - ref)^2) / mean(ref^2)          peak = max |got - ref| / sqrt(mean(ref^2))
Bound: E_mse[tap], E_peak[tap] = the maxima over the case's samples of the same two measures for the SAME oracle with every
layer output rounded through fp16 (the project's model of fp16 storage, as range_ref.E_SEAM) against the fp64 oracle; the
tables below were computed on the CPU and the host test recomputes them to 2 %.  Criterion: measure <= MARGIN * E for every
tap, every sample and both measures; the margin is the one of test_tiny_unet_with_residual_streams_of_1e3 (the HIP path has
fp16 seams inside a block, t0 / t1 / h / q, k, v, that the oracle's layer-boundary rounding does not model).  Nothing here
is derived from device output."""
import functools

import torch
import torch.nn.functional as F

from oracle import unet as o_unet
from oracle import vae as o_vae
from upgpt_amd import synth

F64 = torch.float64
MARGIN = 4.0
UNET_PREFIX = "model.diffusion_model."


def seam(v):
    """fp16 round trip: the storage-precision model of an activation."""
    return v.half().to(v.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# cases
T8 = (981, 401, 21, 1, 500, 777, 901, 141)
UNETS = {"bbox": synth.BBOX_UNET, "upscale": synth.UPSCALE_UNET, "tiny": synth.TINY_UNET}
CASES = {
    # the bench shape: "auto" takes the fused head, cross and feed-forward kernels at the 32x32 level
    "A": dict(kind="bbox", B=8, H=32, W=32, ntok=87, C=4, cc=1, t=T8, seed=21),
    # lower levels of 192 / 48 / 12 tokens: the V^T key padding (vt_ld = 64, 32) is live
    "B": dict(kind="bbox", B=8, H=32, W=24, ntok=87, C=4, cc=1, t=T8, seed=22),
    "C": dict(kind="upscale", B=4, H=32, W=24, ntok=86, C=3, cc=3, t=T8[:4], seed=23),
    # the generic unfused path: head widths 12 / 24 / 48, 3-channel groups
    "D": dict(kind="tiny", B=3, H=32, W=24, ntok=87, C=4, cc=1, t=(1, 500, 999), seed=24),
    # sampler mode: one timestep row per step shared by the batch, the row picked by the device-side step counter
    "S": dict(kind="bbox", B=2, H=16, W=16, ntok=87, C=4, cc=1, t_rows=(981, 500, 21), steps=(0, 2), seed=25),
}


def overrides(kind):
    return {"image_size": [32, 24]} if kind == "upscale" else None


def boxes(B, h, w):
    """The one-channel concat map with a box of its own per sample (synth.person_mask is the same for every sample): the
    values of the bbox mask, -1 outside and -0.99215686 inside."""
    m = torch.full((B, 1, h, w), -1.0)
    for k in range(B):
        top, left = 1 + (2 * k) % (h // 4), 1 + (3 * k) % (w // 4)
        m[k, :, top: top + h // 4 + (5 * k) % (h // 2), left: left + w // 4 + (3 * k) % (w // 2)] = -0.99215686
    return m


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """{"x": latent [B, C, H, W], "cc": concat map, "ctx": context [B, ntok, 768], "t": timesteps [B]} of the device batch;
    every sample has its own of each."""
    c = CASES[name]
    inp = synth.synth_inputs(c["B"], (c["H"], c["W"]), c["C"], c["ntok"], 768, seed=c["seed"], concat_channels=c["cc"])
    cc = boxes(c["B"], c["H"], c["W"]) if c["cc"] == 1 else inp["c_concat"]
    t = torch.tensor(c["t"]) if "t" in c else None
    return {"x": inp["x_T"], "cc": cc, "ctx": inp["c_crossattn"], "t": t}


def oracle_batch(name):
    """(x with the concat map behind it, t, context) as the oracle takes them.  Case S: the device batch once per step,
    stacked along the batch (step-major), each copy at t_rows[step]."""
    c, i = CASES[name], case_inputs(name)
    x = torch.cat([i["x"], i["cc"]], 1)
    if "t" in c:
        return x, i["t"], i["ctx"]
    n = len(c["steps"])
    t = torch.tensor([c["t_rows"][s] for s in c["steps"] for _ in range(c["B"])])
    return x.repeat(n, 1, 1, 1), t, i["ctx"].repeat(n, 1, 1)


_STATE = {}


def state(kind, model=None):
    """Recipe weights of `kind` (fp32; the EMA copies left out).  model: a freshly built model to fill and read them from
    (the GPU tests' own), instead of one built here and dropped."""
    if model is not None or kind not in _STATE:
        import upgpt_amd
        sd = synth.fill_module_(model if model is not None else upgpt_amd.build_model(kind, overrides=overrides(kind)))
        _STATE[kind] = {k: v for k, v in sd.items() if not k.startswith("model_ema.")}
    return _STATE[kind]


def as_dtype(sd, dtype, prefix):
    return {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}


# ---------------------------------------------------------------------------------------------------------------------
# the UNet oracle, per block
def _forward_rewired(sd, cfg, x, t, ctx, taps, dtype, swap_skips=None, hs_first_at=None):
    """oracle.unet._unet_forward with two wiring hooks for the seeded defects (without a hook it is that function, which
    the host test asserts bit for bit).  swap_skips = (i, j): the entries i and j of hs change places.  hs_first_at = o:
    output block o concatenates [hs, h]."""
    prefix = UNET_PREFIX
    inputs, middle, outputs = o_unet.unet_layout(cfg)
    depth = cfg.get("transformer_depth", 1)
    temb = o_unet.timestep_embedding(t, cfg["model_channels"]).to(dtype)
    emb = o_unet._lin(sd, prefix + "time_embed.2", F.silu(o_unet._lin(sd, prefix + "time_embed.0", temb)))
    hs = []
    h = x.to(dtype)
    for i, layers in enumerate(inputs):
        h = o_unet._run_layers(sd, prefix, layers, h, emb, ctx, depth)
        hs.append(h)
        taps["input_blocks.%d" % i] = h
    if swap_skips is not None:
        i, j = swap_skips
        hs[i], hs[j] = hs[j], hs[i]
    h = o_unet._run_layers(sd, prefix, middle, h, emb, ctx, depth)
    taps["middle_block"] = h
    for i, layers in enumerate(outputs):
        h = torch.cat([hs.pop(), h] if i == hs_first_at else [h, hs.pop()], dim=1)
        h = o_unet._run_layers(sd, prefix, layers, h, emb, ctx, depth)
        taps["output_blocks.%d" % i] = h
    h = F.silu(o_unet._gn(sd, prefix + "out.0", h, 1e-5))
    return o_unet._conv(sd, prefix + "out.2", h)


@torch.no_grad()
def unet_taps(kind, x, t, ctx, round_fn=None, dtype=F64, sd=None, chunk=8, **rewire):
    """{tap: [B, C, H, W]} of the oracle with "eps" among them, `chunk` samples at a time (the oracle has no cross-sample
    operation).  sd: a state already in `dtype` (default: the recipe's).  rewire: the hooks of _forward_rewired."""
    sd = as_dtype(state(kind), dtype, UNET_PREFIX) if sd is None else sd
    ctx = ctx.to(dtype)
    parts = []
    for k in range(0, x.shape[0], chunk):
        taps, s = {}, slice(k, k + chunk)
        if rewire:
            prev, o_unet._ROUND = o_unet._ROUND, round_fn
            try:
                taps["eps"] = _forward_rewired(sd, UNETS[kind], x[s], t[s], ctx[s], taps, dtype, **rewire)
            finally:
                o_unet._ROUND = prev
        else:
            taps["eps"] = o_unet.unet_forward(sd, UNETS[kind], x[s], t[s], ctx[s], taps=taps, dtype=dtype, round_fn=round_fn)
        parts.append(taps)
    return {n: torch.cat([p[n] for p in parts]) for n in parts[0]}


@functools.lru_cache(maxsize=None)
def oracle_ref(name):
    """fp64 taps of a case, computed once per process and never written to."""
    return unet_taps(CASES[name]["kind"], *oracle_batch(name))


@functools.lru_cache(maxsize=None)
def oracle_seam(name):
    """The same with every layer output stored as fp16."""
    return unet_taps(CASES[name]["kind"], *oracle_batch(name), round_fn=seam)


def oracle_pair(name):
    return oracle_ref(name), oracle_seam(name)


def taps_nchw(plan):
    """{block name: [B, C, H, W]} of a UNetPlan's recorded activations (views of the plan's fp16 buffers) and "eps"."""
    out = {n: a.t[:, :a.C].reshape(a.B, a.H, a.W, a.C).permute(0, 3, 1, 2) for n, a in plan.taps.items()}
    out["eps"] = plan.eps
    return out


# ---------------------------------------------------------------------------------------------------------------------
# measures and criterion
def measures(got, ref):
    """(rel_mse [B], peak [B]) of got against ref, both [B, ...]."""
    ref = ref.to(F64).flatten(1)
    d = got.to(F64).flatten(1) - ref
    ms = (ref ** 2).mean(1)
    return (d ** 2).mean(1) / ms, d.abs().amax(1) / ms.sqrt()


def seam_error(ref, seamed):
    """{tap: (E_mse, E_peak)}: what fp16 storage alone costs, the maxima over the samples."""
    return {n: tuple(float(m.max()) for m in measures(seamed[n], ref[n])) for n in ref}


def ratios(got, ref, E, samples=None):
    """{tap: (rel_mse / (MARGIN E_mse) [B], peak / (MARGIN E_peak) [B])}; `samples` picks rows of ref when got holds
    only those."""
    out = {}
    for n in ref:
        r = ref[n] if samples is None else ref[n][list(samples)]
        ms, pk = measures(got[n], r)
        out[n] = (ms / (MARGIN * E[n][0]), pk / (MARGIN * E[n][1]))
    return out


def ratio_table(title, rt):
    """One row per tap: the worst ratio over the samples for both measures and which sample it was; -> the worst of all."""
    worst = 0.0
    print("\n%s\n%-18s %10s %3s  %10s %3s" % (title, "tap", "mse/4E", "at", "peak/4E", "at"))
    for n, (ms, pk) in rt.items():
        print("%-18s %10.3f %3d  %10.3f %3d" % (n, float(ms.max()), int(ms.argmax()), float(pk.max()), int(pk.argmax())))
        worst = max(worst, float(ms.max()), float(pk.max()))
    return worst


def failing(rt):
    """[(tap, sample)] whose ratio exceeds 1 in either measure, in tap order."""
    return [(n, k) for n, (ms, pk) in rt.items() for k in range(len(ms)) if float(ms[k]) > 1 or float(pk[k]) > 1]


def check(title, got, ref, E, samples=None):
    rt = ratios(got, ref, E, samples)
    worst = ratio_table(title, rt)
    bad = failing(rt)
    assert not bad, "%s: %d (tap, sample) over %g x E, first %s, worst ratio %.3f" % (title, len(bad), MARGIN, bad[0], worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the VAE, whole output per sample
VAE_PREFIX = "first_stage_model."
DDCONFIGS = {"bbox": synth.BBOX_DDCONFIG, "upscale": synth.UPSCALE_DDCONFIG}
VAE_B, VAE_LATENT = 3, (8, 6)
SCALE_FACTOR = 0.18215


def vae_factor(kind):
    return 2 ** (len(DDCONFIGS[kind]["ch_mult"]) - 1)


@functools.lru_cache(maxsize=None)
def vae_inputs(kind):
    """{"z": scaled latents [3, zc, 8, 6] as decode_first_stage takes them, "img": images [3, 3, 8 f, 6 f] in [-1, 1]}."""
    g = torch.Generator().manual_seed(77 + len(kind))
    h, w = VAE_LATENT
    f = vae_factor(kind)
    z = SCALE_FACTOR * 4.0 * torch.randn(VAE_B, DDCONFIGS[kind]["z_channels"], h, w, generator=g)
    return {"z": z, "img": torch.rand(VAE_B, 3, h * f, w * f, generator=g) * 2 - 1}


@torch.no_grad()
def vae_outputs(kind, round_fn=None, dtype=F64, sd=None, scale_factor=SCALE_FACTOR, samples=None):
    """{"decode": image, "moments": the encoder's moments} of the oracle."""
    sd = as_dtype(state(kind), dtype, VAE_PREFIX) if sd is None else sd
    i = vae_inputs(kind)
    s = slice(None) if samples is None else list(samples)
    return {"decode": o_vae.decode_first_stage(sd, DDCONFIGS[kind], i["z"][s], scale_factor, dtype=dtype, round_fn=round_fn),
            "moments": o_vae.encode_moments(sd, DDCONFIGS[kind], i["img"][s], dtype=dtype, round_fn=round_fn)}


@functools.lru_cache(maxsize=None)
def vae_ref(kind):
    return vae_outputs(kind)


@functools.lru_cache(maxsize=None)
def vae_seam(kind):
    return vae_outputs(kind, round_fn=seam)


def vae_pair(kind):
    return vae_ref(kind), vae_seam(kind)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds (tests/test_unet_blocks_host.py recomputes every entry to 2 %): {tap: (E_mse, E_peak)}
E = {
    "A": {
        "input_blocks.0": (4.322e-08, 2.000e-03), "input_blocks.1": (4.898e-07, 4.569e-03), "input_blocks.2": (7.927e-07, 5.485e-03),
        "input_blocks.3": (8.704e-07, 4.331e-03), "input_blocks.4": (1.197e-06, 5.976e-03), "input_blocks.5": (1.446e-06, 6.471e-03),
        "input_blocks.6": (1.429e-06, 5.962e-03), "input_blocks.7": (1.653e-06, 7.173e-03), "input_blocks.8": (1.821e-06, 6.679e-03),
        "input_blocks.9": (1.815e-06, 6.754e-03), "input_blocks.10": (1.867e-06, 6.582e-03), "input_blocks.11": (1.919e-06, 6.783e-03),
        "middle_block": (2.218e-06, 8.043e-03), "output_blocks.0": (2.119e-06, 7.027e-03), "output_blocks.1": (2.093e-06, 7.766e-03),
        "output_blocks.2": (2.160e-06, 8.547e-03), "output_blocks.3": (2.202e-06, 8.015e-03), "output_blocks.4": (2.213e-06, 7.860e-03),
        "output_blocks.5": (2.366e-06, 8.053e-03), "output_blocks.6": (2.321e-06, 7.488e-03), "output_blocks.7": (2.168e-06, 7.783e-03),
        "output_blocks.8": (2.279e-06, 8.163e-03), "output_blocks.9": (2.267e-06, 8.237e-03), "output_blocks.10": (2.206e-06, 8.570e-03),
        "output_blocks.11": (2.124e-06, 8.607e-03), "eps": (3.476e-06, 7.783e-03),
    },
    "B": {
        "input_blocks.0": (4.333e-08, 2.025e-03), "input_blocks.1": (4.892e-07, 4.643e-03), "input_blocks.2": (7.841e-07, 5.867e-03),
        "input_blocks.3": (8.398e-07, 4.585e-03), "input_blocks.4": (1.181e-06, 5.867e-03), "input_blocks.5": (1.393e-06, 7.043e-03),
        "input_blocks.6": (1.409e-06, 6.376e-03), "input_blocks.7": (1.631e-06, 6.395e-03), "input_blocks.8": (1.783e-06, 7.133e-03),
        "input_blocks.9": (1.842e-06, 7.080e-03), "input_blocks.10": (1.896e-06, 6.899e-03), "input_blocks.11": (1.958e-06, 7.032e-03),
        "middle_block": (2.193e-06, 7.387e-03), "output_blocks.0": (2.121e-06, 6.772e-03), "output_blocks.1": (2.138e-06, 6.977e-03),
        "output_blocks.2": (2.130e-06, 7.597e-03), "output_blocks.3": (2.156e-06, 7.549e-03), "output_blocks.4": (2.203e-06, 9.197e-03),
        "output_blocks.5": (2.319e-06, 8.146e-03), "output_blocks.6": (2.299e-06, 7.969e-03), "output_blocks.7": (2.220e-06, 7.749e-03),
        "output_blocks.8": (2.285e-06, 8.504e-03), "output_blocks.9": (2.306e-06, 7.821e-03), "output_blocks.10": (2.273e-06, 8.179e-03),
        "output_blocks.11": (2.196e-06, 8.977e-03), "eps": (3.521e-06, 8.657e-03),
    },
    "C": {
        "input_blocks.0": (4.320e-08, 2.187e-03), "input_blocks.1": (2.092e-07, 3.511e-03), "input_blocks.2": (3.602e-07, 4.276e-03),
        "input_blocks.3": (4.101e-07, 3.672e-03), "input_blocks.4": (8.977e-07, 5.028e-03), "input_blocks.5": (1.198e-06, 5.517e-03),
        "input_blocks.6": (1.251e-06, 5.091e-03), "input_blocks.7": (1.519e-06, 5.655e-03), "input_blocks.8": (1.791e-06, 7.445e-03),
        "input_blocks.9": (1.887e-06, 6.433e-03), "input_blocks.10": (2.355e-06, 7.651e-03), "input_blocks.11": (2.661e-06, 7.832e-03),
        "middle_block": (3.000e-06, 8.075e-03), "output_blocks.0": (3.029e-06, 7.459e-03), "output_blocks.1": (3.150e-06, 8.330e-03),
        "output_blocks.2": (3.170e-06, 8.579e-03), "output_blocks.3": (3.126e-06, 9.220e-03), "output_blocks.4": (2.841e-06, 7.891e-03),
        "output_blocks.5": (2.632e-06, 8.851e-03), "output_blocks.6": (2.545e-06, 7.751e-03), "output_blocks.7": (2.417e-06, 7.802e-03),
        "output_blocks.8": (2.739e-06, 8.282e-03), "output_blocks.9": (2.518e-06, 8.987e-03), "output_blocks.10": (2.202e-06, 8.383e-03),
        "output_blocks.11": (1.989e-06, 7.949e-03), "eps": (2.692e-06, 6.681e-03),
    },
    "D": {
        "input_blocks.0": (4.312e-08, 1.997e-03), "input_blocks.1": (5.020e-07, 4.685e-03), "input_blocks.2": (8.532e-07, 5.109e-03),
        "input_blocks.3": (9.228e-07, 4.358e-03), "input_blocks.4": (1.259e-06, 5.676e-03), "input_blocks.5": (1.534e-06, 5.885e-03),
        "input_blocks.6": (1.590e-06, 5.361e-03), "input_blocks.7": (1.970e-06, 6.437e-03), "input_blocks.8": (2.237e-06, 7.799e-03),
        "input_blocks.9": (2.330e-06, 8.630e-03), "input_blocks.10": (2.387e-06, 9.014e-03), "input_blocks.11": (2.449e-06, 8.843e-03),
        "middle_block": (2.824e-06, 7.659e-03), "output_blocks.0": (2.849e-06, 7.705e-03), "output_blocks.1": (2.591e-06, 6.927e-03),
        "output_blocks.2": (2.556e-06, 7.817e-03), "output_blocks.3": (2.793e-06, 8.111e-03), "output_blocks.4": (2.676e-06, 7.104e-03),
        "output_blocks.5": (2.878e-06, 8.549e-03), "output_blocks.6": (2.699e-06, 8.343e-03), "output_blocks.7": (2.468e-06, 7.242e-03),
        "output_blocks.8": (2.540e-06, 7.857e-03), "output_blocks.9": (2.519e-06, 7.544e-03), "output_blocks.10": (2.504e-06, 8.082e-03),
        "output_blocks.11": (2.576e-06, 7.987e-03), "eps": (3.757e-06, 7.072e-03),
    },
    "S": {
        "input_blocks.0": (4.313e-08, 2.084e-03), "input_blocks.1": (5.037e-07, 4.385e-03), "input_blocks.2": (8.165e-07, 5.349e-03),
        "input_blocks.3": (8.818e-07, 4.445e-03), "input_blocks.4": (1.221e-06, 5.669e-03), "input_blocks.5": (1.445e-06, 6.130e-03),
        "input_blocks.6": (1.450e-06, 6.945e-03), "input_blocks.7": (1.800e-06, 5.854e-03), "input_blocks.8": (1.998e-06, 7.464e-03),
        "input_blocks.9": (2.024e-06, 6.102e-03), "input_blocks.10": (2.070e-06, 6.062e-03), "input_blocks.11": (2.090e-06, 6.680e-03),
        "middle_block": (2.433e-06, 6.934e-03), "output_blocks.0": (2.336e-06, 6.900e-03), "output_blocks.1": (2.322e-06, 7.222e-03),
        "output_blocks.2": (2.239e-06, 8.034e-03), "output_blocks.3": (2.445e-06, 7.394e-03), "output_blocks.4": (2.504e-06, 7.000e-03),
        "output_blocks.5": (2.572e-06, 7.747e-03), "output_blocks.6": (2.580e-06, 8.014e-03), "output_blocks.7": (2.400e-06, 7.786e-03),
        "output_blocks.8": (2.414e-06, 7.732e-03), "output_blocks.9": (2.359e-06, 8.139e-03), "output_blocks.10": (2.352e-06, 7.459e-03),
        "output_blocks.11": (2.281e-06, 7.269e-03), "eps": (3.952e-06, 7.955e-03),
    },
}
E_VAE = {
    "bbox": {"decode": (1.769e-06, 7.695e-03), "moments": (2.344e-06, 7.301e-03)},
    "upscale": {"decode": (1.360e-06, 4.211e-03), "moments": (1.629e-06, 4.623e-03)},
}
