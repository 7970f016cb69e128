"""Every UNet block and every batch position against the fp64 oracle (tests/block_ref.py: two measures per tap and per
sample, bound 4 x what fp16 storage costs the oracle itself), for each lowering the engine can give a block: the default,
every fusion off, every fusion forced, and the shared-chip table; the batch rotated; sampler-mode row addressing; each
run twice, bit for bit.  The VAE's decode and encoder moments per sample by the same rule.

What the module-scoped state costs: the fp64 oracle of case A about 7 s of CPU, B 3 s, C 2 s, D and S under 1 s, and a
model built and filled once per kind (bbox 7 s); the first test that asks pays.  After that a test is one plan build and two
forwards (under 0.1 s)."""
import collections
import contextlib

import pytest
import torch

import block_ref as R
import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import knobs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED = ("xblock ", "hblock ", "mlp ", "attn+q ")
LOWERINGS = {
    "default": dict(knobs={}, lanes=1),
    "off": dict(knobs=dict(UPS_PHASES=False, LN_ROWS=False, QPROJ_FUSE=False, GN_REDUCE_APPLY=False, MLP_FUSE="0",
                           XBLOCK="0", HBLOCK="0", WEIGHT_PREFETCH="0"), lanes=1),
    "forced": dict(knobs=dict(MLP_FUSE="1", XBLOCK="1", HBLOCK="1"), lanes=1),
    "shared_chip4": dict(knobs={}, lanes=4),
}
_models = {}
_labels = {}  # (case, lowering) -> Counter of the body's labels


def get_model(kind):
    if kind not in _models:
        m = upgpt_amd.build_model(kind, overrides=R.overrides(kind))
        R.state(kind, m)  # (recipe weights into the model; the oracle reads the same tensors)
        _models[kind] = m.cuda()
    return _models[kind]


@contextlib.contextmanager
def lowering(unet, name):
    """The knobs of one lowering on a UNet whose packed weights and plans are its own: the plan-cache key does not hold
    the knobs and packed weights may depend on them, so both are dropped on the way in and on the way out."""
    lw = LOWERINGS[name]
    old = {k: getattr(knobs, k) for k in lw["knobs"]}
    if old:
        unet.invalidate()
    try:
        for k, v in lw["knobs"].items():
            setattr(knobs, k, v)
        with L.shared_chip(lw["lanes"]) if lw["lanes"] > 1 else contextlib.nullcontext():
            yield
    finally:
        for k, v in old.items():
            setattr(knobs, k, v)
        if old:
            unet.invalidate()


def snapshot(plan):
    torch.cuda.synchronize()
    return {n: v.detach().cpu().clone() for n, v in R.taps_nchw(plan).items()}


def forward_taps(model, name, rot=0):
    """Two forwards of a forward-mode case through LatentDiffusion.apply_model; -> (taps of both, the plan)."""
    c, i = R.CASES[name], R.case_inputs(name)
    roll = lambda v: v.roll(rot, 0).to(DEV)
    cond = {"c_crossattn": roll(i["ctx"]), "c_concat": [roll(i["cc"])]}
    unet = model.model.diffusion_model
    runs = []
    for _ in range(2):
        eps = model.apply_model(roll(i["x"]), roll(i["t"]), cond)
        pl = unet.plan(c["B"], c["H"], c["W"], c["ntok"], c["B"], "forward")
        runs.append(snapshot(pl))
        assert torch.equal(eps.cpu(), runs[-1]["eps"])
    return runs, pl


def sampler_taps(model, name):
    """Case S: the sampler-mode plan driven as a sampler's fast path drives it, the step counter at each of the case's
    steps; the taps of the steps stacked along the batch as block_ref.oracle_batch stacks the reference."""
    c, i = R.CASES[name], R.case_inputs(name)
    unet = model.model.diffusion_model
    pl = unet.plan(c["B"], c["H"], c["W"], c["ntok"], len(c["t_rows"]), "sampler")
    assert pl.mode == "sampler" and pl.rows == len(c["t_rows"])
    runs = []
    for _ in range(2):
        with torch.cuda.device(pl.dev):
            pl.load_sampler_inputs(i["x"].to(DEV), i["cc"].to(DEV), i["ctx"].to(DEV), unet.in_channels, ("block_ref", name),
                                   torch.tensor(c["t_rows"], dtype=torch.float32))
            pl.prep.run()
            per_step = []
            for s in c["steps"]:
                pl.step.fill_(s)
                pl.body.run()
                per_step.append(snapshot(pl))
        runs.append({n: torch.cat([p[n] for p in per_step]) for n in per_step[0]})
    return runs, pl


def label_census(pl):
    labs = collections.Counter(lab for lab in pl.body.labels if lab)
    fused = {f.strip(): sum(n for lab, n in labs.items() if lab.startswith(f)) for f in FUSED}
    return labs, fused


def run_case(name, low, rot=0):
    model = get_model(R.CASES[name]["kind"])
    with lowering(model.model.diffusion_model, low):
        (a, b), pl = (sampler_taps(model, name) if name == "S" else forward_taps(model, name, rot))
        labs, fused = label_census(pl)
    print("\ncase %s, %s: %d launches in the body, fused %s" % (name, low, len(pl.body.labels), fused))
    for n in a:
        assert torch.equal(a[n], b[n]), "case %s %s: %s differs between two runs" % (name, low, n)
    ref = R.oracle_ref(name)
    if rot:
        ref = {n: v.roll(rot, 0) for n, v in ref.items()}
    assert set(a) == set(ref)
    R.check("case %s, %s%s: ratios to %g x E" % (name, low, ", batch rotated by %d" % rot if rot else "", R.MARGIN), a, ref,
            R.E[name])
    return labs, fused


@pytest.mark.parametrize("low", list(LOWERINGS))
def test_case_a_bench_shape(low):
    """bbox UNet, B = 8, 32x32: the four lowerings, each proven from the plan's labels."""
    labs, fused = run_case("A", low)
    _labels[low] = labs
    if low == "off":
        assert not any(fused.values()), fused
    else:  # ("auto" takes the fused head, cross and feed-forward kernels at this shape; "1" takes no fewer)
        assert fused["hblock"] > 0 and fused["xblock"] > 0 and fused["mlp"] > 0, fused


def test_case_a_lowerings_differ():
    """The four lowerings of case A launched pairwise different multisets of labels (they ran above, or run here)."""
    for low in LOWERINGS:
        if low not in _labels:
            _labels[low] = run_case("A", low)[0]
    names = list(LOWERINGS)
    for i, u in enumerate(names):
        print("%-13s %3d launches, %3d distinct labels" % (u, sum(_labels[u].values()), len(_labels[u])))
        for v in names[i + 1:]:
            assert _labels[u] != _labels[v], (u, v)
    count = lambda low: sum(n for lab, n in _labels[low].items() if lab.startswith(FUSED[:3]))
    assert count("forced") > count("default") > count("off") == 0, [count(low) for low in names]


def test_case_a_batch_rotated_by_3():
    """Sample k at position (k + 3) mod 8, the default lowering, the rotated reference: nothing in the plan may depend on
    where in the batch a sample sits."""
    run_case("A", "default", rot=3)


@pytest.mark.parametrize("low", ["default", "shared_chip4"])
def test_case_b_padded_key_counts(low):
    """bbox UNet, B = 8, 32x24: 192, 48 and 12 tokens at the lower levels (V^T rows padded to 64 and 32 keys)."""
    labs, _ = run_case("B", low)
    for nq in (768, 192, 48, 12):
        assert any(lab.startswith("attn ") and " nq%d nkv%d " % (nq, nq) in lab for lab in labs), (nq, sorted(labs))


def test_case_c_upscale_unet():
    """upscale UNet (6 input channels, 3-channel concat, 86 context tokens), B = 4, 32x24."""
    labs, _ = run_case("C", "default")
    assert any(lab.startswith("attn B4 ") and " nq192 nkv192 " in lab for lab in labs), sorted(labs)  # (attention from 16x12 down)


def test_case_d_tiny_unet_generic_path():
    """tiny UNet, B = 3, 32x24: head widths 12 / 24 / 48 and 3-channel groups take no fused row-chain kernel."""
    _, fused = run_case("D", "default")
    assert fused["xblock"] == 0 and fused["hblock"] == 0 and fused["mlp"] == 0, fused


def test_case_s_sampler_rows():
    """Sampler mode: steps 0 and 2 of t_rows = (981, 500, 21), the reference at t_rows[step] for both samples."""
    run_case("S", "default")


# ---------------------------------------------------------------------------------------------------------------------
# the VAE, whole output per sample
@pytest.mark.parametrize("byproduct", ["0", "1"])
@pytest.mark.parametrize("kind", ["bbox", "upscale"])
def test_vae_decode_and_moments_per_sample(kind, byproduct):
    model = get_model(kind)
    fs = model.first_stage_model
    assert abs(float(model.scale_factor) - R.SCALE_FACTOR) < 1e-7
    i = R.vae_inputs(kind)

    def reset():  # (the plans read the knob when they are built and are not keyed by it)
        fs._plans.drop(device=DEV)
        fs._enc_plans.drop(device=DEV)

    def census():  # (launch count, labels) of the decode and encode plans as the knob stands
        h, w = R.VAE_LATENT
        plans = (fs._decode_plan(R.VAE_B, h, w, float(model.scale_factor)), fs._encode_plan(R.VAE_B, *i["img"].shape[2:]))
        return [(pl.prog.n_launch, collections.Counter(lab for lab in pl.prog.labels if lab)) for pl in plans]

    old = knobs.VAE_GN_BYPRODUCT
    reset()
    try:
        knobs.VAE_GN_BYPRODUCT = {"0": "1", "1": "0"}[byproduct]
        other = census()
        reset()
        knobs.VAE_GN_BYPRODUCT = byproduct
        runs = []
        for _ in range(2):
            img = model.decode_first_stage(i["z"].to(DEV))
            mom = model.encode_first_stage(i["img"].to(DEV)).parameters
            torch.cuda.synchronize()
            runs.append({"decode": img.cpu(), "moments": mom.cpu()})
        mine = census()
    finally:
        knobs.VAE_GN_BYPRODUCT = old
        reset()
    print("\nVAE %s by-product %s: %d + %d launches (the other setting: %d + %d)" % (
        kind, byproduct, mine[0][0], mine[1][0], other[0][0], other[1][0]))
    assert mine[0] != other[0] and mine[1] != other[1]  # (the knob changed what both halves launch)
    a, b = runs
    for n in a:
        assert torch.equal(a[n], b[n]), n
    f = R.vae_factor(kind)
    assert a["decode"].shape == (R.VAE_B, 3, R.VAE_LATENT[0] * f, R.VAE_LATENT[1] * f)
    R.check("VAE %s, GroupNorm by-product %s: ratios to %g x E" % (kind, byproduct, R.MARGIN), a, R.vae_ref(kind),
            R.E_VAE[kind])
