"""upk_q_sample_keyed_f32 (upgpt_amd/csrc/loss.hip, include/upk.h) and the keyed loss surface on a real MI355X.

The kernel is pinned bit for bit by the two-launch composition it replaces: upk_randn_keyed_f32 (rows = 1, row0 = 0,
stream_id = STREAM_LOSS_NOISE) for the noise, the host's (w0 * n_t) >> 32 (tests/val_ref.py) for the timesteps and
upk_q_sample_f32 for x_noisy / xin.  Every comparison is exact; the only tolerance involved is the 1e-5 of the normals
against fp64, inherited through that bit-equality (tests/test_rng_gpu.py) and not restated."""
import os

import numpy as np
import pytest
import torch

import rng_ref
import val_ref
import upgpt_amd
from upgpt_amd import _lib, rng, synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
N_T, LD, SENTINEL = 1000, 32, 7.5
# (batch, c, hw, every pointer offset by 4 bytes)
CASES = [(1, 4, 1, False), (3, 4, 35, True), (2, 4, 768, False), (5, 3, 4099, False)]
_cache = {}


def tables():
    if "t" not in _cache:
        g = np.load(os.path.join(G, "loss.npz"))
        _cache["t"] = (torch.from_numpy(g["sqrt_alphas_cumprod"]), torch.from_numpy(g["sqrt_one_minus_alphas_cumprod"]))
    return _cache["t"]


def get_model():
    if "m" not in _cache:
        m = upgpt_amd.build_model("tiny")
        synth.fill_module_(m)
        synth.fill_ema_(m, salt=1)
        _cache["m"] = m.cuda()
    return _cache["m"]


def dev(t, off=False):
    """A device copy of the host tensor `t`; off: at a 4-byte offset from an allocation (16-byte aligned by torch)."""
    if not off:
        return t.cuda()
    k = 4 // t.element_size()
    buf = torch.zeros(t.numel() + k, dtype=t.dtype, device="cuda")
    buf[k:].copy_(t.reshape(-1))
    assert buf[k:].data_ptr() % 16 == 4
    return buf[k:].view(t.shape)


def bits(x):
    x = x.contiguous().cpu()
    return x.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[x.element_size()])


def x_of(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(200 + seed))


def run_keyed(ctx, hkeys, draw, x0, t_in=None, off=False, want=("noise", "xn", "xin")):
    """-> (t_out, noise_out, x_noisy, xin) as host tensors (None for an output that was not asked for)."""
    B, C, HW = x0.shape
    a, s = tables()
    keys = dev(torch.from_numpy(hkeys.view(np.int32).copy()), off)
    t_out = dev(torch.full((B,), -7, dtype=torch.int32), off)
    nz = dev(torch.full(x0.shape, float("inf")), off) if "noise" in want else None
    xn = dev(torch.full(x0.shape, float("inf")), off) if "xn" in want else None
    xin = dev(torch.full((B * HW, LD), SENTINEL, dtype=torch.float16), off) if "xin" in want else None
    ctx.q_sample_keyed(keys, draw, dev(x0, off), None if t_in is None else dev(t_in, off), dev(a, off), dev(s, off), N_T, t_out,
                       nz, xn, xin, LD, B, C, HW)
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu() for v in (t_out, nz, xn, xin))


def run_two_launches(ctx, hkeys, draw, x0, t):
    """The composition the kernel replaces, all pointers aligned."""
    B, C, HW = x0.shape
    a, s = tables()
    keys = torch.from_numpy(hkeys.view(np.int32).copy()).cuda()
    nz = torch.empty(x0.shape, device="cuda")
    ctx.randn_keyed(keys, B, C * HW, 0, 1, rng.STREAM_LOSS_NOISE, draw, None, nz)
    xn = torch.empty(x0.shape, device="cuda")
    xin = torch.full((B * HW, LD), SENTINEL, dtype=torch.float16, device="cuda")
    ctx.q_sample(x0.cuda(), nz, t.cuda(), a.cuda(), s.cuda(), N_T, xn, xin, LD, B, C, HW)
    torch.cuda.synchronize()
    return nz.cpu(), xn.cpu(), xin.cpu()


@pytest.mark.parametrize("B, C, HW, off", CASES)
def test_kernel_equals_the_two_launches(ctx, B, C, HW, off):
    hkeys = rng_ref.keys_of(7, range(10, 10 + B))
    x0 = x_of((B, C, HW), B)
    for draw in (0, 1):
        t_want = torch.from_numpy(val_ref.timesteps(hkeys, N_T, draw)).to(torch.int32)
        nz_w, xn_w, xin_w = run_two_launches(ctx, hkeys, draw, x0, t_want)
        t_out, nz, xn, xin = run_keyed(ctx, hkeys, draw, x0, off=off)
        assert t_out.tolist() == t_want.tolist()
        assert torch.equal(bits(nz), bits(nz_w)) and torch.equal(bits(xn), bits(xn_w))
        assert torch.equal(bits(xin), bits(xin_w)) and bool((xin[:, C:] == SENTINEL).all())
    # each output may be NULL, and the others do not change
    for want in (("noise",), ("xn",), ("xin",), ("noise", "xin")):
        got = dict(zip(("t", "noise", "xn", "xin"), run_keyed(ctx, hkeys, 1, x0, off=off, want=want)))
        assert got["t"].tolist() == t_want.tolist()
        for name, ref in (("noise", nz_w), ("xn", xn_w), ("xin", xin_w)):
            assert (got[name] is None) == (name not in want)
            assert got[name] is None or torch.equal(bits(got[name]), bits(ref))


def test_a_value_depends_on_the_key_alone(ctx):
    """Sample 3 of a batch of 5 has the bits of the same key alone in a batch of 1 (c * hw odd: another alignment too)."""
    B, C, HW = 5, 3, 4099
    hkeys = rng_ref.keys_of(7, range(10, 10 + B))
    x0 = x_of((B, C, HW), B)
    t5, nz5, xn5, xin5 = run_keyed(ctx, hkeys, 0, x0)
    for off in (False, True):
        t1, nz1, xn1, xin1 = run_keyed(ctx, hkeys[3:4], 0, x0[3:4], off=off)
        assert int(t1[0]) == int(t5[3])
        assert torch.equal(bits(nz1[0]), bits(nz5[3])) and torch.equal(bits(xn1[0]), bits(xn5[3]))
        assert torch.equal(bits(xin1), bits(xin5[3 * HW:4 * HW]))
    assert not torch.equal(bits(nz5[3]), bits(nz5[2]))


def test_t_in_is_honoured(ctx):
    B, C, HW = 3, 4, 35
    hkeys = rng_ref.keys_of(7, range(B))
    x0 = x_of((B, C, HW), 0)
    t_in = torch.tensor([N_T - 1, 0, 417], dtype=torch.int32)
    nz_w, xn_w, xin_w = run_two_launches(ctx, hkeys, 2, x0, t_in)
    t_out, nz, xn, xin = run_keyed(ctx, hkeys, 2, x0, t_in=t_in)
    assert t_out.tolist() == t_in.tolist() and t_out.tolist() != val_ref.timesteps(hkeys, N_T, 2).tolist()
    assert torch.equal(bits(nz), bits(nz_w)) and torch.equal(bits(xn), bits(xn_w)) and torch.equal(bits(xin), bits(xin_w))
    # a timestep outside the tables is never used as an index: that sample's x_noisy / xin are NaN, the rest as without it
    bad = torch.tensor([N_T - 1, N_T, 417], dtype=torch.int32)
    t_out, nz, xn, xin = run_keyed(ctx, hkeys, 2, x0, t_in=bad)
    assert t_out.tolist() == bad.tolist() and torch.equal(bits(nz), bits(nz_w))
    assert bool(torch.isnan(xn[1]).all()) and torch.equal(bits(xn[0]), bits(xn_w[0])) and torch.equal(bits(xn[2]), bits(xn_w[2]))
    xin = xin.reshape(B, HW, LD)
    assert bool(torch.isnan(xin[1, :, :C]).all()) and bool((xin[:, :, C:] == SENTINEL).all())


def test_error_codes(ctx):
    a, s = (v.cuda() for v in tables())
    x0 = x_of((1, 4, 15), 0).cuda()
    keys = torch.from_numpy(rng_ref.keys_of(1, [0]).view(np.int32).copy()).cuda()
    t_out = torch.empty(1, dtype=torch.int32, device="cuda")
    nz, xn = torch.empty_like(x0), torch.empty_like(x0)
    xin = torch.empty(15, LD, dtype=torch.float16, device="cuda")
    good = dict(keys=keys, draw=0, x_start=x0, t_in=None, sqrt_ac=a, sqrt_1m_ac=s, n_t=N_T, t_out=t_out, noise_out=nz,
                x_noisy=xn, xin=xin, ld_xin=LD, batch=1, c=4, hw=15)
    ctx.q_sample_keyed(**good)
    cases = [(dict(keys=None), -1), (dict(x_start=None), -1), (dict(sqrt_ac=None), -1), (dict(sqrt_1m_ac=None), -1),
             (dict(t_out=None), -1), (dict(noise_out=None, x_noisy=None, xin=None), -1), (dict(batch=0), -1), (dict(c=0), -1),
             (dict(hw=-1), -1), (dict(n_t=0), -1), (dict(ld_xin=3), -1), (dict(x_start=x0.data_ptr() + 2), -1),
             (dict(keys=keys.data_ptr() + 2), -1), (dict(t_in=t_out.data_ptr() + 1), -1), (dict(noise_out=nz.data_ptr() + 2), -1),
             (dict(xin=xin.data_ptr() + 1), -1),
             (dict(c=1 << 16, hw=1 << 15, xin=None), -2)]  # c * hw does not fit
    for override, code in cases:
        with pytest.raises(_lib.UpkError) as ei:
            ctx.q_sample_keyed(**dict(good, **override))
        assert ei.value.code == code, (override, ei.value)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- validation_step(noise_keys=)
def a15_batch(B):
    """The DeepFashion-shaped batch of tests/test_loss_gpu.py, with the loader's loss_w."""
    g0 = torch.Generator().manual_seed(3)
    w = torch.ones(B, 1, 32, 24)
    w[:, :, 0:8], w[:, :, 20:32] = 2.0, 0.5
    return {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
            "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
            "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24), "loss_w": w}


KEYS = ["val/loss_simple", "val/loss_vlb", "val/loss", "val/loss_simple_ema", "val/loss_vlb_ema", "val/loss_ema"]


def test_validation_step_keyed(monkeypatch):
    m = get_model()
    unet = m.model.diffusion_model
    batch = {k: v.cuda() for k, v in a15_batch(2).items()}
    keys = rng.NoiseKeys(7, [0, 1], device="cuda")
    keys.keys
    torch.manual_seed(21)
    d1 = m.validation_step(batch, 0, noise_keys=keys)
    assert list(d1) == KEYS + [m.PER_SAMPLE]
    rows1 = d1[m.PER_SAMPLE].cpu()
    v1 = [float(d1[k]) for k in KEYS]
    print("keyed validation_step:", dict(zip(KEYS, v1)), rows1.tolist())
    assert rows1.shape == (2, 6) and rows1.dtype == torch.float64
    assert bool(torch.isfinite(rows1).all()) and all(np.isfinite(v1))  # twelve per-sample values, six means
    assert all(a != b for a, b in zip(v1[:3], v1[3:]))  # (the EMA weights are another recipe draw)
    assert not torch.equal(rows1[:, 1], rows1[:, 4])
    # the timesteps are the host's: draw 0 for the live pass, draw 1 for the EMA pass
    assert rows1[:, 0].tolist() == [769.0, 419.0] and rows1[:, 3].tolist() == [902.0, 661.0]
    assert m.loss_t.tolist() == [902, 661] and m.loss_terms.shape == (8,)
    assert unet._weight_override is None and unet._weight_selection() is None
    # the same bits on a second call, and after another torch seed; the torch generator's state is untouched
    before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    entries = []
    real = _lib.pools_in_flight  # (host_io() asks it once per entry when the thread's concurrency is 1)
    monkeypatch.setattr(_lib, "pools_in_flight", lambda: (entries.append(1), real())[1])
    d2 = m.validation_step(batch, 0, noise_keys=keys)
    monkeypatch.undo()
    assert entries == [], "a warm keyed validation_step entered host_io() %d times" % len(entries)
    torch.manual_seed(99)
    before2 = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    d3 = m.validation_step(batch, 0, noise_keys=keys)
    for d in (d2, d3):
        assert [float(d[k]) for k in KEYS] == v1 and torch.equal(bits(d[m.PER_SAMPLE]), bits(rows1))
    assert torch.equal(before2[0], torch.get_rng_state()) and torch.equal(before2[1], torch.cuda.get_rng_state())
    assert not torch.equal(before[0], before2[0])
    # another key, other draws; the per-sample values of a key do not depend on its neighbour in the batch being there
    other = m.validation_step(batch, 0, noise_keys=rng.NoiseKeys(8, [0, 1], device="cuda"))[m.PER_SAMPLE].cpu()
    assert other[:, 0].tolist() != rows1[:, 0].tolist() and not torch.equal(other[:, 1], rows1[:, 1])


def test_keyed_p_losses_matches_the_unkeyed_path_on_the_same_draws():
    """forward(noise_keys=) = p_losses(t = the host's timesteps, noise = upk_randn_keyed_f32's table): the same bits."""
    m = get_model()
    torch.manual_seed(5)
    inp = synth.synth_inputs(2, (32, 24), 4, 87, 768, seed=11, steps=1)
    x0 = (0.18215 * 4.0 * inp["x_T"]).cuda()
    cond = {"c_crossattn": inp["c_crossattn"].cuda(), "c_concat": [inp["c_concat"].cuda()]}
    keys = rng.NoiseKeys(7, [0, 1], device="cuda").fork(1)
    loss_k, dk = m(x0, cond, noise_keys=keys)
    terms_k = m.loss_terms.clone()
    assert m.loss_t.tolist() == [902, 661]
    noise = rng.randn(keys, tuple(x0.shape), rng.STREAM_LOSS_NOISE)
    loss_u, du = m.p_losses(x0, cond, torch.tensor([902, 661], device="cuda"), noise=noise)
    assert torch.equal(bits(terms_k), bits(m.loss_terms)) and float(loss_k) == float(loss_u) and list(dk) == list(du)
    # a given t is honoured with keys
    m.p_losses(x0, cond, torch.tensor([3, 981], device="cuda"), noise_keys=keys)
    assert m.loss_t.tolist() == [3, 981]
    with pytest.raises(ValueError, match="both name the noise"):
        m.p_losses(x0, cond, None, noise=noise, noise_keys=keys)


def test_without_keys_the_generator_path_is_what_it_was():
    m = get_model()
    batch = {k: v.cuda() for k, v in a15_batch(2).items()}
    torch.manual_seed(21)
    d1 = m.validation_step(batch, 0)
    torch.manual_seed(21)
    d2 = m.validation_step(batch, 0)
    torch.manual_seed(22)
    d3 = m.validation_step(batch, 0)
    assert list(d1) == KEYS == list(d2)
    assert [float(d1[k]) for k in KEYS] == [float(d2[k]) for k in KEYS] != [float(d3[k]) for k in KEYS]
