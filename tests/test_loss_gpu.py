"""The validation loss on the MI355X: upk_q_sample_f32 against torch's fp32 expression on the CPU (bit for bit),
upk_p_losses_f32 against tests/loss_ref.py in fp64, LatentDiffusion.p_losses against the reference's own run
(tests/golden/loss.npz, made by tests/golden/make_loss_golden.py), validation_step and evaluate.run_validation."""
import json
import os

import numpy as np
import pytest
import torch

import loss_ref as lr
import upgpt_amd
from upgpt_amd import _lib, evaluate, synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
N_T = 1000
EPS = 4 * 2.0 ** -24  # three roundings per non-negative fp32 term, one at the output
SHAPES = [(1, 4, 5, 3), (3, 4, 32, 24), (2, 3, 128, 96)]
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(G, "loss.npz")))
    return _cache["g"]


def tables():
    g = golden()
    return torch.from_numpy(g["sqrt_alphas_cumprod"]), torch.from_numpy(g["sqrt_one_minus_alphas_cumprod"])


def get_model():
    if "m" not in _cache:
        m = upgpt_amd.build_model("tiny")
        synth.fill_module_(m)
        synth.fill_ema_(m, salt=1)
        _cache["m"] = m.cuda()
    return _cache["m"]


def timesteps(B):
    return torch.tensor([N_T - 1, 0, 417, 3, 981][:B], dtype=torch.int32)


def qs_inputs(shape, seed=0):
    gen = torch.Generator().manual_seed(100 + seed)
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)


def qs_torch(x0, noise, t):
    """The reference's expression (ddpm.py:271-274) in fp32 on the CPU."""
    a, s = tables()
    t = t.long()
    return a[t].reshape(-1, 1, 1, 1) * x0 + s[t].reshape(-1, 1, 1, 1) * noise


def run_q_sample(ctx, x0, noise, t, want_xn=True, want_xin=True, ld=32, sentinel=7.5):
    a, s = tables()
    B, C, H, W = x0.shape
    xn = torch.full(x0.shape, float("inf"), device="cuda") if want_xn else None
    xin = torch.full((B * H * W, ld), sentinel, dtype=torch.float16, device="cuda") if want_xin else None
    ctx.q_sample(x0.cuda(), noise.cuda(), t.cuda(), a.cuda(), s.cuda(), N_T, xn, xin, ld, B, C, H * W)
    torch.cuda.synchronize()
    return (None if xn is None else xn.cpu()), (None if xin is None else xin.cpu())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nhwc_half(x, C):
    B = x.shape[0]
    return x.half().permute(0, 2, 3, 1).reshape(-1, C)


# ---------------------------------------------------------------- upk_q_sample_f32
@pytest.mark.parametrize("shape", SHAPES)
def test_q_sample_bit_equal_to_torch(ctx, shape):
    B, C = shape[:2]
    x0, noise = qs_inputs(shape)
    ts = [timesteps(B)] + ([torch.tensor([0], dtype=torch.int32)] if B == 1 else [])
    for t in ts:
        want = qs_torch(x0, noise, t)
        xn, xin = run_q_sample(ctx, x0, noise, t)
        assert same_bits(xn, want)
        assert torch.equal(xin[:, :C].view(torch.int16), nhwc_half(want, C).view(torch.int16))
        assert bool((xin[:, C:] == 7.5).all())  # (the other channels of a row are left untouched)
        xn2, none = run_q_sample(ctx, x0, noise, t, want_xin=False)
        assert none is None and same_bits(xn2, want)
        none, xin2 = run_q_sample(ctx, x0, noise, t, want_xn=False)
        assert none is None and torch.equal(xin2.view(torch.int16), xin.view(torch.int16))


def test_q_sample_without_16_byte_alignment(ctx):
    """Pointers that are only 4-byte aligned: every element goes alone, the same bits."""
    shape = (3, 4, 32, 24)
    x0, noise = qs_inputs(shape, 1)
    t = timesteps(3)
    a, s = tables()
    n = x0.numel()
    bx, bn, bo = (torch.zeros(n + 1, device="cuda") for _ in range(3))
    bx[1:].copy_(x0.reshape(-1))
    bn[1:].copy_(noise.reshape(-1))
    assert bx[1:].data_ptr() % 16 == 4
    ctx.q_sample(bx[1:], bn[1:], t.cuda(), a.cuda(), s.cuda(), N_T, bo[1:], None, 0, 3, 4, 32 * 24)
    torch.cuda.synchronize()
    assert same_bits(bo[1:].cpu().reshape(shape), qs_torch(x0, noise, t)) and float(bo[0]) == 0.0


@pytest.mark.parametrize("bad", [N_T, -1])
def test_q_sample_timestep_outside_the_tables(ctx, bad):
    shape = (3, 4, 32, 24)
    x0, noise = qs_inputs(shape, 2)
    t = torch.tensor([5, bad, 7], dtype=torch.int32)
    xn, xin = run_q_sample(ctx, x0, noise, t)
    ok = torch.tensor([5, 0, 7], dtype=torch.int32)
    want = qs_torch(x0, noise, ok)
    assert bool(torch.isnan(xn[1]).all()) and same_bits(xn[0], want[0]) and same_bits(xn[2], want[2])
    xin = xin.reshape(3, 32 * 24, 32)
    wh = nhwc_half(want, 4).reshape(3, 32 * 24, 4)
    assert bool(torch.isnan(xin[1, :, :4]).all()) and bool((xin[1, :, 4:] == 7.5).all())
    assert torch.equal(xin[0, :, :4], wh[0]) and torch.equal(xin[2, :, :4], wh[2])


def test_q_sample_error_codes(ctx):
    x0, noise = qs_inputs((1, 4, 5, 3))
    a, s = tables()
    x0, noise, a, s, t = x0.cuda(), noise.cuda(), a.cuda(), s.cuda(), timesteps(1).cuda()
    xn = torch.empty_like(x0)
    xin = torch.empty(15, 32, dtype=torch.float16, device="cuda")
    good = dict(x_start=x0, noise=noise, t=t, sqrt_ac=a, sqrt_1m_ac=s, n_t=N_T, x_noisy=xn, xin=xin, ld_xin=32, batch=1, c=4, hw=15)
    ctx.q_sample(**good)
    cases = [(dict(x_start=None), -1), (dict(noise=None), -1), (dict(t=None), -1), (dict(sqrt_ac=None), -1),
             (dict(sqrt_1m_ac=None), -1), (dict(x_noisy=None, xin=None), -1), (dict(batch=0), -1), (dict(c=0), -1),
             (dict(hw=-1), -1), (dict(n_t=0), -1), (dict(ld_xin=3), -1), (dict(x_start=x0.data_ptr() + 2), -1),
             (dict(xin=xin.data_ptr() + 1), -1),
             (dict(c=1 << 16, hw=1 << 15, x_noisy=xn, xin=None), -2),              # c * hw does not fit
             (dict(batch=1 << 20, c=1 << 10, hw=1 << 20, xin=None), -2)]           # 2^50 elements: too many workgroups
    for override, code in cases:
        with pytest.raises(_lib.UpkError) as ei:
            ctx.q_sample(**dict(good, **override))
        assert ei.value.code == code, (override, ei.value)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- upk_p_losses_f32
def pl_inputs(shape, wmode, seed=0):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(200 + seed)
    pred, target = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    w = None if wmode == 0 else 0.25 + 2.0 * torch.rand(B, 1 if wmode == 1 else C, H, W, generator=gen)
    logvar = 2.0 * torch.rand(N_T, generator=gen) - 1.0  # both signs
    for i, tb in enumerate(timesteps(B).tolist()):
        logvar[tb] = (-1.0) ** i * (0.3 + 0.1 * i)
    return pred, target, w, logvar


def run_p_losses(ctx, pred, target, w, t, logvar, loss_type, lsw=0.7, oew=0.3, override=None):
    B, C, H, W = pred.shape
    lvlb = torch.from_numpy(golden()["lvlb_weights"])
    nbytes = ctx.p_losses_ws_bytes(B, C, H * W)
    assert nbytes == B * ((C * H * W + 4095) // 4096) * 16
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((4 + 2 * B,), float("inf"), device="cuda")
    args = dict(model_out=pred.cuda(), target=target.cuda(), loss_w=None if w is None else w.cuda(),
                loss_w_channels=0 if w is None else w.shape[1], t=t.cuda(), logvar=logvar.cuda(), lvlb_weights=lvlb.cuda(),
                n_t=N_T, loss_type=_lib.LOSS_L1 if loss_type == "l1" else _lib.LOSS_L2, l_simple_weight=lsw,
                original_elbo_weight=oew, out=out, batch=B, c=C, hw=H * W, ws=ws, ws_bytes=nbytes)
    args.update(override or {})
    ctx.p_losses(**args)
    torch.cuda.synchronize()
    return out.cpu(), args


def check_p_losses(out, ref, B):
    got = out.double().numpy()
    simple, plain = got[4::2], got[5::2]
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    errs = {"simple": rel(simple, ref["simple"]), "plain": rel(plain, ref["plain"]),
            "loss_simple": rel(got[1], ref["loss_simple"]), "loss_vlb": rel(got[3], ref["loss_vlb"]),
            "loss_gamma": abs(got[2] - ref["loss_gamma"]) / ref["gamma_mag"], "loss": abs(got[0] - ref["loss"]) / ref["loss_mag"]}
    print("p_losses errors in units of 2^-24:", {k: "%.2f" % (v * 2.0 ** 24) for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= EPS, (k, v, EPS)


@pytest.mark.parametrize("wmode", [0, 1, 2], ids=["w_none", "w_1ch", "w_full"])
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("shape", SHAPES + [(5, 4, 8, 6)])
def test_p_losses_against_fp64(ctx, shape, loss_type, wmode):
    """simple, plain, loss_simple, loss_vlb: relative 4 * 2^-24 against loss_ref on the same fp32 inputs (non-negative terms
    of at most three fp32 roundings, one more rounding at the output); loss_gamma and loss, where logvar can cancel: 4 * 2^-24
    of the sum of the magnitudes of their terms.  Run twice: the same bits."""
    B = shape[0]
    pred, target, w, logvar = pl_inputs(shape, wmode)
    t = timesteps(B)
    out, _ = run_p_losses(ctx, pred, target, w, t, logvar, loss_type)
    ref = lr.p_losses(pred.numpy(), target.numpy(), t.numpy(), logvar.numpy(), golden()["lvlb_weights"],
                      None if w is None else w.numpy(), loss_type, np.float32(0.7), np.float32(0.3))
    assert bool(torch.isfinite(out).all())
    check_p_losses(out, ref, B)
    again, _ = run_p_losses(ctx, pred, target, w, t, logvar, loss_type)
    assert same_bits(out, again)


@pytest.mark.parametrize("shape", [(5, 4, 8, 6), (5, 3, 128, 96)])
def test_p_losses_sample_value_independent_of_batch(ctx, shape):
    """simple and plain of a sample: the same bits as sample 0 of a batch of 1 and as sample 4 of a batch of 5 (one
    workgroup per sample at 4 x 8 x 6, nine at 3 x 128 x 96)."""
    pred, target, w, logvar = pl_inputs(shape, 1, seed=3)
    t = timesteps(5)
    full, _ = run_p_losses(ctx, pred, target, w, t, logvar, "l2")
    one, _ = run_p_losses(ctx, pred[4:], target[4:], w[4:], t[4:], logvar, "l2")
    assert same_bits(full[4 + 2 * 4:], one[4:6])
    # and with loads of one element (pointers only 4-byte aligned)
    n = pred[4:].numel()
    bp, bt = torch.zeros(n + 1), torch.zeros(n + 1)
    bp[1:], bt[1:] = pred[4:].reshape(-1), target[4:].reshape(-1)
    bp, bt = bp.cuda(), bt.cuda()
    odd, _ = run_p_losses(ctx, pred[4:], target[4:], w[4:], t[4:], logvar, "l2", override=dict(model_out=bp[1:], target=bt[1:]))
    assert same_bits(odd, one)


@pytest.mark.parametrize("bad", [N_T, -1])
def test_p_losses_timestep_outside_the_tables(ctx, bad):
    shape = (3, 4, 32, 24)
    pred, target, w, logvar = pl_inputs(shape, 1, seed=4)
    good, _ = run_p_losses(ctx, pred, target, w, timesteps(3), logvar, "l2")
    out, _ = run_p_losses(ctx, pred, target, w, torch.tensor([N_T - 1, bad, 417], dtype=torch.int32), logvar, "l2")
    assert bool(torch.isnan(out[:4]).all()) and bool(torch.isnan(out[6:8]).all())
    assert same_bits(out[4:6], good[4:6]) and same_bits(out[8:10], good[8:10])


def test_p_losses_error_codes(ctx):
    shape = (2, 4, 8, 6)
    pred, target, w, logvar = pl_inputs(shape, 1)
    _, good = run_p_losses(ctx, pred, target, w, timesteps(2), logvar, "l2")
    p = lambda k: good[k].data_ptr()
    cases = [(dict(model_out=None), -1), (dict(target=None), -1), (dict(t=None), -1), (dict(logvar=None), -1),
             (dict(lvlb_weights=None), -1), (dict(out=None), -1), (dict(ws=None), -1), (dict(batch=0), -1), (dict(c=-4), -1),
             (dict(hw=0), -1), (dict(n_t=0), -1), (dict(loss_type=2), -1), (dict(loss_w_channels=2), -1),
             (dict(model_out=p("model_out") + 2), -1), (dict(out=p("out") + 1), -1), (dict(ws=p("ws") + 8), -1),
             (dict(c=1 << 16, hw=1 << 15, loss_w=None), -2),                     # c * hw does not fit
             (dict(batch=1 << 14, c=1 << 10, hw=1 << 20, loss_w=None), -2),      # 2^32 workgroups
             (dict(ws_bytes=good["ws_bytes"] - 1), -3), (dict(batch=3), -3)]
    for override, code in cases:
        with pytest.raises(_lib.UpkError) as ei:
            ctx.p_losses(**dict(good, **override))
        assert ei.value.code == code, (override, ei.value)
    assert ctx.p_losses_ws_bytes(0, 4, 48) == 0 and ctx.p_losses_ws_bytes(1 << 14, 1 << 10, 1 << 20) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- LatentDiffusion.p_losses
def _fixture():
    g = golden()
    x, noise, w, cond = lr.fixture_inputs(int(g["seed"]))
    cond = {"c_crossattn": cond["c_crossattn"].cuda(), "c_concat": [cond["c_concat"][0].cuda()]}
    return g, x, noise, w, cond, torch.from_numpy(g["t"]).long()


def _model_output(m):
    return m.model.diffusion_model.plan(2, 32, 24, 87, 2, "forward").eps.clone().cpu()


@pytest.mark.parametrize("weights", ["live", "ema"])
def test_p_losses_against_the_reference(weights):
    """tiny recipe, B = 2, t = [999, 3], against the reference's run.  m = the per-sample MSE of our model output against
    the reference's, below 1e-3 (the standing parity target); the per-sample loss within what that m allows (Cauchy-Schwarz
    on mean(w ((a + d)^2 - a^2)), a = target - reference output, d = the difference of the outputs):
        |simple - simple_ref| <= wmax (2 sqrt(plain_ref m) + m) + 1e-6 simple_ref       (l2)
        |simple - simple_ref| <= wmax sqrt(m)                                           (l1)
    Measured on the MI355X: m = 1.2e-6 .. 1.5e-6 for both weight sets; the per-sample loss is off by
    relative 8e-5 .. 1.6e-4 (l2, live), 3e-5 .. 8e-5 (l2, EMA) and 5e-6 .. 7e-5 (l1), where the bounds allow 2e-3 .. 4e-3."""
    import contextlib
    g, x, noise, w, cond, t = _fixture()
    m = get_model()
    assert not m.training
    wmax = float(w.max())
    with (m.ema_scope() if weights == "ema" else contextlib.nullcontext()):
        for case, ltype, lw in (("w", "l2", w), ("none", "l2", None), ("l1", "l1", w)):
            m.loss_type = ltype
            try:
                loss, d = m.p_losses(x.cuda(), cond, t.cuda(), noise=noise.cuda(), loss_w=None if lw is None else lw.cuda())
            finally:
                m.loss_type = "l2"
            assert list(d) == ["val/loss_simple", "val/loss_vlb", "val/loss"]
            assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in d.values()) and loss.dim() == 0
            ours = _model_output(m)
            terms = m.loss_terms.double().cpu().numpy()
            gold = g[weights + "/model_output"]
            mse = ((ours.double().numpy() - gold.astype(np.float64)) ** 2).reshape(2, -1).mean(1)
            ref = lr.p_losses(gold, noise.numpy(), t.numpy(), np.zeros(N_T), g["lvlb_weights"],
                              None if lw is None else lw.numpy(), ltype)
            simple = terms[4::2]
            err = np.abs(simple - ref["simple"])
            wm = wmax if lw is not None else 1.0
            bound = wm * np.sqrt(mse) if ltype == "l1" else wm * (2 * np.sqrt(ref["plain"] * mse) + mse) + 1e-6 * ref["simple"]
            gs, gv = float(g["%s/%s/loss_simple" % (weights, case)]), float(g["%s/%s/loss_vlb" % (weights, case)])
            print("%s %s: model_output MSE per sample %s; simple rel err %s (bound %s); loss_simple %.6f (reference %.6f, rel "
                  "%.2e); loss_vlb %.6f (reference %.6f, rel %.2e)" % (
                      weights, case, ["%.2e" % v for v in mse], ["%.2e" % v for v in err / ref["simple"]],
                      ["%.2e" % v for v in bound / ref["simple"]], float(d["val/loss_simple"]), gs,
                      abs(float(d["val/loss_simple"]) - gs) / gs, float(d["val/loss_vlb"]), gv,
                      abs(float(d["val/loss_vlb"]) - gv) / gv))
            assert (mse < 1e-3).all(), mse
            assert (err <= bound).all(), (err, bound)
            # the dict is the batch view of the same per-sample values (logvar = 0, l_simple_weight = 1, no ELBO term)
            assert abs(float(d["val/loss_simple"]) - simple.mean()) <= 2.0 ** -23 * simple.mean()
            assert float(d["val/loss"]) == float(d["val/loss_simple"]) == float(loss)
            assert abs(float(d["val/loss_simple"]) - gs) <= bound.mean() + 1e-6 * gs
            lvlb_t = g["lvlb_weights"].astype(np.float64)[t.numpy()]
            assert abs(float(d["val/loss_vlb"]) - gv) <= float((lvlb_t * np.where(
                ltype == "l1", np.sqrt(mse), 2 * np.sqrt(ref["plain"] * mse) + mse)).mean()) + 1e-6 * gv


def test_p_losses_keys_prefix_logvar_and_x0():
    """The prefix follows model.training; learn_logvar adds loss_gamma and logvar; a non-zero logvar and ELBO weight enter
    as in the reference's formula; the x0 parameterization takes x_start as the target; noise defaults to a device draw."""
    g, x, noise, w, cond, t = _fixture()
    m = get_model()
    keep = (m.training, m.learn_logvar, m.logvar, m.l_simple_weight, m.original_elbo_weight, m.parameterization)
    xc, nc, wc, tc = x.cuda(), noise.cuda(), w.cuda(), t.cuda()
    try:
        m.training = True
        _, d = m.p_losses(xc, cond, tc, noise=nc, loss_w=wc)
        assert list(d) == ["train/loss_simple", "train/loss_vlb", "train/loss"]
        m.training = False
        m.learn_logvar, m.l_simple_weight, m.original_elbo_weight = True, 0.7, 0.3
        m.logvar = torch.linspace(-0.5, 0.5, N_T)
        loss, d = m.p_losses(xc, cond, tc, noise=nc, loss_w=wc)
        assert list(d) == ["val/loss_simple", "val/loss_gamma", "logvar", "val/loss_vlb", "val/loss"]
        assert abs(float(d["logvar"])) < 1e-6
        ref = lr.p_losses(_model_output(m).numpy(), noise.numpy(), t.numpy(), m.logvar.numpy(), g["lvlb_weights"], w.numpy(),
                          "l2", np.float32(0.7), np.float32(0.3))
        assert abs(float(d["val/loss_gamma"]) - ref["loss_gamma"]) <= EPS * ref["gamma_mag"]
        assert abs(float(loss) - ref["loss"]) <= EPS * ref["loss_mag"] and float(loss) == float(d["val/loss"])
        assert abs(float(d["val/loss_vlb"]) - ref["loss_vlb"]) <= EPS * ref["loss_vlb"]
        m.parameterization = "x0"
        _, d = m.p_losses(xc, cond, tc, noise=nc, loss_w=None)
        ref = lr.p_losses(_model_output(m).numpy(), x.numpy(), t.numpy(), m.logvar.numpy(), g["lvlb_weights"], None, "l2")
        assert abs(float(d["val/loss_simple"]) - ref["loss_simple"]) <= EPS * ref["loss_simple"]
        m.parameterization = "eps"
        torch.manual_seed(7)
        _, d1 = m.p_losses(xc, cond, tc)
        torch.manual_seed(7)
        _, d2 = m.p_losses(xc, cond, tc)
        torch.manual_seed(8)
        _, d3 = m.p_losses(xc, cond, tc)
        assert float(d1["val/loss"]) == float(d2["val/loss"]) != float(d3["val/loss"])
    finally:
        m.training, m.learn_logvar, m.logvar, m.l_simple_weight, m.original_elbo_weight, m.parameterization = keep


# ---------------------------------------------------------------- validation_step / run_validation
def a15_batch(B):
    """The DeepFashion-shaped batch of tests/golden/make_goldens.py (a15_batch), with the loader's loss_w."""
    g0 = torch.Generator().manual_seed(3)
    w = torch.ones(B, 1, 32, 24)
    w[:, :, 0:8], w[:, :, 20:32] = 2.0, 0.5
    return {"image": torch.rand(B, 256, 192, 3, generator=g0) * 2 - 1,
            "txt": torch.randn(B, 77, 768, generator=g0), "styles": 0.45 * torch.randn(B, 9, 768, generator=g0),
            "smpl": 0.5 * torch.randn(B, 1, 85, generator=g0), "person_mask": synth.person_mask(B, 32, 24), "loss_w": w}


KEYS = ["val/loss_simple", "val/loss_vlb", "val/loss", "val/loss_simple_ema", "val/loss_vlb_ema", "val/loss_ema"]


def test_validation_step():
    m = get_model()
    batch = {k: v.cuda() for k, v in a15_batch(2).items()}
    logged = []
    m.log_dict = lambda d, **k: logged.append((dict(d), k))
    try:
        torch.manual_seed(21)
        d1 = m.validation_step(batch, 0)
        torch.manual_seed(21)
        d2 = m.validation_step(batch, 0)
    finally:
        del m.log_dict
    assert list(d1) == KEYS and len(logged) == 2 and list(logged[0][0]) == KEYS and logged[0][1]["on_epoch"] is True
    v1, v2 = [float(d1[k]) for k in KEYS], [float(d2[k]) for k in KEYS]
    print("validation_step:", dict(zip(KEYS, v1)))
    assert all(np.isfinite(v1)) and v1 == v2
    assert all(a != b for a, b in zip(v1[:3], v1[3:]))  # (the EMA weights are another recipe draw)
    assert m.model.diffusion_model._weight_override is None


class _Batches:
    def __init__(self, batch, sizes):
        self.batch, self.sizes, self.asked = batch, sizes, []

    def batches(self, batch_size):
        self.asked.append(batch_size)
        i = 0
        for n in self.sizes:
            yield {k: v[i:i + n] for k, v in self.batch.items()}
            i += n


def test_run_validation(tmp_path, monkeypatch):
    """Three batches of sizes 2, 2 and 1: the epoch means are the size-weighted means of the validation_step dicts, and the
    whole run synchronises once."""
    m = get_model()
    data = _Batches({k: v.cuda() for k, v in a15_batch(5).items()}, (2, 2, 1))
    evaluate.run_validation(m, data, batch_size=2, seed=5)  # (plans and packed weights exist from here on)
    torch.manual_seed(5)
    dicts = [m.validation_step(b, i) for i, b in enumerate(data.batches(2))]
    want = {k: sum(float(d[k]) * n for d, n in zip(dicts, (2, 2, 1))) / 5.0 for k in KEYS}
    syncs = []
    count = lambda name, fn: (lambda *a, **k: (syncs.append(name), fn(*a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", count("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", count("Stream.synchronize", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", count("Event.synchronize", torch.cuda.Event.synchronize))
    for name in ("item", "cpu", "tolist", "numpy"):
        fn = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda name, fn: lambda self, *a, **k: (
            syncs.append(name) if self.is_cuda else None, fn(self, *a, **k))[1])(name, fn))
    got = evaluate.run_validation(m, data, batch_size=2, seed=5, save_dir=tmp_path)
    monkeypatch.undo()
    assert syncs == ["Stream.synchronize"], syncs
    assert data.asked[-1] == 2 and list(got) == KEYS and all(isinstance(v, float) for v in got.values())
    for k in KEYS:
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])
    assert json.load(open(tmp_path / "val_metrics.json")) == got
    two = evaluate.run_validation(m, data, batch_size=2, seed=5, max_batches=2)
    want2 = {k: sum(float(d[k]) * n for d, n in zip(dicts[:2], (2, 2))) / 4.0 for k in KEYS}
    assert all(abs(two[k] - want2[k]) <= 1e-6 * abs(want2[k]) for k in KEYS)
