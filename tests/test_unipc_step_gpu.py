"""upk_unipc_step_f32 (upgpt_amd/csrc/unipc.hip) through the C ABI against tests/unipc_ref.py: the fp64 restatement of one
launch and its bound |got - ref64| <= 64 * 2^-24 * A.

As in test_dpm_step_gpu.py, every device buffer a launch may touch sits between sentinel-filled guard regions at least one
latent long, the static / pad channels of xin hold a random pattern, and all of them — and every operand the launch only
reads — must come back bit-identical.  Before every launch x_corr and every ring slot the row's zero weights say the kernel
must not read are filled with NaN: it may not load them, not even to multiply them by a zero weight."""
import numpy as np
import pytest
import torch

import unipc_ref as R
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 32          # xin row stride: C latent channels, live concat channels behind them, pad up to 32
SENT = -1234.5
SCALE = 3.0
S_ROWS = 6       # the order-3 table: (corrector, predictor) orders (0,1) (1,2) (2,3) (3,3) (3,2) (2,1) per row
SHAPES = [(1, 4, 3, 5), (2, 4, 8, 6), (3, 3, 5, 7), (2, 4, 32, 24)]  # 1, 1, 1 (C != 4, n % 4 != 0) and 6 workgroups
ROWS = [0, 1, 2, 3, 5]
NAN = float("nan")
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.float16: torch.int16}


def _bits(t):
    return t.view(_BITS[t.dtype])


class Guarded:
    """`live` (a CPU tensor) on the device between two guard regions of `guard` elements filled with a sentinel."""

    def __init__(self, live, guard, shift=0):
        guard = (guard + 63) // 64 * 64 + shift
        n = live.numel()
        self.sent = SENT if live.dtype.is_floating_point else int(SENT)
        self.full = torch.full((2 * guard + n,), self.sent, dtype=live.dtype, device=DEV)
        self.live = self.full[guard:guard + n].view(live.shape)
        self.live.copy_(live)
        self.guards = (self.full[:guard], self.full[guard + n:])
        self.before = None

    def snapshot(self):
        self.before = self.full.clone()

    def guards_intact(self):
        sent = _bits(torch.tensor(self.sent, dtype=self.full.dtype)).item()
        return all(bool((_bits(g) == sent).all()) for g in self.guards)

    def unchanged(self):
        return torch.equal(_bits(self.full), _bits(self.before))

    def live_before(self):
        g = self.guards[0].numel()
        return self.before[g:g + self.live.numel()].view(self.live.shape)


def _nhwc(x, B, C, hw):
    """[B, C, H, W] values -> [B * hw, C] in xin's row order."""
    return x.reshape(B, C, hw).permute(0, 2, 1).reshape(B * hw, C)


def _table():
    """The real S = 6 order-3 logSNR table of the configs' schedule, fp32 as the kernel reads it."""
    acp = R.linear_alphas_cumprod()
    tab = R.coefficient_table(*R.tables(acp, R.logsnr_nodes(acp, S_ROWS)[1:]), order=3)
    assert [int(v) for v in tab[:, 11]] == [0, 1, 1, 1, 1, 1]
    assert [(bool(r[5]), bool(r[6]), bool(r[9]), bool(r[10])) for r in tab] == [
        (False, False, False, False), (False, False, True, False), (True, False, True, True), (True, True, True, True),
        (True, True, True, False), (True, False, False, False)]
    return torch.from_numpy(tab.astype(np.float32))


def _inputs(shape, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"x": 2.0 * rn(*shape), "eps": rn(2 if cfg else 1, *shape), "hist": 1.5 * rn(3, *shape), "x_corr": 2.0 * rn(*shape)}


def _run(ctx, shape, cfg, row, null, ld=LD, shift=0):
    """One launch with the operand named by `null` (None / "pred" / "xin" / "step") passed as NULL; everything checked."""
    B, C, H, W = shape
    hw, n = H * W, int(np.prod(shape))
    halves = 2 if cfg else 1
    inp, tab = _inputs(shape, cfg, 100 * row + n), _table()
    if null == "step":  # step == NULL reads row 0 (and the ring slots of evaluation 0): the table from `row` on
        tab, row = tab[row:].clone(), 0
    reads = R.step(inp["x"].numpy(), inp["eps"].numpy(), tab.numpy(), row, inp["hist"].numpy(), inp["x_corr"].numpy(),
                   SCALE, cfg).reads
    s0, s1, s2 = R.slots(row)
    hist, x_corr = inp["hist"].clone(), inp["x_corr"].clone()
    for name, slot in (("h0", s0), ("h1", s1), ("h2", s2)):  # what the row does not name is poison
        if not reads[name]:
            hist[slot] = NAN
    if not reads["x_corr"]:
        x_corr[:] = NAN
    ref = R.step(inp["x"].numpy(), inp["eps"].numpy(), tab.numpy(), row, hist.numpy(), x_corr.numpy(), SCALE, cfg)
    G = n + 256
    g = torch.Generator().manual_seed(n)
    d = {"x": Guarded(inp["x"], G), "eps": Guarded(inp["eps"], G), "coefs": Guarded(tab, G), "hist": Guarded(hist, G),
         "x_corr": Guarded(x_corr, G), "done": Guarded(torch.zeros(1, dtype=torch.int32), 64)}
    if null != "pred":
        d["pred"] = Guarded(torch.full(shape, 5.0), G)
    if null != "xin":
        d["xin"] = Guarded((torch.randn(halves * B * hw, ld, generator=g) * 3.0).half(), G, shift)
    if null != "step":
        d["step"] = Guarded(torch.tensor([row], dtype=torch.int32), 64)
    for b in d.values():
        b.snapshot()
    p = lambda k: d[k].live if k in d else None
    torch.cuda.synchronize()
    ctx.step_autoadvance(d["done"].live)
    try:
        ctx.unipc_step(p("x"), p("eps"), p("coefs"), p("step"), p("hist"), p("x_corr"), p("pred"), p("xin"), ld, B, C, hw,
                       cfg_scale=SCALE, cfg=cfg)
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    tag = (shape, cfg, row, null, ld, shift)
    assert int(d["done"].live.item()) == 0, tag  # the arrival counter is re-armed
    if "step" in d:
        assert int(d["step"].live.item()) == row + 1, tag
    x, ring, was = d["x"].live, d["hist"].live, d["hist"].live_before()
    for name, got, want, A in (("x", x, ref.x, ref.A["x"]), ("x_corr", d["x_corr"].live, ref.xc, ref.A["xc"]),
                               ("m", ring[s2], ref.m, ref.A["m"])):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), tag + (name,)
        dev = np.abs(got - want)
        worst = float((dev / np.maximum(A, 1e-30)).max()) / R.BOUND
        print("%s %s: worst error / bound %.3f" % (tag, name, worst))
        assert R.within(got, want, A).all(), tag + (name, worst)
    for slot in (s0, s1):  # the ring: one slot written, two left alone (NaN poison included)
        assert torch.equal(_bits(ring[slot]), _bits(was[slot])), tag + (slot,)
    if not reads["x_corr"]:
        assert torch.equal(d["x_corr"].live.cpu(), inp["x"]), tag  # no corrector: x_corr is the latent it was handed
    if "pred" in d:
        assert torch.equal(_bits(d["pred"].live), _bits(ring[s2])), tag  # both are m
    if "xin" in d:
        xin, before = d["xin"].live, d["xin"].live_before()
        assert torch.equal(_bits(xin[:, C:]), _bits(before[:, C:])), tag  # static concat channels and pad
        lat = xin[:B * hw, :C]
        want = _nhwc(torch.from_numpy(ref.xin).reshape(shape), B, C, hw)
        tol = R.BOUND * _nhwc(torch.from_numpy(ref.A["x"]).reshape(shape), B, C, hw) + 2.0 ** -11 * want.abs() + 2.0 ** -25
        assert bool(((lat.double().cpu() - want).abs() <= tol).all()), tag
        assert torch.equal(_bits(lat), _bits(_nhwc(x, B, C, hw).half())), tag  # the written x rounded once, bit for bit
        if cfg:
            assert torch.equal(_bits(xin[B * hw:, :C]), _bits(lat)), tag  # both halves refreshed identically
    for name, b in d.items():
        assert b.guards_intact(), tag + (name,)
    for name in ("eps", "coefs"):
        assert d[name].unchanged(), tag + (name,)
    return ref


_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_single_launch_parity(ctx, shape, cfg):
    seen = []
    for row in ROWS:
        for null in (None, "pred", "xin", "step"):
            r = _run(ctx, shape, cfg, row, null).reads
            seen.append((r["x_corr"], r["h0"], r["h1"], r["h2"]))
    # the cases do run every branch: nothing / corrector 1 / corrector 2 + predictor 3 / corrector 3 / corrector 2 alone
    assert seen[::4] == [(False, False, False, False), (True, True, False, False), (True, True, True, False),
                         (True, True, True, True), (True, True, True, False)]
    assert all(seen[i] == seen[i - i % 4] for i in range(len(seen)))


@pytest.mark.parametrize("ld,shift", [(6, 0), (5, 0), (32, 2), (4, 1)])
def test_xin_rows_that_are_not_8_byte_aligned(ctx, ld, shift):
    """C = 4 writes a pixel's row as one 8-byte store only where the row's address allows it: strides of 12 and 10 bytes
    and bases 4 and 2 bytes off take the element stores for some or all rows, inside one launch."""
    for cfg in (False, True):
        _run(ctx, (2, 4, 8, 6), cfg, 3, None, ld=ld, shift=shift)


def test_guidance_changes_the_result(ctx):
    plain = _run(ctx, SHAPES[1], False, 3, None)
    guided = _run(ctx, SHAPES[1], True, 3, None)
    assert float(np.abs(plain.x - guided.x).max()) > 1e-2 and float(np.abs(plain.xc - guided.xc).max()) > 1e-2


def test_error_returns(ctx):
    """UPK_EINVAL (-1) for a missing operand, a non-positive extent, a stem input narrower than the latent or a pointer
    that is not aligned to its element; nothing is launched, nothing written."""
    shape = SHAPES[1]
    B, C, H, W = shape
    hw, n = H * W, int(np.prod(shape))
    inp = _inputs(shape, False, 1)
    d = {"x": Guarded(inp["x"], n), "eps": Guarded(inp["eps"], n), "coefs": Guarded(_table(), n),
         "hist": Guarded(inp["hist"], n), "x_corr": Guarded(inp["x_corr"], n), "pred": Guarded(torch.zeros(shape), n),
         "xin": Guarded(torch.zeros(B * hw, LD).half(), n), "step": Guarded(torch.zeros(1, dtype=torch.int32), 64)}
    for b in d.values():
        b.snapshot()
    good = dict(x=d["x"].live, eps=d["eps"].live, coefs=d["coefs"].live, step=d["step"].live, hist=d["hist"].live,
                x_corr=d["x_corr"].live, pred_x0=d["pred"].live, xin=d["xin"].live, ld_xin=LD, batch=B, c=C, hw=hw)
    off = lambda k, by: good[k].data_ptr() + by
    bad = [dict(x=None), dict(eps=None), dict(coefs=None), dict(hist=None), dict(x_corr=None), dict(batch=0), dict(c=0),
           dict(hw=0), dict(batch=-1), dict(ld_xin=C - 1), dict(x=off("x", 2)), dict(eps=off("eps", 1)),
           dict(coefs=off("coefs", 2)), dict(step=off("step", 2)), dict(hist=off("hist", 3)), dict(x_corr=off("x_corr", 2)),
           dict(pred_x0=off("pred_x0", 2)), dict(xin=off("xin", 1))]
    for change in bad:
        with pytest.raises(L.UpkError) as ei:
            ctx.unipc_step(**dict(good, **change))
        assert ei.value.code == -1, change
    assert ctx.lib.upk_unipc_step_f32(None, *([None] * 8), LD, B, C, hw, 1.0, 0, None) == -1  # no context
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in d.values())  # nothing was launched
    ctx.unipc_step(**dict(good, xin=None, ld_xin=0))  # (ld_xin is not looked at without xin)
    torch.cuda.synchronize()
    assert all(d[k].unchanged() for k in ("eps", "coefs", "xin", "step")) and all(b.guards_intact() for b in d.values())
