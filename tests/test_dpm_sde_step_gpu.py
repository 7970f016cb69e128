"""upk_dpmpp_2m_sde_step_f32 (upgpt_amd/csrc/dpm_sde.hip) through the C ABI against tests/sde_ref.py: the fp64 restatement
of one launch and its bound |got - ref64| <= 40 * 2^-24 * A.

As in test_unipc_step_gpu.py, every device buffer a launch may touch sits between sentinel-filled guard regions, the static /
pad channels of xin hold a random pattern, and all of them — and every operand the launch only reads — must come back
bit-identical.  On a first-order row m_old holds NaN before the launch: the kernel may not load it.  The mask holds 0, 1 and
0.25: where it is 1 the written x is the keep row bit for bit, where it is 0 it is x_plain bit for bit."""
import itertools

import numpy as np
import pytest
import torch

import sde_ref as R
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1234.5
SCALE = 3.0
S_ROWS = 6
# (B, C, hw, ld_xin, shift of the xin base in halves): one pixel; one partial block; two blocks and the general-C row; two
# blocks with rows of 16 bytes on a base 2 bytes off an 8-byte boundary — every C = 4 row takes the element stores
SHAPES = [(1, 4, 1, 32, 0), (2, 4, 96, 32, 0), (3, 3, 130, 32, 0), (2, 4, 260, 8, 1)]
ROWS = [0, 2, 5]  # first-order (the chain's first), second-order, the first-order last row (never blended)
ETAS = [0.0, 0.5, 1.0]
NAN = float("nan")
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.float16: torch.int16}
_worst = {"frac": 0.0}


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
    """[B, C, hw] values -> [B * hw, C] in xin's row order."""
    return x.reshape(B, C, hw).permute(0, 2, 1).reshape(B * hw, C)


_tables = {}


def _table(eta):
    """The real S = 6 logSNR table of the configs' schedule at `eta`, fp32 as the kernel reads it."""
    if eta not in _tables:
        acp = R.linear_alphas_cumprod()
        tab = R.coefficient_table(*R.tables(acp, R.logsnr_nodes(acp, S_ROWS)[1:]), eta=eta)
        assert [bool(w) for w in tab[:, 4]] == [False, True, True, True, True, False]
        _tables[eta] = torch.from_numpy(tab.astype(np.float32))
    return _tables[eta]


def _inputs(shape, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    n = int(np.prod(shape))
    mask = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.25])[torch.randint(0, 5, (n,), generator=g)]
    return {"x": 2.0 * rn(*shape), "eps": rn(2 if cfg else 1, *shape), "m_old": 1.5 * rn(*shape),
            "noise": 0.7 * rn(S_ROWS, n), "keep": 2.0 * rn(S_ROWS, n), "mask": mask}


def _run(ctx, case, eta, row, cfg, noise, mask, null):
    """One launch; `null` (None / "pred" / "plain" / "xin" / "step") names the optional operand passed as NULL."""
    B, C, hw, ld, shift = case
    shape = (B, C, hw)
    n = B * C * hw
    halves = 2 if cfg else 1
    inp, tab = _inputs(shape, cfg, 1000 * row + n), _table(eta)
    n_rows = S_ROWS
    if null == "step":  # step == NULL reads row 0 of the coefficients and the noise and keep row 1: the tables from `row` on
        tab, inp["noise"], inp["keep"] = tab[row:].clone(), inp["noise"][row:].clone(), inp["keep"][row:].clone()
        n_rows, row = n_rows - row, 0
    second = bool(tab[row, 4] != 0)
    m_old = inp["m_old"].clone()
    if not second:
        m_old[:] = NAN  # a first-order row must not load it
    ref = R.step(inp["x"].numpy(), inp["eps"].numpy(), tab.numpy(), row, m_old.numpy(), inp["noise"].numpy() if noise else None,
                 inp["keep"].numpy() if mask else None, inp["mask"].numpy() if mask else None, n_rows, SCALE, cfg)
    assert ref.second == second and ref.blended == (mask and row + 1 < n_rows)
    G = n + 256
    g = torch.Generator().manual_seed(n)
    d = {"x": Guarded(inp["x"], G), "eps": Guarded(inp["eps"], G), "coefs": Guarded(tab, G), "m_old": Guarded(m_old, G),
         "done": Guarded(torch.zeros(1, dtype=torch.int32), 64)}
    if noise:
        d["noise"] = Guarded(inp["noise"], G)
    if mask:
        d["keep"], d["mask"] = Guarded(inp["keep"], G), Guarded(inp["mask"], G)
    if null != "pred":
        d["pred"] = Guarded(torch.full(shape, 5.0), G)
    if null != "plain":
        d["plain"] = Guarded(torch.full(shape, 6.0), G)
    if null != "xin":
        d["xin"] = Guarded((torch.randn(halves * B * hw, ld, generator=g) * 3.0).half(), G, shift)
        assert d["xin"].live.data_ptr() % 8 == (2 * shift) % 8
    if null != "step":
        d["step"] = Guarded(torch.tensor([row], dtype=torch.int32), 64)
    for b in d.values():
        b.snapshot()
    p = lambda k: d[k].live if k in d else None
    torch.cuda.synchronize()
    ctx.step_autoadvance(d["done"].live)
    try:
        ctx.dpmpp_2m_sde_step(p("x"), p("eps"), p("coefs"), p("noise"), p("keep"), p("mask"), n_rows, p("step"), p("m_old"),
                              p("pred"), p("plain"), p("xin"), ld, B, C, hw, cfg_scale=SCALE, cfg=cfg)
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    tag = (case, eta, row, cfg, noise, mask, null)
    assert int(d["done"].live.item()) == 0, tag  # the arrival counter is re-armed
    if "step" in d:
        assert int(d["step"].live.item()) == row + 1, tag  # advanced once
    x = d["x"].live
    outs = [("x", x, ref.x, ref.A["x"]), ("m_old", d["m_old"].live, ref.m, ref.A["m"])]
    if "plain" in d:
        outs.append(("x_plain", d["plain"].live, ref.x_plain, ref.A["x_plain"]))
    for name, got, want, A in outs:
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), tag + (name,)
        frac = float((np.abs(got - want) / np.maximum(A, 1e-30)).max()) / R.BOUND
        _worst["frac"] = max(_worst["frac"], frac)
        assert R.within(got, want, A).all(), tag + (name, frac)
    if "pred" in d:
        assert torch.equal(_bits(d["pred"].live), _bits(d["m_old"].live)), tag  # both are m
    if "plain" in d:
        plain = d["plain"].live.reshape(-1)
        if ref.blended:
            mk, kp = inp["mask"].to(DEV), d["keep"].live[row + 1]
            assert torch.equal(_bits(x.reshape(-1)[mk == 1]), _bits(kp[mk == 1])), tag  # kept: the keep row, bit for bit
            assert torch.equal(_bits(x.reshape(-1)[mk == 0]), _bits(plain[mk == 0])), tag  # generated: the plain update
            assert not bool((mk == 1).any()) or not torch.equal(x.reshape(-1), plain), tag
        else:
            assert torch.equal(_bits(x.reshape(-1)), _bits(plain)), tag  # no mask, or the last row: unblended
    if "xin" in d:
        xin, before = d["xin"].live, d["xin"].live_before()
        assert torch.equal(_bits(xin[:, C:]), _bits(before[:, C:])), tag  # static concat channels and pad
        lat = xin[:B * hw, :C]
        assert torch.equal(_bits(lat), _bits(_nhwc(x, B, C, hw).half())), tag  # the written x rounded once, bit for bit
        if cfg:
            assert torch.equal(_bits(xin[B * hw:, :C]), _bits(lat)), tag  # both halves refreshed identically
    for name, b in d.items():
        assert b.guards_intact(), tag + (name,)
    for name in ("eps", "coefs", "noise", "keep", "mask"):
        assert name not in d or d[name].unchanged(), tag + (name,)
    return ref


_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("case", SHAPES, ids=_ids)
def test_single_launch_parity(ctx, case, cfg):
    seen = set()
    for eta, row, noise, mask in itertools.product(ETAS, ROWS, (False, True), (False, True)):
        for null in (None, "pred", "plain", "xin", "step"):
            r = _run(ctx, case, eta, row, cfg, noise, mask, null)
            seen.add((r.second, r.blended))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}  # every branch ran
    print("%s cfg %s: worst error / bound so far %.3f" % (case, cfg, _worst["frac"]))


def test_noise_mask_and_guidance_change_the_result(ctx):
    case = SHAPES[1]
    base = _run(ctx, case, 1.0, 2, False, False, False, None)
    for kw in (dict(cfg=True), dict(noise=True), dict(mask=True)):
        args = dict(dict(cfg=False, noise=False, mask=False), **kw)
        other = _run(ctx, case, 1.0, 2, args["cfg"], args["noise"], args["mask"], None)
        assert float(np.abs(base.x - other.x).max()) > 1e-2, kw


def test_error_returns(ctx):
    """UPK_EINVAL (-1) for a missing operand, a mask without keep rows, a non-positive extent, a stem input narrower than
    the latent or a pointer that is not aligned to its element; nothing is launched, the poisoned outputs stay."""
    B, C, hw, LD, _ = SHAPES[1]
    shape, n = (B, C, hw), B * C * hw
    inp = _inputs(shape, False, 1)
    poison = lambda: torch.full(shape, 7.0)
    d = {"x": Guarded(inp["x"], n), "eps": Guarded(inp["eps"], n), "coefs": Guarded(_table(1.0), n),
         "noise": Guarded(inp["noise"], n), "keep": Guarded(inp["keep"], n), "mask": Guarded(inp["mask"], n),
         "m_old": Guarded(poison(), n), "pred": Guarded(poison(), n), "plain": Guarded(poison(), n),
         "xin": Guarded(torch.full((B * hw, LD), 7.0).half(), n), "step": Guarded(torch.ones(1, dtype=torch.int32), 64)}
    for b in d.values():
        b.snapshot()
    good = dict(x=d["x"].live, eps=d["eps"].live, coefs=d["coefs"].live, noise=d["noise"].live, keep=d["keep"].live,
                mask=d["mask"].live, n_rows=S_ROWS, step=d["step"].live, m_old=d["m_old"].live, pred_x0=d["pred"].live,
                x_plain=d["plain"].live, xin=d["xin"].live, ld_xin=LD, batch=B, c=C, hw=hw)
    off = lambda k, by: good[k].data_ptr() + by
    bad = [dict(x=None), dict(eps=None), dict(coefs=None), dict(m_old=None), dict(keep=None), dict(n_rows=0),
           dict(n_rows=-1), dict(batch=0), dict(c=0), dict(hw=0), dict(batch=-1), dict(ld_xin=C - 1)]
    bad += [dict([(k, off(k, 2))]) for k in ("x", "eps", "coefs", "noise", "keep", "mask", "step", "m_old", "pred_x0", "x_plain")]
    bad += [dict(m_old=off("m_old", 1)), dict(xin=off("xin", 1))]
    for change in bad:
        with pytest.raises(L.UpkError) as ei:
            ctx.dpmpp_2m_sde_step(**dict(good, **change))
        assert ei.value.code == -1, change
    assert ctx.lib.upk_dpmpp_2m_sde_step_f32(None, *([None] * 6), S_ROWS, *([None] * 5), LD, B, C, hw, 1.0, 0, None) == -1
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in d.values())  # nothing was launched
    # (without a mask keep and n_rows are not looked at; without xin ld_xin is not)
    ctx.dpmpp_2m_sde_step(**dict(good, mask=None, keep=None, n_rows=0, xin=None, ld_xin=0))
    torch.cuda.synchronize()
    assert all(d[k].unchanged() for k in ("eps", "coefs", "noise", "keep", "mask", "xin", "step"))
    assert all(b.guards_intact() for b in d.values())
    assert not torch.equal(d["pred"].live.cpu(), poison())  # (that one did run)
