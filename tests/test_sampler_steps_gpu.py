"""The four fused sampler step kernels and the device-side step counter (upgpt_amd/csrc/misc.hip) through the C ABI,
against oracle/steps.py: the fp64 restatement of one launch and its derived bound |got - ref64| <= 32 * 2^-24 * A.

Every device buffer a launch may touch sits between sentinel-filled guard regions at least one table row long, and the
static / pad channels of xin hold a random pattern: all of them, and every operand the launch only reads, must come
back bit-identical."""
import numpy as np
import pytest
import torch

from oracle import steps as st
from upgpt_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 32          # xin row stride: C latent channels, live concat channels behind them, pad up to 32
SENT = -1234.5
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.float16: torch.int16}


def _bits(t):
    return t.view(_BITS[t.dtype])


class Guarded:
    """`live` (a CPU tensor) on the device between two guard regions of `guard` elements filled with a sentinel."""

    def __init__(self, live, guard):
        guard = (guard + 63) // 64 * 64
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


def _make_xin(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, LD, generator=g) * 3.0).half()  # stale latent channels, live concat channels, pad


def _launch(ctx, kernel, d, mode, shape, cfg, step_t, scale=st.CFG_SCALE):
    """One launch of `kernel` on the Guarded buffers in d (absent = NULL)."""
    B, C, H, W = shape
    p = lambda k: d[k].live if k in d else None
    tail = (p("pred"), p("xin"), LD, B, C, H * W)
    if kernel == "ddim":
        ctx.ddim_step(p("x"), p("eps"), p("coefs"), p("noise"), step_t, *tail)
    elif kernel == "ddim_cfg":
        ctx.ddim_step_cfg(p("x"), p("eps"), p("coefs"), p("noise"), step_t, *tail, scale)
    elif kernel == "plms":
        ctx.plms_step(p("x"), p("eps"), p("coefs"), step_t, p("hist"), *tail, scale, cfg)
    else:
        ctx.ddpm_step(p("x"), p("eps"), p("coefs"), p("noise"), p("noise2"), p("x0"), p("mask"), step_t, *tail,
                      mode.get("flags", 0))


def _upload(kernel, inp, mode, cfg):
    """Guarded device copies of the operands of one launch (the guards are longer than a table row, so that even a row
    index off by one stays inside the allocation)."""
    kw = st.operands(kernel, inp, mode)
    B, C, H, W = inp["shape"]
    n, G = inp["n"], inp["n"] + 256
    d = {"x": Guarded(inp["x"], G), "coefs": Guarded(inp["coefs"], G),
         "eps": Guarded(kw["eps2"] if kernel == "ddim_cfg" else kw["model_out"] if kernel == "ddpm" else kw["eps"], G),
         "done": Guarded(torch.zeros(1, dtype=torch.int32), 64)}
    for k in ("noise", "noise2", "x0", "mask", "hist"):
        if kw.get(k) is not None:
            d[k] = Guarded(kw[k], G)
    if mode["pred"]:
        d["pred"] = Guarded(torch.full(inp["shape"], 5.0), G)
    if mode["xin"]:
        d["xin"] = Guarded(_make_xin(B * H * W * (2 if cfg else 1), C, n), G)
    if mode["step"] is not None:
        d["step"] = Guarded(torch.tensor([mode["step"]], dtype=torch.int32), 64)
    return d, kw


def _check_launch(ctx, kernel, inp, mode):
    shape = inp["shape"]
    B, C, H, W = shape
    hw = H * W
    cfg = kernel == "ddim_cfg" or (kernel == "plms" and mode["cfg"])
    d, kw = _upload(kernel, inp, mode, cfg)
    ref = st.STEP_FNS[kernel](**kw)
    for b in d.values():
        b.snapshot()
    torch.cuda.synchronize()
    ctx.step_autoadvance(d["done"].live)
    try:
        _launch(ctx, kernel, d, mode, shape, cfg, d["step"].live if "step" in d else None)
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    tag = (kernel, shape, mode)
    # the step counter: + 1 exactly, the arrival counter re-armed
    assert int(d["done"].live.item()) == 0, tag
    if "step" in d:
        assert int(d["step"].live.item()) == mode["step"] + 1, tag
    # x, pred_x0 and the history ring against the fp64 restatement
    x = d["x"].live
    assert bool(st.within(x, ref.x, ref.A["x"]).all()), tag
    if ref.commit:
        if "pred" in d:
            assert bool(st.within(d["pred"].live, ref.pred_x0, ref.A["pred_x0"]).all()), tag
    else:  # PLMS evaluation 0: x and pred_x0 are not committed
        assert d["x"].unchanged() and ("pred" not in d or d["pred"].unchanged()), tag
    if "hist" in d:
        hist = d["hist"].live.reshape(3, *shape)
        assert bool(st.within(hist, ref.hist, ref.A["hist"]).all()), tag
        for s in range(3):  # a slot the step does not own
            if s != ref.slot:
                assert torch.equal(_bits(d["hist"].live[s]), _bits(d["hist"].live_before()[s])), tag + (s,)
    # the stem input
    if "xin" in d:
        xin, was = d["xin"].live, d["xin"].live_before()
        assert torch.equal(_bits(xin[:, C:]), _bits(was[:, C:])), tag  # static concat channels and pad
        lat = xin[:B * hw, :C]
        want = _nhwc(ref.xin, B, C, hw)
        tol = st.BOUND * _nhwc(ref.A["xin"], B, C, hw) + 2.0 ** -11 * want.abs() + 2.0 ** -25  # + the fp16 rounding
        assert bool(((lat.double().cpu() - want).abs() <= tol).all()), tag
        if ref.commit:
            assert torch.equal(_bits(lat), _bits(_nhwc(x, B, C, hw).half())), tag  # .half() of the x the kernel wrote
        if cfg:
            assert torch.equal(_bits(xin[B * hw:, :C]), _bits(lat)), tag  # both halves refreshed identically
    # guards, and everything the launch only reads
    for name, b in d.items():
        assert b.guards_intact(), tag + (name,)
    for name in ("eps", "coefs", "noise", "noise2", "x0", "mask"):
        if name in d:
            assert d[name].unchanged(), tag + (name,)


_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", st.SHAPES, ids=_ids)
@pytest.mark.parametrize("kernel", st.KERNELS)
def test_single_launch_parity(ctx, kernel, shape):
    inp = st.make_inputs(kernel, shape)
    for mode in st.modes(kernel):
        _check_launch(ctx, kernel, inp, mode)


def test_plms_needs_its_evaluation_counter(ctx):
    """upk_plms_step_f32 has no `step == NULL` mode (include/upk.h: *step is the evaluation counter): the call is
    refused and nothing is written."""
    inp = st.make_inputs("plms", st.SHAPES[2])
    mode = dict(noise=False, pred=True, xin=True, step=0, cfg=False)
    d, _ = _upload("plms", inp, mode, False)
    for b in d.values():
        b.snapshot()
    with pytest.raises(L.UpkError) as ei:
        _launch(ctx, "plms", d, mode, inp["shape"], False, None)
    torch.cuda.synchronize()
    assert ei.value.code == -1 and all(b.unchanged() for b in d.values())


# ------------------------------------------------------------------------------------------------------ step counter
@pytest.mark.parametrize("kernel", st.KERNELS)
def test_step_counter_armed_disarmed_null(ctx, kernel):
    inp = st.make_inputs(kernel, st.SHAPES[2])  # two workgroups, the second ragged
    mode = dict(noise=True, pred=True, xin=True, step=3, flags=0, mask=None, cfg=False)
    if kernel == "plms":
        mode["noise"] = False
    cfg = kernel == "ddim_cfg"
    d, _ = _upload(kernel, inp, mode, cfg)
    step, done = d["step"].live, d["done"].live
    seen = []
    for armed, with_step in ((True, True), (False, True), (True, False), (True, True)):
        if kernel == "plms" and not with_step:
            continue
        ctx.step_autoadvance(done if armed else None)
        try:
            _launch(ctx, kernel, d, mode, inp["shape"], cfg, step if with_step else None)
        finally:
            ctx.step_autoadvance(None)
        torch.cuda.synchronize()
        seen.append((int(step.item()), int(done.item())))
    want = [(4, 0), (4, 0), (4, 0), (5, 0)] if kernel != "plms" else [(4, 0), (4, 0), (5, 0)]
    assert seen == want
    assert all(b.guards_intact() for b in d.values())


N_LONG = 200


def _long_buffers(kernel, shape, rows):
    """Device operands for `rows` back-to-back launches: distinct coefficient rows whose update contracts (the
    trajectory stays O(1)), fresh eps per launch."""
    B, C, H, W = shape
    n = B * C * H * W
    g = torch.Generator(device=DEV).manual_seed(11 + st.KERNELS.index(kernel))
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    cfg = kernel in ("ddim_cfg", "plms")
    b = {"x0_init": 2.0 * rn(n), "eps_all": rn(rows, (2 if cfg else 1) * n),
         "coefs": 0.3 + 0.6 * torch.rand(rows + 1, 8 if kernel == "ddpm" else 4, generator=g, device=DEV)}
    if kernel != "plms":  # (a spare row in front: a row index off by one stays inside the allocation)
        b["noise"] = (0.5 * rn(rows + 1, n))[1:]
    if kernel == "ddpm":
        b["noise2"], b["x0"] = (0.5 * rn(rows + 1, n))[1:], rn(n)
        b["mask"] = (torch.arange(n, device=DEV) % 3).float() * 0.5
    for k, shp, dt in (("x", n, torch.float32), ("pred", n, torch.float32), ("hist", 3 * n, torch.float32),
                       ("step", 1, torch.int32), ("done", 1, torch.int32)):
        b[k] = torch.zeros(shp, dtype=dt, device=DEV)
    b["xin"] = torch.zeros(B * H * W * (2 if cfg else 1), LD, dtype=torch.float16, device=DEV)
    return b


def _long_launch(ctx, kernel, b, eps, shape):
    B, C, H, W = shape
    tail = (b["pred"], b["xin"], LD, B, C, H * W)
    if kernel == "ddim":
        ctx.ddim_step(b["x"], eps, b["coefs"], b["noise"], b["step"], *tail)
    elif kernel == "ddim_cfg":
        ctx.ddim_step_cfg(b["x"], eps, b["coefs"], b["noise"], b["step"], *tail, st.CFG_SCALE)
    elif kernel == "plms":
        ctx.plms_step(b["x"], eps, b["coefs"], b["step"], b["hist"], *tail, st.CFG_SCALE, True)
    else:
        ctx.ddpm_step(b["x"], eps, b["coefs"], b["noise"], b["noise2"], b["x0"], b["mask"], b["step"], *tail,
                      st.UPK_DDPM_CLIP)


def _reset(b):
    b["x"].copy_(b["x0_init"])
    for k in ("pred", "hist", "step", "done", "xin"):
        b[k].zero_()


def _state(b):
    return [_bits(b[k]).clone() for k in ("x", "pred", "hist", "xin")]


@pytest.mark.parametrize("kernel", st.KERNELS)
def test_autoadvance_over_200_launches_and_in_a_graph(ctx, kernel):
    """One deterministic pass at the 576-workgroup shape: the kernels' own increment gives the trajectory of
    upk_advance_step between the launches, bit for bit, eager and as a replayed three-step graph."""
    shape = st.SHAPES[4]
    n = int(np.prod(shape))
    b = _long_buffers(kernel, shape, N_LONG)
    eps = torch.zeros_like(b["eps_all"][0])
    traj = [torch.zeros(N_LONG, n, device=DEV) for _ in range(2)]
    for auto in (True, False):
        _reset(b)
        ctx.step_autoadvance(b["done"] if auto else None)
        try:
            for i in range(N_LONG):
                eps.copy_(b["eps_all"][i])  # fresh eps, on the same stream
                _long_launch(ctx, kernel, b, eps, shape)
                if not auto:
                    ctx.advance_step(b["step"])
                traj[0 if auto else 1][i].copy_(b["x"])
        finally:
            ctx.step_autoadvance(None)
        torch.cuda.synchronize()
        assert int(b["step"].item()) == N_LONG and int(b["done"].item()) == 0, auto
    assert bool(torch.isfinite(traj[1]).all()) and float(traj[1][-1].abs().max()) > 0
    assert not torch.equal(traj[1][-1], traj[1][-2])
    assert torch.equal(_bits(traj[0]), _bits(traj[1]))
    del traj

    # the same loop as a captured graph of three steps, replayed; eager: the same twelve launches
    replays = 4
    _reset(b)
    ctx.step_autoadvance(b["done"])
    try:
        for i in range(3 * replays):
            _long_launch(ctx, kernel, b, b["eps_all"][i % 3], shape)
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    eager = _state(b)
    assert int(b["step"].item()) == 3 * replays and int(b["done"].item()) == 0
    _reset(b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.graph_begin()
        ctx.step_autoadvance(b["done"])
        try:
            for i in range(3):
                _long_launch(ctx, kernel, b, b["eps_all"][i], shape)
        finally:
            ctx.step_autoadvance(None)
            g = ctx.graph_end()
        for _ in range(replays):
            ctx.graph_launch(g)
    s.synchronize()
    torch.cuda.synchronize()
    try:
        assert int(b["step"].item()) == 3 * replays and int(b["done"].item()) == 0
        for got, want in zip(_state(b), eager):
            assert torch.equal(got, want)
    finally:
        ctx.graph_destroy(g)


# ------------------------------------------------------------------------------ chains against the CPU sampler oracles
def _chain_on_device(ctx, case):
    kind, shape, S, eta, guided = case
    B, C, H, W = shape
    hw, n = H * W, int(np.prod(shape))
    x_T, cond, uncond, noise = st.chain_inputs(shape, S)
    ts, coefs, sig = st.kernel_tables(S, eta)
    G = n + 256
    halves = 2 if guided else 1
    x = Guarded(x_T, G)
    pred = Guarded(torch.zeros(shape), G)
    xin0 = _make_xin(halves * B * hw, C, n)
    xin0[:, :C] = _nhwc(x_T, B, C, hw).half().repeat(halves, 1)
    xin = Guarded(xin0, G)
    tab = Guarded(coefs, G)
    nz = Guarded(sig[:, None] * noise.reshape(S, n), G) if eta > 0 else None  # sigma_t * randn, fp32
    hist = Guarded(torch.zeros(3, n), G)
    step, done = Guarded(torch.zeros(1, dtype=torch.int32), 64), Guarded(torch.zeros(1, dtype=torch.int32), 64)
    eps = Guarded(torch.zeros(halves, *shape), G)
    cond_d, uncond_d = cond.to(DEV).double(), uncond.to(DEV).double()
    xin.snapshot()

    def model(t):
        """The synthetic denoiser on what the UNet would read: the fp16 stem input (fp64 on the device, rounded to the
        fp32 eps the kernel takes; both halves under guidance)."""
        tt = torch.full((B,), int(t), dtype=torch.long, device=DEV)
        for h in range(halves):
            lat = xin.live[h * B * hw:(h + 1) * B * hw, :C].reshape(B, hw, C).permute(0, 2, 1).reshape(shape).double()
            eps.live[h].copy_(st.eps_fn(lat, tt, cond_d if (h == 1 or not guided) else uncond_d))

    xs, preds = [], []
    evals = S + 1 if kind == "plms" else S
    ctx.step_autoadvance(done.live)
    try:
        for k in range(evals):
            tail = (pred.live, xin.live, LD, B, C, hw)
            if kind == "plms":
                model(ts[0] if k == 0 else ts[min(1, S - 1)] if k == 1 else ts[k - 1])
                ctx.plms_step(x.live, eps.live, tab.live, step.live, hist.live, *tail, st.CHAIN_SCALE, guided)
            else:
                model(ts[k])
                if guided:
                    ctx.ddim_step_cfg(x.live, eps.live, tab.live, nz and nz.live, step.live, *tail, st.CHAIN_SCALE)
                else:
                    ctx.ddim_step(x.live, eps.live, tab.live, nz and nz.live, step.live, *tail)
            if kind != "plms" or k > 0:
                xs.append(x.live.clone())
                preds.append(pred.live.clone())
    finally:
        ctx.step_autoadvance(None)
    torch.cuda.synchronize()
    assert int(step.live.item()) == evals and int(done.live.item()) == 0
    for b in (x, pred, xin, tab, hist, step, done, eps) + ((nz,) if nz else ()):
        assert b.guards_intact()
    assert torch.equal(_bits(xin.live[:, C:]), _bits(xin.live_before()[:, C:]))
    return x.live.clone(), xs, preds


@pytest.mark.parametrize("case", list(st.chain_cases()),
                         ids=lambda c: "%s-%s-S%d-eta%d-%s" % (c[0], _ids(c[1]), c[2], c[3], "cfg" if c[4] else "plain"))
def test_chain_with_a_synthetic_denoiser(ctx, case):
    got = _chain_on_device(ctx, case)
    ref = st.chain_oracle(case, torch.float64)
    assert len(got[1]) == len(ref[1]) == case[2]
    dev = st.chain_deviation(got, ref)
    print("chain %s: deviation / max|z| = %.3e (bound %.3e)" % (case, dev, st.CHAIN_TOL))
    assert dev <= st.CHAIN_TOL
