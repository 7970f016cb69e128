"""Host side of UniPC: the coefficient table of upgpt_amd/schedule.py against the fp64 restatement of tests/unipc_ref.py,
that restatement's table-driven chain against the paper's own form and against DPM-Solver++(2M) (tests/dpm_ref.py), the
solver on the analytic Gaussian model (the modelled project has no UniPC, so the reference is validated on a problem whose
exact solution is known), and the ABI / engine / sampler surfaces that need no device."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import dpm_ref as D
import unipc_ref as R
from upgpt_amd import _lib, build, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACP64 = R.linear_alphas_cumprod()


def _ulps(got32, want64):
    """|got - want| in units of the fp32 spacing at `want`."""
    want64 = np.asarray(want64, dtype=np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


def _tables(S, grid="logsnr"):
    ts = R.logsnr_nodes(ACP64, S)[1:] if grid == "logsnr" else D.uniform_timesteps(S)
    return R.tables(ACP64, ts)


# --------------------------------------------------------------------------------------------------------------- table
@pytest.mark.parametrize("S,grid,kw", [
    (6, "logsnr", dict(order=3)), (6, "logsnr", dict(order=2)), (12, "logsnr", dict(order=3, variant="bh1")),
    (20, "logsnr", dict(order=2, variant="bh1")), (15, "logsnr", dict(order=3, lower_order_final=False)),
    (10, "uniform", dict(order=3)), (12, "logsnr", dict(order=1)), (12, "logsnr", dict(order=2, corrector=False)),
    (6, "logsnr", dict(order=3, start=2)), (1, "logsnr", dict(order=3)), (2, "logsnr", dict(order=3))])
def test_table_is_the_fp64_reference_rounded_once(S, grid, kw):
    a_t, a_p = _tables(S, grid)
    got = schedule.unipc_coefficient_table(torch.from_numpy(a_t).float(), a_p, **kw)
    want = R.coefficient_table(a_t, a_p, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S - kw.get("start", 0), 12)
    # rounded once: within HALF an fp32 spacing of the fp64 value (+ 1e-6: the two sides need not share the last fp64
    # bit of log / expm1 / the 3x3 solve); a table built in fp32 misses this by whole spacings
    assert (_ulps(got.numpy(), want)[want != 0] <= 0.5 + 1e-6).all()
    assert (got.numpy()[want == 0] == 0).all()


def test_rows_say_which_operands_exist():
    """S = 6, order 3: (corrector order, predictor order) per row = (0,1) (1,2) (2,3) (3,3) (3,2) (2,1)."""
    t = schedule.unipc_coefficient_table(*_tables(6), order=3).numpy()
    nz = lambda r: [bool(v != 0) for v in r]
    want = [(0, 1), (1, 2), (2, 3), (3, 3), (3, 2), (2, 1)]
    for row, (c, p) in zip(t, want):
        assert row[11] == (1.0 if c else 0.0)
        assert nz(row[2:5]) == [c > 0] * 3 and nz(row[5:7]) == [c > 1, c > 2]
        assert nz(row[9:11]) == [p > 1, p > 2]
    # the closed forms: UniC-1's own weight and UniP-2's are -alpha B(h) / 2 and -alpha B(h) / (2 r_1)
    al, sg, lam = R._points(*_tables(6))
    assert _ulps(t[1, 4], -al[1] * np.expm1(-(lam[1] - lam[0])) * 0.5) <= 0.5 + 1e-6
    h = lam[2] - lam[1]
    assert _ulps(t[1, 9], -al[2] * np.expm1(-h) * 0.5 / ((lam[0] - lam[1]) / h)) <= 0.5 + 1e-6
    off = schedule.unipc_coefficient_table(*_tables(6), order=3, corrector=False).numpy()
    assert (off[:, 2:7] == 0).all() and (off[:, 11] == 0).all() and np.array_equal(off[:, 7:11], t[:, 7:11])
    full = schedule.unipc_coefficient_table(*_tables(6), order=3, lower_order_final=False).numpy()
    assert nz(full[5, 9:11]) == [True, True] and nz(full[4, 9:11]) == [True, True]


@pytest.mark.parametrize("S", [6, 16, 50])
def test_order_one_without_corrector_is_the_ddim_update(S):
    """x_p = sqrt(a_p) x0 + sqrt(1 - a_p) eps with x0 = (x - sigma_t eps) / alpha_t, written in (x, x0):
    x_p = (sigma_p / sigma_t) x + (alpha_p - sigma_p / sigma_t alpha_t) x0."""
    a_t, a_p = _tables(S)
    got = schedule.unipc_coefficient_table(a_t, a_p, order=1, corrector=False).numpy()
    a_t, a_p = a_t[::-1], a_p[::-1]
    c7 = np.sqrt(1 - a_p) / np.sqrt(1 - a_t)
    c8 = np.sqrt(a_p) - c7 * np.sqrt(a_t)
    assert (_ulps(got[:, 0], np.sqrt(1 - a_t)) <= 0.5 + 1e-6).all() and (_ulps(got[:, 1], 1 / np.sqrt(a_t)) <= 0.5 + 1e-6).all()
    assert (_ulps(got[:, 7], c7) <= 4).all()
    assert (_ulps(got[:, 8], c8) <= 4).all()
    assert (got[:, 2:7] == 0).all() and (got[:, 9:] == 0).all()


@pytest.mark.parametrize("start", [1, 2, 5])
def test_a_chain_that_starts_inside_the_schedule_has_no_history(start):
    a_t, a_p = _tables(6)
    t = schedule.unipc_coefficient_table(a_t, a_p, order=3, start=start).numpy()
    full = schedule.unipc_coefficient_table(a_t, a_p, order=3).numpy()
    assert t.shape == (6 - start, 12)
    assert t[0, 11] == 0 and (t[0, 2:7] == 0).all() and (t[0, 9:11] == 0).all()  # no corrector, first-order predictor
    assert np.array_equal(t[0, [0, 1, 7, 8]], full[start, [0, 1, 7, 8]])
    if t.shape[0] > 1:
        assert t[1, 11] == 1 and t[1, 5] == 0  # corrector of order 1
    if start <= 2:  # from its fourth row on the chain has its full history
        assert np.array_equal(t[3:], full[start + 3:])


def test_bad_arguments():
    a_t, a_p = _tables(6)
    for order in (0, 4, 2.5, None):
        with pytest.raises(ValueError):
            schedule.unipc_coefficient_table(a_t, a_p, order=order)
    with pytest.raises(ValueError):
        schedule.unipc_coefficient_table(a_t, a_p, variant="vary_coeff")
    for start in (-1, 6):
        with pytest.raises(ValueError):
            schedule.unipc_coefficient_table(a_t, a_p, start=start)
    with pytest.raises(ValueError):
        schedule.unipc_coefficient_table(a_t[::-1], a_p[::-1])  # lambda must ascend along the chain


# ----------------------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("kw", [dict(order=1), dict(order=2), dict(order=3), dict(order=3, variant="bh1"),
                                dict(order=3, lower_order_final=False), dict(order=3, corrector=False), dict(order=3, start=2)])
def test_table_chain_is_the_papers_chain(kw):
    """The folded weights against the update written with D_i / r_i and rho, on a nonlinear vector model."""
    S = 9
    ts = R.logsnr_nodes(ACP64, S)[1:]
    a_t, a_p = R.tables(ACP64, ts)
    rng = np.random.default_rng(1)
    x_T, W = rng.standard_normal(7), 0.3 * rng.standard_normal((7, 7))
    model = lambda x, t, i: np.tanh(W @ x) * np.sqrt(1 - ACP64[t]) + 0.1 * x
    want, xs_w, ms_w = R.paper_chain(model, x_T, a_t, a_p, ts[::-1], **kw)
    start = kw.get("start", 0)
    got, xs, ms = R.chain(model, x_T, ts[::-1][start:], R.coefficient_table(a_t, a_p, **kw))
    assert len(xs) == len(xs_w) == S - start
    for u, v in zip(xs + ms, xs_w + ms_w):
        assert np.abs(u - v).max() <= 1e-12 * max(1.0, np.abs(v).max())


@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_predictor_of_order_two_is_dpmpp_2m(s2):
    """UniP-2 with B(h) = expm1(-h) and rho = 1/2 is DPM-Solver++(2M): the same final latent on the Gaussian model."""
    S = 12
    ts = R.logsnr_nodes(ACP64, S)[1:]
    a_t, a_p = R.tables(ACP64, ts)
    model, x_T = R.gaussian_eps(ACP64, s2), np.asarray([1.0])
    tab = schedule.unipc_coefficient_table(a_t, a_p, order=2, corrector=False, variant="bh2").numpy().astype(np.float64)
    tab64 = R.coefficient_table(a_t, a_p, order=2, corrector=False, variant="bh2")
    assert np.abs(tab - tab64).max() <= 2.0 ** -23 * np.abs(tab64).max()
    got = R.chain(model, x_T, ts[::-1], tab64)[0]
    want = D.chain(model, x_T, ts[::-1], D.coefficient_table(a_t, a_p, order=2, lower_order_final=True))[0]
    assert abs(got[0] - want[0]) <= 1e-10 * abs(want[0])
    assert abs(R.gaussian_error(ACP64, s2, S, 2, corrector=False) - D.gaussian_error(ACP64, s2, "2m", "logsnr", S)) < 1e-9


# what the fp64 experiment behind DESIGN.md 41 gave, two digits: rows (order, S), columns s^2 = 0.25, 1, 4
TABLE = {(2, 12): (8.2e-3, 9.6e-3, 9.8e-3), (2, 20): (2.1e-3, 2.3e-3, 2.3e-3), (2, 25): (8.7e-4, 1.1e-3, 1.2e-3),
         (2, 50): (1.4e-4, 8.2e-5, 1.4e-4), (3, 12): (3.9e-3, 1.1e-3, 6.6e-4), (3, 15): (6.6e-4, 2.6e-4, 9.4e-5)}


@pytest.mark.parametrize("col,s2", list(enumerate([0.25, 1.0, 4.0])))
def test_solver_on_the_gaussian_model(col, s2):
    err = {k: R.gaussian_error(ACP64, s2, k[1], k[0]) for k in TABLE}
    m2 = {S: D.gaussian_error(ACP64, s2, "2m", "logsnr", S) for S in (12, 20, 50)}
    print("s2 = %g: UniPC (order, S) %s; 2M %s" % (s2, {k: "%.2e" % v for k, v in err.items()}, {k: "%.2e" % v for k, v in m2.items()}))
    for k, v in err.items():  # the recorded table, to its two digits
        assert abs(v - TABLE[k][col]) <= 0.06 * TABLE[k][col], (k, v)
        assert abs(v - R.gaussian_error(ACP64, s2, k[1], k[0], paper=True)) <= 1e-9 * v + 1e-13
    assert err[(2, 12)] < m2[12]
    assert err[(2, 20)] <= m2[20] / 2
    assert err[(3, 15)] < m2[50]
    assert err[(2, 25)] / err[(2, 50)] >= 5


def test_reference_launch_reads_only_what_the_row_names():
    rng = np.random.default_rng(0)
    shape = (2, 4, 3, 5)
    x, e, xc = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    tab = R.coefficient_table(*_tables(6), order=3).astype(np.float32)
    want = [dict(x_corr=False, h0=False, h1=False, h2=False), dict(x_corr=True, h0=True, h1=False, h2=False),
            dict(x_corr=True, h0=True, h1=True, h2=False), dict(x_corr=True, h0=True, h1=True, h2=True),
            dict(x_corr=True, h0=True, h1=True, h2=True), dict(x_corr=True, h0=True, h1=True, h2=False)]
    for st in range(6):
        hist = rng.standard_normal((3,) + shape)
        s0, s1, s2 = R.slots(st)
        assert sorted((s0, s1, s2)) == [0, 1, 2]
        for name, slot in (("h0", s0), ("h1", s1), ("h2", s2)):
            if not want[st][name]:
                hist[slot] = np.nan
        r = R.step(x, e, tab, st, hist, xc if want[st]["x_corr"] else np.full(shape, np.nan))
        assert r.reads == want[st], st
        assert all(np.isfinite(v).all() for v in (r.x, r.xc, r.m, r.A["x"], r.A["xc"], r.A["m"])), st
        assert (np.abs(r.x) <= r.A["x"]).all() and (np.abs(r.xc) <= r.A["xc"]).all()
    assert np.array_equal(R.step(x, e, tab, 0).xc, x)


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_header_binding_and_source():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    declared = set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    assert "upk_unipc_step_f32" in declared and "upk_unipc_step_f32" in _lib.SYMBOLS
    assert "unipc.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "unipc.hip"))
    fn = _lib.load_library().upk_unipc_step_f32
    assert len(fn.argtypes) == 16  # ctx + 15 (include/upk.h)
    assert hasattr(_lib.Context, "unipc_step")


class _Plan:
    """What SamplerState reads of a sampler-mode UNetPlan, with host memory behind alloc()."""
    mode, B, H, W, rows = "sampler", 2, 4, 4, 6

    def alloc(self, *shape, dtype=torch.float16, zero=False):
        return torch.zeros(*shape, dtype=dtype)


def test_sampler_state_kind():
    from upgpt_amd.engine import SamplerState
    for cfg in (False, True):
        st = SamplerState(_Plan(), 4, "unipc", cfg=cfg)
        B = 1 if cfg else 2
        n = B * 4 * 4 * 4
        assert tuple(st.coefs.shape) == (6, 12) and st.coefs.dtype == torch.float32
        assert tuple(st.hist.shape) == (3, n) and tuple(st.x_corr.shape) == (n,) and st.x0_old is None
        assert st.hist.dtype == st.x_corr.dtype == torch.float32 and st.variant is None
        for v in ("plain", "masked", (0, False)):
            with pytest.raises(ValueError, match="no step variant"):
                st.set_variant(v)
        with pytest.raises(ValueError, match="eta = 0"):
            SamplerState._STEP["unipc"](st, 1234, 1.0)  # a noise table: refused before anything is read
    assert SamplerState(_Plan(), 4, "dpm").x_corr is None and tuple(SamplerState(_Plan(), 4, "dpm").coefs.shape) == (6, 8)


def test_alias_and_surface():
    from ldm.models.diffusion.uni_pc import UniPCSampler
    from upgpt_amd import unipc
    from upgpt_amd.ddim import DDIMSampler
    from upgpt_amd.dpm_solver import DPMSolverSampler
    assert UniPCSampler is unipc.UniPCSampler and issubclass(UniPCSampler, DDIMSampler)
    p = inspect.signature(UniPCSampler.sample).parameters
    own = dict(order=2, variant="bh2", corrector=True, lower_order_final=True, discretize="logsnr")
    assert {k: p[k].default for k in own} == own
    base = inspect.signature(DPMSolverSampler.sample).parameters
    assert [k for k in base if k not in own and k != "kwargs"] == [k for k in p if k not in own and k != "kwargs"]


def test_refusals_without_a_device():
    from upgpt_amd.unipc import UniPCSampler
    model = types.SimpleNamespace(num_timesteps=1000, parameterization="eps")
    s = UniPCSampler(model)
    cond = {"c_crossattn": torch.zeros(1, 1, 8)}
    with pytest.raises(ValueError, match="eta"):
        s.sample(6, 1, (4, 8, 8), cond, eta=0.5, verbose=False)
    with pytest.raises(ValueError, match="eta"):
        s.make_schedule(6, ddim_eta=1.0, verbose=False)
    with pytest.raises(NotImplementedError, match="dpmpp_2m"):
        s.sample(6, 1, (4, 8, 8), cond, mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8), verbose=False)
    with pytest.raises(NotImplementedError, match="dpmpp_2m"):
        s.unipc_sampling(cond, (1, 4, 8, 8), mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8))
    from upgpt_amd.inference import InferenceModel
    with pytest.raises(NotImplementedError, match="dpmpp_2m"):  # a region edit is a masked chain: refused before any upload
        InferenceModel.edit_region(None, np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8), "top", {}, sampler="unipc")
    with pytest.raises(NotImplementedError, match="eps"):
        UniPCSampler(types.SimpleNamespace(num_timesteps=1000, parameterization="x0")).sample(6, 1, (4, 8, 8), cond, verbose=False)
    model.alphas_cumprod = torch.from_numpy(ACP64.astype(np.float32))
    model.alphas_cumprod_prev = torch.cat([torch.ones(1), model.alphas_cumprod[:-1]])
    model.betas = 1 - model.alphas_cumprod / model.alphas_cumprod_prev
    model.device = torch.device("cpu")
    for bad in (dict(order=4), dict(order=0), dict(variant="bh3")):
        with pytest.raises(ValueError):
            s.make_schedule(6, verbose=False, **bad)
    s.make_schedule(6, verbose=False, order=3)
    assert s.ddim_timesteps.tolist() == R.logsnr_nodes(ACP64, 6)[1:].tolist()
    want = R.coefficient_table(*R.tables(ACP64, s.ddim_timesteps), order=3).astype(np.float32)
    assert np.array_equal(s.unipc_coefs.numpy(), want)
