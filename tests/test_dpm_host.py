"""Host side of DPM-Solver++(2M): the logSNR grid and the coefficient table of upgpt_amd/schedule.py against the fp64
restatement of tests/dpm_ref.py, and that restatement against an analytic Gaussian model (the modelled project has no DPM
solver, so the reference is validated on a problem whose exact solution is known).  No device."""
import os
import re

import numpy as np
import pytest
import torch

import dpm_ref as R
from upgpt_amd import _lib, build, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACP64 = R.linear_alphas_cumprod()
ACP = torch.from_numpy(ACP64.astype(np.float32))  # the model's fp32 buffer
T = 1000


def _ulps(got32, want64):
    """|got - want| in units of the fp32 spacing at `want`."""
    want64 = np.asarray(want64, dtype=np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- grid
def test_logsnr_nodes_for_ten_steps():
    nodes = schedule.make_logsnr_timesteps(ACP, 10)
    assert nodes.tolist() == [0, 2, 11, 36, 103, 233, 413, 597, 757, 888, 999]
    assert nodes.tolist() == R.logsnr_nodes(ACP64, 10).tolist()


def test_logsnr_nodes_are_strictly_increasing_between_the_ends():
    for S in range(1, 201):
        nodes = schedule.make_logsnr_timesteps(ACP, S)
        assert nodes.shape == (S + 1,) and nodes[0] == 0 and nodes[-1] == T - 1, S
        assert (np.diff(nodes) > 0).all(), S
        assert nodes.tolist() == R.logsnr_nodes(ACP64, S).tolist(), S


@pytest.mark.parametrize("S", [0, -3, T, T + 5])
def test_logsnr_nodes_refuse_what_does_not_fit(S):
    with pytest.raises(ValueError):
        schedule.make_logsnr_timesteps(ACP, S)


def test_uniform_grid_is_untouched():
    assert schedule.make_ddim_timesteps("uniform", 50, T, verbose=False).tolist() == R.uniform_timesteps(50).tolist()


# --------------------------------------------------------------------------------------------------------------- table
def _tables(S, grid="logsnr"):
    ts = R.logsnr_nodes(ACP64, S)[1:] if grid == "logsnr" else R.uniform_timesteps(S)
    return R.tables(ACP64, ts)


@pytest.mark.parametrize("S,grid,order,lof", [(6, "logsnr", 2, None), (16, "logsnr", 2, None), (20, "logsnr", 2, True),
                                               (10, "uniform", 2, False), (12, "logsnr", 1, None), (1, "logsnr", 2, None)])
def test_table_is_the_fp64_reference_rounded_once(S, grid, order, lof):
    a_t, a_p = _tables(S, grid)
    got = schedule.dpm_coefficient_table(torch.from_numpy(a_t).float(), a_p, order=order, lower_order_final=lof)
    want = R.coefficient_table(a_t, a_p, order=order, lower_order_final=lof)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, 8)
    # rounded once: within HALF an fp32 spacing of the fp64 value (+ 1e-6 for the last fp64 bit of log / expm1, which
    # numpy's vector and scalar paths need not share); a table built in fp32 misses this by whole spacings
    assert (_ulps(got.numpy(), want)[want != 0] <= 0.5 + 1e-6).all()
    assert (got.numpy()[want == 0] == 0).all()
    assert (got[:, 5:] == 0).all()


@pytest.mark.parametrize("S", [6, 16, 50])
def test_first_order_row_is_the_ddim_update(S):
    """x_p = sqrt(a_p) x0 + sqrt(1 - a_p) eps with x0 = (x - sigma_t eps) / alpha_t, written in (x, x0):
    x_p = (sigma_p / sigma_t) x + (alpha_p - sigma_p / sigma_t alpha_t) x0."""
    a_t, a_p = _tables(S)
    got = schedule.dpm_coefficient_table(a_t, a_p, order=1).numpy()
    a_t, a_p = a_t[::-1], a_p[::-1]
    c2 = np.sqrt(1 - a_p) / np.sqrt(1 - a_t)
    c3 = np.sqrt(a_p) - c2 * np.sqrt(a_t)
    assert (_ulps(got[:, 2], c2) <= 4).all()
    assert (_ulps(got[:, 3], c3) <= 4).all()
    assert (got[:, 4] == 0).all()


def test_first_order_rows():
    for S in (1, 2, 6, 14, 15, 16, 40):
        a_t, a_p = _tables(S)
        w = schedule.dpm_coefficient_table(a_t, a_p)[:, 4].numpy()
        assert w[0] == 0, S
        assert (w[1:-1] > 0).all(), S
        if S > 1:
            assert (w[-1] == 0) == (S < 15), S
        assert (schedule.dpm_coefficient_table(a_t, a_p, order=1)[:, 4] == 0).all()
        assert schedule.dpm_coefficient_table(a_t, a_p, lower_order_final=True)[-1, 4] == 0
        if S > 1:
            assert schedule.dpm_coefficient_table(a_t, a_p, lower_order_final=False)[-1, 4] > 0
    with pytest.raises(ValueError):
        schedule.dpm_coefficient_table(a_t, a_p, order=3)


# ------------------------------------------------------------------------------------------------------ analytic model
@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_reference_chain_on_the_gaussian_model(s2):
    err = lambda solver, grid, S: R.gaussian_error(ACP64, s2, solver, grid, S)
    ddim50 = err("ddim", "uniform", 50)
    e12, e20, e25, e50 = (err("2m", "logsnr", S) for S in (12, 20, 25, 50))
    print("s2 = %g: DDIM/50 %.3e; 2M logSNR 12 / 20 / 25 / 50: %.3e %.3e %.3e %.3e" % (s2, ddim50, e12, e20, e25, e50))
    assert e20 <= ddim50 / 3
    assert e12 < ddim50
    assert e25 / e50 >= 3  # second order: (50 / 25)^2 = 4 in the limit


def test_reference_launch_is_first_order_without_reading_the_history():
    rng = np.random.default_rng(0)
    x, e = rng.standard_normal((2, 4, 3, 5)), rng.standard_normal((2, 4, 3, 5))
    tab = R.coefficient_table(*_tables(6)).astype(np.float32)
    nan = np.full(x.shape, np.nan)
    for st, first in ((0, 0), (5, 0), (2, 2)):
        r = R.step(x, e, tab, st, nan, first_row=first)
        assert not r.second and np.isfinite(r.x).all() and np.isfinite(r.p0).all()
    r = R.step(x, e, tab, 2, np.zeros_like(x))
    assert r.second and not np.allclose(r.x, R.step(x, e, tab, 2, np.zeros_like(x), first_row=2).x)


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_header_binding_and_source():
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    declared = set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    assert "upk_dpmpp_2m_step_f32" in declared and "upk_dpmpp_2m_step_f32" in _lib.SYMBOLS
    assert "dpm.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "dpm.hip"))
    fn = _lib.load_library().upk_dpmpp_2m_step_f32
    assert len(fn.argtypes) == 16  # ctx + 15 (include/upk.h)
    assert hasattr(_lib.Context, "dpmpp_2m_step")


def test_alias_and_surface():
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from upgpt_amd import dpm_solver
    from upgpt_amd.ddim import DDIMSampler
    assert DPMSolverSampler is dpm_solver.DPMSolverSampler and issubclass(DPMSolverSampler, DDIMSampler)
    import inspect
    p = inspect.signature(DPMSolverSampler.sample).parameters
    assert p["order"].default == 2 and p["discretize"].default == "logsnr" and p["lower_order_final"].default is None
    base = inspect.signature(DDIMSampler.sample).parameters
    assert [k for k in base if k != "kwargs"] == [k for k in p if k not in ("order", "discretize", "lower_order_final", "kwargs")]
