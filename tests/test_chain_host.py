"""The shared chain driver (upgpt_amd/chain.py) and engine.SamplerState's (kind, variant) check, the parts that need no GPU:
how a chain's steps are grouped into graph launches, for every combination of chain length, start position, steps per
graph, log interval and callbacks; and that a step variant or guidance a kind does not have is refused."""
import itertools

import pytest
import torch

from upgpt_amd import chain
from upgpt_amd.engine import SamplerState

TOTALS, FIRSTS, SPGS, LOGS = range(1, 21), (0, 3), (1, 2, 8), (None, 1, 3, 7, 1000)


def test_groups_cover_the_chain_end_at_every_logged_step_and_are_maximal():
    for total, first, spg, log_every_t, watched in itertools.product(TOTALS, FIRSTS, SPGS, LOGS, (False, True)):
        what = (total, first, spg, log_every_t, watched)
        end = first + total  # loop positions first .. end - 1 of a chain of `end` positions
        logged = chain.logged_at(end, log_every_t)
        groups = list(chain.group_sizes(first, total, spg, watched, logged))
        assert sum(groups) == total and min(groups) >= 1 and max(groups) <= spg, what
        if watched:
            assert groups == [1] * total, what
        ends = set(itertools.accumulate(groups, initial=first))  # the position after each group (and `first`)
        for i in range(first, end):
            if logged(i):
                assert i + 1 in ends, (what, i)  # a group ends immediately after every logged position
        pos = first
        for n in groups:
            pos += n
            if n < spg and not watched:  # maximal: a short group ends at a logged position or at the chain's end
                assert pos == end or logged(pos - 1), (what, pos)


def test_logged_positions_are_the_reference_rule():
    """index % log_every_t == 0 or index == total - 1 with index = T - 1 - i (ddim.py:139-147); None logs nothing."""
    for T, log_every_t in itertools.product(TOTALS, LOGS):
        logged = chain.logged_at(T, log_every_t)
        for i in range(T):
            index = T - 1 - i
            assert logged(i) == (log_every_t is not None and (index % log_every_t == 0 or index == T - 1))


@pytest.mark.parametrize("spg", [1, 2, 8, 16])
def test_the_full_ddpm_chain_groups_as_the_gpu_test_counts_them(spg):
    """tests/test_ddpm_gpu.py::test_bbox_full_chain_batch8: T = 1000, log_every_t = 1000 -> the first step alone (it is
    logged), then ceil(999 / spg) groups."""
    T = 1000
    groups = list(chain.group_sizes(0, T, spg, False, chain.logged_at(T, 1000)))
    assert groups[0] == 1 and sum(groups) == T and len(groups) == 1 + -(-999 // spg)


class _Launches:
    def __init__(self):
        self.calls = []

    def launch(self, with_noise, scale=1.0, nsteps=1):
        self.calls.append((with_noise, scale, nsteps))


def test_run_launches_each_group_and_yields_its_last_position():
    st, T = _Launches(), 11
    logged = chain.logged_at(T, 4)
    seen = list(chain.run(st, T, 8, False, logged, True, 3.0))
    sizes = list(chain.group_sizes(0, T, 8, False, logged))
    assert st.calls == [(True, 3.0, n) for n in sizes]
    assert seen == [p - 1 for p in itertools.accumulate(sizes)] and seen[-1] == T - 1
    # PLMS: one evaluation per launch from position -1 (the predictor evaluation), whatever is logged
    st = _Launches()
    assert list(chain.run(st, 5, 1, True, logged, False, first=-1)) == [-1, 0, 1, 2, 3]
    assert st.calls == [(False, 1.0, 1)] * 5


def test_start_latent_prefers_x_T_and_converts_only_on_request():
    x = torch.zeros(1, 2, 3, 4, dtype=torch.float64)
    assert chain.start_latent(x, None, x.shape, "cpu") is x
    assert chain.start_latent(x, None, x.shape, "cpu", torch.float32).dtype == torch.float32
    torch.manual_seed(3)
    a = chain.start_latent(None, None, (1, 2, 3, 4), "cpu")
    torch.manual_seed(3)
    assert torch.equal(a, torch.randn(1, 2, 3, 4))
    assert chain.on_host(None, x) and not chain.on_host(None, 3.0)


class _Plan:
    """What SamplerState reads of a sampler-mode UNetPlan, with host memory behind alloc()."""
    mode, B, H, W, rows = "sampler", 2, 4, 4, 3

    def alloc(self, *shape, dtype=torch.float16, zero=False):
        return torch.zeros(*shape, dtype=dtype)


def test_a_kind_refuses_variants_and_guidance_it_does_not_have():
    assert SamplerState(_Plan(), 4).kind == "ddim" and SamplerState(_Plan(), 4).variant is None
    for kind in ("plms", "dpm"):
        st = SamplerState(_Plan(), 4, kind, cfg=True)
        for v in ("plain", "masked", (0, False)):
            with pytest.raises(ValueError, match="no step variant"):
                st.set_variant(v)
        assert st.variant is None
    with pytest.raises(ValueError, match="no guidance"):
        SamplerState(_Plan(), 4, "ddpm", cfg=True)
    with pytest.raises(ValueError, match="kind must be one of"):
        SamplerState(_Plan(), 4, "euler")
    st = SamplerState(_Plan(), 4, "ddpm")
    assert st.variant == (0, False)
    st.set_variant((3, True))
    for v in (None, "masked", (0,), ("x0", True)):
        with pytest.raises(ValueError, match="no step variant"):
            st.set_variant(v)
    assert st.variant == (3, True)
    st = SamplerState(_Plan(), 4, "ddim")
    for v in (None, "plain", "masked"):
        st.set_variant(v)
    for v in ("edit", (0, False), True):
        with pytest.raises(ValueError, match="no step variant"):
            st.set_variant(v)
