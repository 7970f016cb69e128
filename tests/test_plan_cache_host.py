"""PlanCache (upgpt_amd/plancache.py) with fake plans: key tail, per-lane bound, hit / miss / invalid / failed build,
drop, the dict surface the tests and scripts read, and the two knobs that are read when called.  No device is touched:
`device` is None or a CPU device everywhere."""
import threading

import pytest
import torch

from upgpt_amd import _lib as L
from upgpt_amd import knobs
from upgpt_amd.plancache import PlanCache


class Closable:
    def __init__(self, head=None):
        self.head, self.closed = head, 0

    def close(self):
        self.closed += 1


class Bare:
    """A plan with no close() at all (the VAE's, LPIPS', FID's and the CLIP towers')."""

    def __init__(self, head=None):
        self.head = head


class Builder:
    def __init__(self, kind):
        self.kind, self.calls = kind, 0

    def __call__(self, head=None):
        def build():
            self.calls += 1
            return self.kind(head)
        return build


def get(cache, head, builder, **kw):
    with L.PLAN_LOCK:
        return cache.get(head, builder(head), None, **kw)


def test_key_tail_follows_lane_and_table():
    tuned, plain, b = PlanCache(4), PlanCache(4, tuned=False), Builder(Bare)
    get(tuned, ("live", 2), b)
    get(plain, (2, 64), b)
    with L.lane(3):
        get(tuned, ("live", 2), b)
        get(plain, (2, 64), b)
        with L.shared_chip(4):
            get(tuned, ("live", 2), b)
            get(plain, (2, 64), b)  # (the table is no part of an untuned plan's identity: a hit)
    with L.shared_chip(2):
        get(tuned, ("live", 2), b)
    assert list(tuned) == [("live", 2, False, 0), ("live", 2, False, 3), ("live", 2, True, 3), ("live", 2, True, 0)]
    assert list(plain) == [(2, 64, 0), (2, 64, 3)]
    assert b.calls == 6
    assert all(k[0] == "live" and k[1] == 2 for k in tuned) and [k[-1] for k in plain] == [0, 3]


def test_key_tail_is_the_calling_threads():
    cache, b = PlanCache(2), Builder(Bare)

    def worker():
        with L.lane(1, concurrency=2):
            get(cache, (7,), b)
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    get(cache, (7,), b)
    assert list(cache) == [(7, True, 1), (7, False, 0)]


@pytest.mark.parametrize("kind", [Closable, Bare])
@pytest.mark.parametrize("limit", [2, 4, 8])
def test_bound_is_per_lane_and_evicts_the_oldest(limit, kind):
    cache, b = PlanCache(limit), Builder(kind)
    built, other = [], []
    for i in range(limit + 1):
        built.append(get(cache, (i,), b))
        with L.lane(1):
            other.append(get(cache, (100 + i,), b))
            other.append(get(cache, (200 + i,), b))
        assert len([k for k in cache if k[-1] == 0]) == min(i + 1, limit)
    lane0 = [k for k in cache if k[-1] == 0]
    assert lane0 == [(i, False, 0) for i in range(1, limit + 1)]  # exactly `limit` left, the first one gone
    assert [cache[k] for k in lane0] == built[1:]
    if kind is Closable:
        assert [p.closed for p in built] == [1] + [0] * limit  # closed exactly once, nothing else closed
    # lane 1 evicted its own oldest only; what it still holds is unclosed, and lane 0 never touched it
    lane1 = [k for k in cache if k[-1] == 1]
    assert len(lane1) == limit and all(cache[k] in other for k in lane1)
    if kind is Closable:
        assert all(cache[k].closed == 0 for k in lane1)
        assert sum(p.closed for p in other) == len(other) - limit and max(p.closed for p in other) == 1


def test_hit_returns_the_same_object_without_building():
    cache, b = PlanCache(2), Builder(Closable)
    first = get(cache, (1, 2), b)
    assert get(cache, (1, 2), b) is first and get(cache, [1, 2], b) is first
    assert b.calls == 1 and first.closed == 0


def test_two_threads_one_missing_key_build_once():
    cache, b = PlanCache(2), Builder(Bare)
    go, got = threading.Barrier(2), []

    def worker():
        go.wait()
        got.append(get(cache, (5,), b))
    threads = [threading.Thread(target=worker) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert b.calls == 1 and got[0] is got[1] and len(cache) == 1


@pytest.mark.parametrize("kind", [Closable, Bare])
def test_invalid_entry_is_replaced_in_place_without_eviction(kind):
    cache, b = PlanCache(2), Builder(kind)
    a, c = get(cache, (1,), b), get(cache, (2,), b)  # the lane is at its bound
    assert get(cache, (1,), b, valid=lambda p: True) is a and b.calls == 2
    seen = []
    a2 = get(cache, (1,), b, valid=lambda p: seen.append(p) or False)
    assert seen == [a] and a2 is not a and b.calls == 3
    assert list(cache.items()) == [((1, False, 0), a2), ((2, False, 0), c)]  # same key, same place, nothing evicted
    if kind is Closable:
        assert c.closed == 0
    assert get(cache, (3,), b, valid=lambda p: False) is cache[(3, False, 0)]  # (a miss never asks `valid`)
    assert list(cache) == [(2, False, 0), (3, False, 0)]


def test_failed_build_leaves_the_key_absent():
    cache, b = PlanCache(2), Builder(Closable)
    with L.lane(1):
        theirs = [get(cache, (i,), b) for i in range(2)]
    mine = get(cache, (1,), b)

    def boom():
        raise ValueError("no such shape")
    with L.PLAN_LOCK, pytest.raises(ValueError, match="no such shape"):
        cache.get((9,), boom, None)
    assert (9, False, 0) not in cache
    assert list(cache.items()) == [((0, False, 1), theirs[0]), ((1, False, 1), theirs[1]), ((1, False, 0), mine)]
    assert [p.closed for p in theirs + [mine]] == [0, 0, 0]
    later = get(cache, (9,), b)
    assert cache[(9, False, 0)] is later and b.calls == 4
    # at the bound the eviction is made once the cache has decided to build, and only that: the lane's oldest
    with L.PLAN_LOCK, pytest.raises(ValueError):
        cache.get((10,), boom, None)
    assert list(cache) == [(0, False, 1), (1, False, 1), (9, False, 0)] and mine.closed == 1 and later.closed == 0


def test_drop_closes_exactly_the_matching_entries():
    cache, b = PlanCache(8), Builder(Closable)
    live = [get(cache, ("live", i), b) for i in range(2)]
    ema = [get(cache, ("ema", i), b) for i in range(2)]
    bare = get(cache, ("ema", 9), Builder(Bare))  # (an entry without close() is dropped all the same)
    with L.lane(1):
        live.append(get(cache, ("live", 0), b))
    cache.drop(lambda k: k[0] == "ema", torch.device("cpu"))
    assert [p.closed for p in ema] == [1, 1] and [p.closed for p in live] == [0, 0, 0]
    assert bare not in cache.values() and [k[0] for k in cache] == ["live"] * 3
    cache.drop(lambda k: k[0] == "ema")  # nothing matches: nothing happens
    assert [p.closed for p in ema + live] == [1, 1, 0, 0, 0]
    cache.drop()
    assert len(cache) == 0 and cache == {} and [p.closed for p in ema + live] == [1, 1, 1, 1, 1]
    cache.drop()


def test_it_is_a_dict():
    cache, b = PlanCache(4), Builder(Closable)
    plans = [get(cache, ("live", i), b) for i in range(3)]
    assert isinstance(cache, dict) and len(cache) == 3
    assert list(cache.values()) == plans
    assert list(cache.items()) == [(("live", i, False, 0), plans[i]) for i in range(3)]
    assert next(iter(cache.values())) is plans[0]
    assert cache.pop(("live", 1, False, 0)) is plans[1] and plans[1].closed == 0  # (pop is dict's: the caller closes)
    assert list(cache) == [("live", 0, False, 0), ("live", 2, False, 0)]
    cache.clear()
    assert len(cache) == 0 and not cache and [p.closed for p in plans] == [0, 0, 0]
    assert get(cache, ("live", 0), b) is not plans[0]


def test_knobs_are_read_when_called(monkeypatch):
    monkeypatch.delenv("UPGPT_LANES_TUNING", raising=False)
    monkeypatch.delenv("UPGPT_AUTOTUNE", raising=False)
    assert knobs.lanes_tuning() is True and knobs.autotune_missing() is False
    monkeypatch.setenv("UPGPT_LANES_TUNING", "0")
    monkeypatch.setenv("UPGPT_AUTOTUNE", "1")
    assert knobs.lanes_tuning() is False and knobs.autotune_missing() is True
    monkeypatch.setenv("UPGPT_AUTOTUNE", "0")
    monkeypatch.delenv("UPGPT_LANES_TUNING")
    assert knobs.lanes_tuning() is True and knobs.autotune_missing() is False
