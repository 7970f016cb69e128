"""PlanCache — the per-lane plan cache of every module (DESIGN.md "Plan caches").  A plan is the buffers, descriptors and
captured graphs built for one shape; the cache is a plain dict of them, key = head + (tuning table,) + (lane,)."""
import contextlib

import torch

from . import _lib


def _cuda(device):
    return device is not None and (isinstance(device, int) or torch.device(device).type == "cuda")


def _close(plan):
    close = getattr(plan, "close", None)
    if close is not None:
        close()


class PlanCache(dict):
    """limit: plans one lane holds at most (device memory of stale shapes; per lane, since another lane's plans may be
    executing).  tuned=False: the plans never call apply_tuning, so the table is no part of their identity."""

    def __init__(self, limit, tuned=True):
        super().__init__()
        self.limit, self.tuned = int(limit), bool(tuned)

    def get(self, head, build, device, valid=None):
        """The calling lane's plan for `head`, built by build() on a miss; call with _lib.PLAN_LOCK held.  valid(plan)
        false: the plan is rebuilt under its key (it does not count toward the bound: nothing is evicted for it)."""
        lane = _lib.current_lane()
        key = tuple(head) + ((_lib.concurrency() > 1,) if self.tuned else ()) + (lane,)
        plan = dict.get(self, key)
        if plan is not None and (valid is None or valid(plan)):
            return plan
        if plan is None:
            mine = [k for k in self if k[-1] == lane]
            if len(mine) >= self.limit:
                _close(self.pop(mine[0]))  # (the lane's oldest)
        with torch.cuda.device(device) if _cuda(device) else contextlib.nullcontext(), _lib.host_io():
            plan = build()  # (host_io: descriptor tables are uploaded from the host)
        self[key] = plan
        return plan

    def drop(self, pred=None, device=None):
        """Drops the plans whose key satisfies pred (all without one), e.g. those of a weight set that was repacked:
        the device is drained first (another lane may still be replaying their graphs or reading the old packed
        weights from its own stream), then each is closed, its captured graphs with it."""
        keys = [k for k in self if pred is None or pred(k)]
        if keys and _cuda(device):
            torch.cuda.synchronize(device)
        for k in keys:
            _close(self.pop(k))
