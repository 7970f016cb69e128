"""The captured-chain driver the six samplers share (DDIM with its editing chains, PLMS, DDPM ancestral, DPM-Solver++(2M),
UniPC, SDE-DPM-Solver++(2M) with its editing chains):
how a chain's steps are grouped into graph launches, the loop that launches the groups and hands control back to the
sampler between them, the start latent, and the lock rule in front of the loop.  The four samplers of the
DDIM family observe a chain the same way, so their host work after a group is here too (run_observed); DDPM's differs
(it logs first and hands the callbacks the timestep and x) and stays in ancestral.py.  What stays with each sampler: its
tables and draws in front of the loop and the lock rule they need.
"""
import contextlib

import torch

from . import rng
from ._lib import host_io


def logged_at(T, log_every_t):
    """Which loop positions 0 .. T-1 of a chain are logged: the first one, and every log_every_t-th counted from the end
    (the reference's `index % log_every_t == 0 or index == total_steps - 1` with index = T - 1 - i).  None: nothing."""
    return lambda i: log_every_t is not None and ((T - 1 - i) % log_every_t == 0 or i == 0)


def group_sizes(first, total, steps_per_graph, watched, logged):
    """The graph launches of `total` steps at loop positions first .. first + total - 1, as step counts: up to
    `steps_per_graph` steps per launch, and a step the host looks at ends a launch — every step when `watched` (a
    callback runs after each), else the positions `logged(i)` names."""
    i, end = first, first + total
    while i < end:
        n = 1
        while n < steps_per_graph and i + n < end and not (watched or logged(i + n - 1)):
            n += 1
        yield n
        i += n


def run(st, total, steps_per_graph, watched, logged, with_noise, scale=1.0, first=0):
    """Launches the chain on `st` (an engine.SamplerState with its variant set) group by group and yields the loop position
    of each group's last step, for the sampler's host work there.  steps_per_graph: ddim.STEPS_PER_GRAPH as the caller
    reads it at call time; PLMS passes 1 and first=-1 (position -1 is the predictor evaluation of its first step)."""
    i = first
    for n in group_sizes(first, total, steps_per_graph, watched, logged):
        st.launch(with_noise, scale, n)
        i += n
        yield i - 1


def run_observed(st, first_latent, T, steps_per_graph, callback, img_callback, log_every_t, with_noise, scale=1.0,
                 first=0, plain=False):
    """run() with the host work the DDIM family shares (DDIM, PLMS, DPM-Solver++, UniPC) after each group that ends at loop
    position i >= 0: callback(i), img_callback(pred_x0, i), then x and pred_x0 logged where logged_at(T, log_every_t)
    says so.  Returns the intermediates, which start from `first_latent`.  plain: log st.x_plain (a masked DDIM chain:
    st.x already holds the blend for the next step, the reference logs the unblended value).  first=-1 with
    steps_per_graph=1 is PLMS: T + 1 single launches, nothing for the host at its predictor evaluation."""
    intermediates = {"x_inter": [first_latent], "pred_x0": [first_latent.clone()]}
    # (steps whose result the host looks at — callbacks, logged intermediates: ddim.py:139-147 — end a graph)
    watched = callback is not None or img_callback is not None
    logged = logged_at(T, log_every_t)
    for i in run(st, T - first, steps_per_graph, watched, logged, with_noise, scale, first):
        if i < 0:
            continue
        if callback:
            callback(i)
        if img_callback:
            img_callback(st.pred_x0.clone(), i)
        if logged(i):
            intermediates["x_inter"].append((st.x_plain if plain else st.x).clone())
            intermediates["pred_x0"].append(st.pred_x0.clone())
    return intermediates


def start_latent(x_T, noise_keys, shape, device, dtype=None):
    """x_T when given, else the keyed draw (rng.STREAM_XT, row 0), else one torch.randn from the device generator.
    dtype: what a given x_T is converted to (the captured chains keep fp32 state; the step-by-step paths take it as is)."""
    if x_T is not None:
        return x_T.to(device) if dtype is None else x_T.to(device, dtype)
    return torch.randn(shape, device=device) if noise_keys is None else rng.randn(noise_keys, shape, rng.STREAM_XT)


def on_host(*tensors):
    """Whether any of a call's inputs still has to be uploaded."""
    return any(t is not None and torch.is_tensor(t) and not t.is_cuda for t in tensors)


def upload_lock(take):
    """The context of a fast path's prelude (start latent, tables, draws, plan.prep.run()): host_io() when `take`, else
    nothing.  Uploads from the host never overlap another lane's graph capture (_lib.host_io); a call that uploads
    nothing takes no lock, which is what lets warm keyed calls of several lanes run side by side.  Each sampler states
    its own rule where it calls this; they differ on purpose:

      DDIM  fresh or on_host or (with_noise and not keyed)   # unkeyed step noise: S draws and row copies
      PLMS  fresh or on_host                                 # eta = 0: its discarded draws touch no table
      DPM   fresh or on_host or (x_T is None and not keyed)  # the only draw is x_T
      UniPC as DPM
      SDE-DPM as DDIM                                        # eta > 0 draws per step; keyed or eta = 0 draws into no table
      DDPM  always                                           # uploads its coefficient and temperature rows every call

    fresh: a timestep-row, coefficient or noise-scale table of this call differs from what the device holds."""
    return host_io() if take else contextlib.nullcontext()
