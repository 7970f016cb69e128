"""Rows per workgroup of the row-chain kernels (hblock / xblock, csrc/xblock.hip) with four forwards in flight, on one MI355X:
for every setting the captured UNet forward (8 x 32 x 32 latents, bbox UNet, 87 context tokens, real operands) of four lanes
is replayed concurrently; reported are the WALL time per forward and what the hblock and the xblock launches cost in chip time
(forward in flight minus the same forward without them, the method of lanes_ablate.py).  "default" first and last: their
spread is the noise figure of the session.  The list of settings is walked `cycles` times (the group costs are measured in
the first walk only), so that every setting is also seen next to a drifting clock.  Usage: row_chain_rows_lab.py [reps] [cycles]"""
import contextlib, ctypes as C, io, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import upgpt_amd
from upgpt_amd import _lib as L
from upgpt_amd import knobs, synth
from upgpt_amd.lanes import LanePool

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
CYCLES = int(sys.argv[2]) if len(sys.argv) > 2 else 1
LANES, B, H, W = 4, 8, 32, 32
with contextlib.redirect_stdout(io.StringIO()):
    model = upgpt_amd.build_model("bbox")
synth.fill_module_(model)
model = model.cuda()
unet = model.model.diffusion_model
inp = synth.synth_inputs(B, (H, W), 4, 87, 768, seed=0, text_only=True)
inp = {k: inp[k].cuda() for k in ("x_T", "c_concat", "c_crossattn")}


def lane_plan(i, stream):
    with L.lane(i, stream, concurrency=LANES):
        p = unet.plan(B, H, W, 87, 50, "sampler")
        p.load_x_nchw(inp["x_T"], 0, 0)
        p.load_x_nchw(inp["c_concat"], 4, p.cin_pad)
        p.load_context(inp["c_crossattn"])
        p.t_rows.copy_(torch.arange(981, 0, -20, dtype=torch.float32)[:50])
        p._t_rows_key = None
        p.prep.run()
    return p


def replay(plans, streams, skip_idx=()):
    """ms per forward (wall / (reps * lanes)), best of 5."""
    gs = []
    for p, s in zip(plans, streams):
        ctx = p.ctx
        with torch.cuda.stream(s):
            ctx._chk(ctx.lib.upk_graph_begin(ctx.h, s.cuda_stream))
            p.body.run(s.cuda_stream, skip_idx=skip_idx)
            g = C.c_void_p()
            ctx._chk(ctx.lib.upk_graph_end(ctx.h, s.cuda_stream, C.byref(g)))
        gs.append(g)
    torch.cuda.synchronize()
    for p, g, s in zip(plans, gs, streams):  # warm
        p.ctx._chk(p.lib.upk_graph_launch(p.hctx, g, s.cuda_stream))
    best = 1e9
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            for p, g, s in zip(plans, gs, streams):
                p.ctx._chk(p.lib.upk_graph_launch(p.hctx, g, s.cuda_stream))
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / (REPS * len(plans)) * 1e3)
    for p, g in zip(plans, gs):
        p.ctx.graph_destroy(g)
    return best


pool = LanePool(LANES)
streams = list(pool.streams)
SETS = (("default", {}), ("hblock 64  xblock 32", {"HB_ROWS": 64, "XB_ROWS": 32}), ("hblock 128 xblock 32", {"HB_ROWS": 128, "XB_ROWS": 32}),
        ("hblock 32  xblock 64", {"HB_ROWS": 32, "XB_ROWS": 64}), ("hblock 32  xblock 128", {"HB_ROWS": 32, "XB_ROWS": 128}),
        ("hblock 64  xblock 64", {"XB_ROWS": 64}), ("hblock 128 xblock 128", {"XB_ROWS": 128}),
        ("hblock 128 xblock 64", {"HB_ROWS": 128, "XB_ROWS": 64}), ("default again", {}))
if os.environ.get("LAB_SETS"):  # a subset by name, e.g. LAB_SETS="hblock 64  xblock 32,hblock 32  xblock 64" (default / default again stay)
    keep = set(os.environ["LAB_SETS"].split(","))
    SETS = tuple(x for x in SETS if not x[1] or x[0] in keep)
print("%-24s %14s %12s %12s   row-chain ops" % ("setting", "ms per forward", "hblock us", "xblock us"), flush=True)
for cycle in range(CYCLES):
    for name, kv in SETS[1 if cycle else 0:]:
        old = {k: getattr(knobs, k) for k in kv}
        for k, v in kv.items():
            setattr(knobs, k, v)
        for pl in list(unet._plans.values()):
            pl.close()
        unet._plans.clear()
        try:
            plans = [lane_plan(i, s) for i, s in enumerate(streams)]
            labels = plans[0].body.labels
            hb = frozenset(i for i, l in enumerate(labels) if l.startswith("hblock "))
            xb = frozenset(i for i, l in enumerate(labels) if l.startswith("xblock "))
            ms = replay(plans, streams)
            if cycle == 0:
                ms_h, ms_x = replay(plans, streams, hb), replay(plans, streams, xb)
                print("%-24s %14.3f %12.1f %12.1f   %s" % (name, ms, (ms - ms_h) * 1e3, (ms - ms_x) * 1e3,
                                                          sorted(set(labels[i] for i in hb | xb))), flush=True)
            else:
                print("%-24s %14.3f" % (name, ms), flush=True)
        finally:
            for k, v in old.items():
                setattr(knobs, k, v)
