"""Form and rows per workgroup of the fused feed-forward tail (csrc/mlp.hip) with four forwards in flight, on one MI355X:
row_chain_rows_lab.py's method for the third row-chain kernel.  For every setting the captured UNet forward (8 x 32 x 32
latents, bbox UNet, 87 context tokens, real operands) of four lanes is replayed concurrently; reported is the WALL time
per forward.  "default" (the shared-chip table as shipped) first and last: their spread is the noise figure of the
session; "two launches" is GEGLU + (ff.net.2 o proj_out) unfused, the table's answer before it held a tile height.
The list of settings is walked `cycles` times.  Usage: mlp_rows_lab.py [reps] [cycles]"""
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


def replay(plans, streams):
    """ms per forward (wall / (reps * lanes)), best of 5."""
    gs = []
    for p, s in zip(plans, streams):
        ctx = p.ctx
        with torch.cuda.stream(s):
            ctx._chk(ctx.lib.upk_graph_begin(ctx.h, s.cuda_stream))
            p.body.run(s.cuda_stream)
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
# (a forced tile height keeps the launch fused under the shared-chip table: Emitter.geglu_mlp)
SETS = (("default (table)", {}), ("two launches", {"MLP_FUSE": "0"}), ("resident 32", {"MLP_ROWS": 32}),
        ("resident 64", {"MLP_ROWS": 64}), ("streaming 64", {"MLP_ROWS": 64, "MLP_STREAM": True}),
        ("streaming 128", {"MLP_ROWS": 128}), ("default again", {}))
if os.environ.get("LAB_SETS"):  # a subset by name, e.g. LAB_SETS="two launches,streaming 128" (default / default again stay)
    keep = set(os.environ["LAB_SETS"].split(","))
    SETS = tuple(x for x in SETS if not x[1] or x[0] in keep)
print("%-18s %14s %9s   feed-forward ops of a 32x32-level block" % ("setting", "ms per forward", "launches"), flush=True)
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
            ms = replay(plans, streams)
            if cycle == 0:
                ff = sorted(set(l for l in labels if l.startswith("mlp ") or "geglu" in l.lower()))
                print("%-18s %14.3f %9d   %s" % (name, ms, len(labels), ff), flush=True)
            else:
                print("%-18s %14.3f" % (name, ms), flush=True)
        finally:
            for k, v in old.items():
                setattr(knobs, k, v)
