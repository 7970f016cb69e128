"""The stage-isolating operands of tests/range_ref.py (cross_probe, head_probe, mlp_probe) have teeth (CPU only): at every
shape of the instantiation table ROW_CHAIN the faithful fp32 emulations of tests/test_dynamic_range_host.py pass each
stage's own bound, five seeded defects exceed it, and three of those five pass the chained bound of the full-chain
references, which is why the stage tests exist."""
import functools

import pytest
import torch
import torch.nn.functional as F

import range_ref as R
from test_dynamic_range_host import _emulate_groupnorm, emulate_cross, emulate_head, emulate_mlp

XSHAPES = sorted({(row["c"], row["dh"], row["d"], B, hw) for row in R.ROW_CHAIN if row["kind"] == "xblock"
                  for B, hw, _ in R.row_chain_shapes(row)})
HSHAPES = sorted({(B, hw) for row in R.ROW_CHAIN if row["kind"] == "hblock" for B, hw, _ in R.row_chain_shapes(row)})
MSHAPES = sorted({(B, hw, M) for row in R.ROW_CHAIN if row["kind"] == "mlp" for B, hw, M in R.row_chain_shapes(row)})


def xid(v):
    return "-".join(str(t) for t in v)


def test_the_table_lists_eighteen_distinct_instantiations():
    keys = [R.row_chain_key(r) for r in R.ROW_CHAIN]
    assert len(keys) == len(set(keys)) == 18
    assert len({R.row_chain_id(r) for r in R.ROW_CHAIN}) == 18
    assert sum(r["kind"] == "xblock" for r in R.ROW_CHAIN) == 6 and sum(r["kind"] == "hblock" for r in R.ROW_CHAIN) == 8
    assert sorted(R.mlp_rows_per_wg(r) for r in R.ROW_CHAIN if r["kind"] == "mlp") == [32, 64, 128, 64 | R.MLP_STREAM]
    for r in R.ROW_CHAIN:
        assert max(M for _, _, M in R.row_chain_shapes(r)) <= 512
        if r["kind"] == "xblock":
            assert R.HEADS * r["dh"] == r["c"]  # an identity to_out exists


def emulate_fold(o, **kw):
    """The GroupNorm fold: the normalised tile stored as fp16 (the statistics from fp32 sums), then the head."""
    B, hw, c = o["B"], o["hw"], o["c"]
    xn = _emulate_groupnorm(o["x"].reshape(B, hw, c), o["gn_groups"], o["gn_gamma"], o["gn_beta"], o["gn_eps"], False)
    return emulate_head(dict(o, x=xn.reshape(B * hw, c)), **kw)


def head_ratios(o, got):
    (t0, dt0), (qkv, dqkv) = R.head_probe_ref(o)
    assert float(t0.abs().max()) < 6e4 and float(qkv.abs().max()) < 6e4
    r0 = (0.0 if torch.equal(got[0].to(R.F64), t0) else float("inf")) if dt0 is None else R.ratio(got[0], t0, dt0)
    return r0, R.ratio(got[1], qkv, dqkv)


@functools.lru_cache(maxsize=None)
def hidden(s, B, hw, M):
    o = R.mlp_probe("M3", s, B, hw, 32, M=M if not hw else None)
    return R.mlp_hidden_ref(o)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", XSHAPES, ids=xid)
def test_faithful_cross_emulation_passes_every_probe(shape):
    c, dh, dp, B, hw = shape
    top = {}

    def run(probe, s, nkv, ks=1):
        o = R.cross_probe(probe, s, B, hw, nkv, c, dh, dp, ks)
        ref, bound = R.cross_probe_ref(o)
        assert float(ref.abs().max()) < 6e4
        r = R.ratio(emulate_cross(o), ref, bound)
        top[probe] = max(top.get(probe, 0.0), r)
        assert r <= 1, (probe, s, nkv, ks, r)
        return o, ref, bound

    for s in R.STAGE_SCALES:
        run("X1", s, 87)
        run("X3", s, 87)
        for nkv in R.X2_NKV:
            for ks in R.X2_KEY_SCALES:
                o, ref, bound = run("X2", s, nkv, ks)
                if nkv == 1:  # a single key: the value row itself
                    v = o["v"].to(R.F64).reshape(B, 1, c).expand(B, hw, c).reshape(B * hw, c)
                    assert torch.equal(ref, v + o["t0"].to(R.F64))
    for s in R.SCALES:
        run("X4", s, 87)
    print("cross %s: %s" % (xid(shape), "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))


@pytest.mark.parametrize("shape", HSHAPES, ids=xid)
def test_faithful_head_emulation_passes_every_probe(shape):
    B, hw = shape
    for probe, scales in (("H1", R.SCALES), ("H2", R.STAGE_SCALES), ("F1", R.STAGE_SCALES), ("F2", R.STAGE_SCALES)):
        for s in scales:
            o = R.head_probe(probe, s, B, hw)
            r0, r1 = head_ratios(o, (emulate_fold if probe[0] == "F" else emulate_head)(o))
            assert r0 <= 1 and r1 <= 1, (probe, s, r0, r1)


@pytest.mark.parametrize("shape", MSHAPES, ids=xid)
def test_faithful_mlp_emulation_passes_every_probe(shape):
    B, hw, M = shape
    for probe, scales in [("M1", R.STAGE_SCALES), ("M3", R.SCALES)] + [("M2%d" % j, R.STAGE_SCALES) for j in range(4)]:
        for s in scales:
            o = R.mlp_probe(probe, s, B, hw, 32, M=M if not hw else None)
            ref, bound = R.mlp_probe_ref(o, hidden(s, B, hw, M) if probe.startswith("M2") else None)
            assert float(ref.abs().max()) < 6e4
            r = R.ratio(emulate_mlp(o), ref, bound)
            assert r <= 1, (probe, s, r)
            if probe.startswith("M2"):
                assert float(ref.abs().max()) > 1  # (the hidden tile is not a row of zeros)


# ---------------------------------------------------------------------------------------------------------------------
# defects
def drop_last_key(o):
    """The key mask off by one: the last context key takes no part."""
    return dict(o, nkv=o["nkv"] - 1, k=o["k"][:, :-1], v=o["v"][:, :-1])


def wrong_sample(o):
    """Sample 1 attends to sample 0's K / V."""
    return dict(o, k=o["k"][[0, 0]], v=o["v"][[0, 0]])


def tanh_gelu(g):
    return F.gelu(g, approximate="tanh")


@pytest.mark.parametrize("c,dh,dp", [(224, 28, 32), (448, 56, 64)])
def test_attention_defects_exceed_the_stage_bound(c, dh, dp):
    for B, hw in ((2, 16), (2, 64)):
        for s in R.STAGE_SCALES:
            for ks in R.X2_KEY_SCALES:
                for nkv in R.X2_NKV:
                    o = R.cross_probe("X2", s, B, hw, nkv, c, dh, dp, ks)
                    ref, bound = R.cross_probe_ref(o)
                    assert R.ratio(emulate_cross(wrong_sample(o)), ref, bound) > 1, ("sample", s, ks, nkv)
                    if nkv > 1:
                        assert R.ratio(emulate_cross(drop_last_key(o)), ref, bound) > 1, ("mask", s, ks, nkv)


def test_mlp_defects_exceed_the_stage_bound():
    for B, hw, M in ((2, 32, 64), (1, 0, 72)):
        for s in R.STAGE_SCALES:
            for j in range(4):
                o = R.mlp_probe("M2%d" % j, s, B, hw, 32, M=M if not hw else None)
                ref, bound = R.mlp_probe_ref(o, hidden(s, B, hw, M))
                assert R.ratio(emulate_mlp(o, gelu=tanh_gelu), ref, bound) > 1, ("tanh", s, j)
                stale = R.ratio(emulate_mlp(o, stale_slice=True), ref, bound)
                # hidden columns 128..255 lie in the probes 0 (columns 0..223) and 1 (224..447)
                assert (stale > 1) if j < 2 else (stale <= 1), ("stale", s, j, stale)


def test_layernorm_statistics_defect_exceeds_the_stage_bound():
    for B, hw in ((2, 16), (2, 64)):
        for s in R.STAGE_SCALES:
            o = R.head_probe("H2", s, B, hw)
            r0, r1 = head_ratios(o, emulate_head(o, stat_cols=208))
            assert r0 == 0 and r1 > 1, (s, r0, r1)
            o = R.head_probe("F2", s, B, hw)
            assert head_ratios(o, emulate_fold(o, stat_cols=208))[1] > 1, s


def test_the_chained_bound_passes_three_of_the_defects():
    """Why the stage tests exist: under the chained bound of the full-chain references (a worst-case fp16 seam pushed
    through every later stage) a key mask that is off by one, a sample that attends to the other sample's context and a
    tanh GELU all pass.  Whoever sharpens the chained bound flips this test."""
    for c, dh, dp in ((224, 28, 32), (448, 56, 64)):
        for nkv in (16, 17, 80, 87, 96):
            o = R.cross_probe("X4", 1, 2, 64, nkv, c, dh, dp)
            ref, bound = R.cross_probe_ref(o)
            assert R.ratio(emulate_cross(o), ref, bound) <= 1
            r_mask, r_sample = (R.ratio(emulate_cross(f(o)), ref, bound) for f in (drop_last_key, wrong_sample))
            print("chained bound c %d n_kv %d: mask off by one %.3f, wrong sample %.3f" % (c, nkv, r_mask, r_sample))
            assert r_mask <= 1 and r_sample <= 1, (c, nkv, r_mask, r_sample)
    for s in R.SCALES:
        for name in R.MLP_CASES:
            o = R.mlp_case(name, s)
            ref, bound = R.mlp_case_ref(o)
            r = R.ratio(emulate_mlp(o, gelu=tanh_gelu), ref, bound)
            print("chained bound %s scale %g: tanh GELU %.3f" % (name, s, r))
            assert r <= 1, (name, s, r)
