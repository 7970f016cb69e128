"""The attention variant table of tests/range_ref.py without a GPU: a plain-torch fp32 emulation of the kernels' TILED
algorithm passes attention_ref's bound on every row at every scale, seeded defects of the kind a reworked kernel could
have do not, both operand layouts decode to the same operands, and the launch geometry each row was sized for is what
the table says.  tests/test_attention_variants_gpu.py runs the same table on the kernels.

The emulation follows csrc/attention.hip: 64-key tiles while they are full and 32-key tiles for the rest (the LDS-staged
kernel: 64-key tiles only; the wide kernel and d > 128: 32-key tiles only), unscaled fp32 scores, a running maximum with
the accumulators rescaled by exp2((m_old - m_new) c) (exactly 1 for a row whose maximum did not move, so the kernels'
wave-uniform "only when it moved" is the same arithmetic), weights exp2(fma(s, c, -m c)) rounded to fp16, the denominator
the fp32 sum of the ROUNDED weights, masked scores -inf, keys past n_kv read from K row 0 and from the zero padding of
V^T, and for the causal mask the per-wave key range [0, min(n_kv, q0 + 16 qt))."""
import math

import numpy as np
import pytest
import torch

import range_ref as R

F64 = torch.float64
ROWS = R.attn_variant_rows()
GROUPS = sorted({(r["family"], r["d"]) for r in ROWS})


def tile_plan(family, d, end):
    """[(first key, keys)] of the tiles a wave walks over the keys [0, end)."""
    if family == "lds":
        return [(kb, 64) for kb in range(0, end, 64)]
    tiles, kb = [], 0
    if family != "wide" and d <= 128:
        while kb + 64 <= end:
            tiles.append((kb, 64))
            kb += 64
    while kb < end:
        tiles.append((kb, 32))
        kb += 32
    return tiles


def _wave(q, qi, k, v, nkv, tiles, cs, causal, defect):
    """q [..., r, d], k, v [..., nkv, d] fp32 holding fp16 values; qi [r]: the rows' query indices -> fp16 [..., r, d]."""
    lead, r = q.shape[:-2], q.shape[-2]
    m = torch.full((*lead, r, 1), float("-inf"))
    l = torch.zeros(*lead, r, 1)
    o = torch.zeros_like(q)
    kpad = max(nkv, max(kb + n for kb, n in tiles))
    vp = torch.zeros(*lead, kpad, v.shape[-1])
    vp[..., :nkv, :] = v
    for ti, (kb, n) in enumerate(tiles):
        keys = torch.arange(kb, kb + n)
        s = q @ k[..., torch.where(keys < nkv, keys, torch.zeros_like(keys)), :].transpose(-1, -2)
        dead = keys >= (nkv + 1 if defect == "admit_extra" else nkv)
        if defect == "drop_last":
            dead = dead | (keys == nkv - 1)
        dead = dead[None, :].expand(r, n)
        if causal:
            dead = dead | (keys[None, :] > qi[:, None] + (1 if defect == "causal_off" else 0))
        s = s.masked_fill(dead, float("-inf"))
        mnew = torch.maximum(m, s.max(-1, keepdim=True).values)
        if defect != "skip_rescale":
            alpha = torch.exp2((m - mnew) * cs)
            l, o = l * alpha, o * alpha
        m = mnew
        p = torch.exp2((s.double() * float(cs) + (-mnew * cs).double()).float()).half().float()  # (the fma rounds once)
        l = l + p.sum(-1, keepdim=True)
        vb = tiles[0][0] if (defect == "stale_v" and ti == 1) else kb
        o = o + p @ vp[..., vb:vb + n, :]
    return (o * (1.0 / l)).half()


def emulate(q, k, v, scale, family, d, causal=False, qt=1, defect=None):
    """q [B, h, nq, d], k, v [B, h, nkv, d] fp16 -> fp16 [B, h, nq, d]."""
    q, k, v = q.float(), k.float().clone(), v.float().clone()
    nq, nkv = q.shape[-2], k.shape[-2]
    if defect == "k_piece" and nkv > 1:  # one 8-half piece of one K row from the neighbouring row
        k[..., nkv // 2, 8:16] = k[..., nkv // 2 - 1, 8:16]
    if defect == "v_elem" and nkv > 1:  # one element of one value row from its neighbour
        v[..., nkv // 2, 3] = v[..., nkv // 2 - 1, 3]
    cs = np.float32(scale) * np.float32(1.4426950408889634)
    if not causal:
        return _wave(q, torch.arange(nq), k, v, nkv, tile_plan(family, d, nkv), cs, False, defect)
    out = torch.empty(q.shape, dtype=torch.float16)
    for q0 in range(0, nq, 16 * qt):
        qi = torch.arange(q0, min(nq, q0 + 16 * qt))
        out[..., q0:q0 + 16 * qt, :] = _wave(q[..., q0:q0 + 16 * qt, :], qi, k, v, nkv,
                                             tile_plan(family, d, min(nkv, q0 + 16 * qt)), cs, True, defect)
    return out


_CASES = {}


def case(row, s):
    """(q, k, v as [B, h, n, d] fp16, scale, ref, bound) of a row; the reference is computed once per (shape, scale)."""
    key = (row["family"], row["d"], row["nq"], row["nkv"], row["causal"], row["B"], row["heads"], row["variant"], s)
    if key not in _CASES:
        o = R.attn_variant_case(row, s)
        B, h = row["B"], row["heads"]
        if row["family"] == "qproj":
            d = lambda t: t.to(F64)
            dh, nq = o["dh"], o["nq"]
            wf, u, b = R._fold(o["w"], o["gamma"], o["beta"])
            qf, _ = R.linear_ref(d(o["x"]).reshape(B * nq, -1), wf, bias=d(b), ln=(o["eps"], d(u)))
            q = qf.half().reshape(B, nq, h, dh).transpose(1, 2)  # (the fp16 seam of q)
            k, v = o["k"].transpose(1, 2), o["v"].transpose(1, 2)
            ref, bound = R.qproj_case_ref(o)
        else:
            sp = lambda t, n: t.view(B, n, h, row["d"]).transpose(1, 2)
            q, k, v = sp(o["q"], row["nq"]), sp(o["k"], row["nkv"]), sp(o["v"], row["nkv"])
            ref, bound = R.attn_case_ref(o)
        _CASES[key] = (q, k, v, o["scale"], ref, bound)
    return _CASES[key]


def run(row, s, defect=None):
    q, k, v, scale, ref, bound = case(row, s)
    got = emulate(q, k, v, scale, row["family"], row["d"], row["causal"], row["qt"], defect)
    return R.ratio(got, ref, bound)


def test_the_table_names_every_variant_family_once_per_shape():
    names = {r["variant"] for r in ROWS}
    assert names == {"direct32q1", "direct32q2", "direct64q1", "direct64q2", "direct128q1", "direct128q2", "direct256",
                     "direct512", "lds32q1", "lds32q2", "lds64q1", "lds64q2", "wide512", "qproj32q2", "qproj64q1"}
    for fam, d in (("direct", 32), ("direct", 64), ("direct", 128)):
        for qt in (1, 2):
            assert any(r["causal"] for r in ROWS if (r["family"], r["d"], r["qt"]) == (fam, d, qt))
    for r in ROWS:  # preconditions of the paths (a row that broke one would be refused on the GPU)
        if r["family"] == "lds":
            assert r["nkv"] % 64 == 0 and r["nkv"] >= 256 and not r["causal"]
        if r["family"] == "wide":
            assert r["heads"] == 1 and r["nkv"] % 32 == 0 and r["d"] == 512


def test_launch_geometry_is_what_the_table_claims():
    """(workgroups, valid rows of the last live wave, idle waves) from n_q, the query groups per wave and the waves per
    workgroup the row was sized for, against the literal claims of the table."""
    for r in ROWS:
        rows = 16 * r["qt"]
        live = math.ceil(r["nq"] / rows)
        wgs = math.ceil(r["nq"] / (rows * r["w"]))
        assert (wgs, r["nq"] - (live - 1) * rows, wgs * r["w"] - live) == r["claim"], r
        assert r["w"] in r["wpbs"]
    ragged = [r for r in ROWS if not r["causal"] and r["family"] in ("direct", "qproj")]
    assert all(r["claim"][1] == 5 and r["claim"][0] >= 2 for r in ragged)
    assert any(r["claim"][2] > 0 for r in ragged)  # waves past the end
    # with two query groups per wave the 5 valid rows leave the second group wholly invalid
    assert all(r["claim"][1] <= 16 for r in ragged if r["qt"] == 2)
    assert {r["claim"] for r in ROWS if r["family"] == "lds"} == {(1, 7, 3), (2, 5, 2), (2, 21, 3)}


@pytest.mark.parametrize("layout", ["dense", "production"])
def test_layouts_decode_to_the_same_operands(layout):
    for row in (ROWS[1], next(r for r in ROWS if r["causal"] and r["nq"] == 77), next(r for r in ROWS if r["family"] == "wide")):
        o = R.attn_variant_case(row, 1)
        B, h, d, nq, nkv = row["B"], row["heads"], row["d"], row["nq"], row["nkv"]
        L = R.attn_layout(o["q"], o["k"], o["v"], h, d, nq, layout)
        q, k, v = R.attn_layout_decode(L, B, h, d)
        assert torch.equal(q, o["q"]) and torch.equal(k, o["k"]) and torch.equal(v, o["v"])
        rup = (nkv + 31) // 32 * 32
        vt = L["vt"]
        assert vt.shape[-1] == L["vt_ld"] >= rup and not vt[..., nkv:rup].any()
        assert L["vt_ld"] % 8 == 0 and L["ldq"] % 8 == 0 and L["ldk"] % 8 == 0 and L["ldo"] % 4 == 0
        assert R.attn_outside_untouched(L) and bool((R.attn_owned(L) == R.ATTN_FILL).all())
        if layout == "production":
            assert L["vt_ld"] == rup + 32 and bool(torch.isnan(vt[..., rup:]).all())  # NaN only where no kernel may read
            assert not torch.isnan(vt[..., :rup]).any()
            assert L["out_buf"].shape == (B, nq + 2, h * d + 8)
            assert (L["q"].data_ptr() == L["k"].data_ptr() - 2 * h * d) == (nq == nkv)
            R.attn_owned(L)[:] = 1.0
            assert R.attn_outside_untouched(L)
            L["out_buf"][0, nq, 0] = 1.0
            assert not R.attn_outside_untouched(L)
        else:
            assert L["vt_ld"] == rup


@pytest.mark.parametrize("family,d", GROUPS)
def test_tiled_emulation_passes_the_bound(family, d):
    top = 0.0
    for row in ROWS:
        if (row["family"], row["d"]) != (family, d):
            continue
        for s in R.ATTN_VARIANT_SCALES:
            r = run(row, s)
            top = max(top, r)
            assert r <= 1, (row, s, r)
    print("\ntiled emulation %s d=%d: largest ratio %.3f" % (family, d, top))
    assert top > 0


def _row(variant, nkv, causal=False):
    return max((r for r in ROWS if r["variant"] == variant and r["nkv"] == nkv and r["causal"] == causal),
               key=lambda r: r["nq"])


# (variant, n_kv) of the rows each defect is seeded into: every tile path that can show it
MULTI_TILE = [("direct64q1", 95), ("direct32q2", 160), ("direct256", 50), ("lds32q1", 256), ("lds64q2", 320), ("wide512", 96),
              ("qproj32q2", 87)]
TAIL = [("direct32q1", 33), ("direct64q1", 95), ("direct512", 50), ("qproj64q1", 87)]
CAUSAL = [("direct32q1", 17), ("direct64q2", 77), ("direct64q1", 150), ("direct128q1", 77)]
DEFECTS = {"drop_last": MULTI_TILE + TAIL, "admit_extra": TAIL, "stale_v": MULTI_TILE, "skip_rescale": MULTI_TILE,
           "k_piece": MULTI_TILE + TAIL, "v_elem": MULTI_TILE + TAIL}


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("defect", list(DEFECTS) + ["causal_off"])
def test_seeded_defects_exceed_the_bound(defect, s):
    low = float("inf")
    for variant, n in (CAUSAL if defect == "causal_off" else DEFECTS[defect]):
        row = _row(variant, n, defect == "causal_off")
        assert run(row, s) <= 1
        r = run(row, s, defect)
        low = min(low, r)
        assert r > 1, (defect, variant, n, s, r)
    print("\ndefect %-12s scale %-4g smallest ratio %.3g" % (defect, s, low))


@pytest.mark.parametrize("defect", ["stale_v", "skip_rescale", "causal_off"])
def test_seeded_defects_exceed_the_bound_at_near_one_hot_rows(defect):
    """s = 2^10: a dropped key is legitimately invisible there (its weight underflows), these three are not."""
    s = 2 ** 10
    for variant, n in (CAUSAL if defect == "causal_off" else MULTI_TILE):
        row = _row(variant, n, defect == "causal_off")
        r = run(row, s, defect)
        assert r > 1, (defect, variant, n, r)
