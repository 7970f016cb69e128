"""CPU checks of tests/norm_ref.py, the tables and bounds tests/test_norm_paths_gpu.py judges norm.hip with:

* the tables agree with themselves and with the library's chunking, and their data stays inside fp16 and inside
  |mu| / sigma <= 4 per group and per row at every scale used;
* every bound tells the algorithm from its near misses (a dropped pixel, a moved chunk boundary, a missing row slot, a
  seam-straddling group fed by one source, a neighbour's statistics, parameters shifted by a channel, a missing row
  block, swapped planes, a missing stride of the fold, a missing vector or a padded count in LayerNorm).  Statistics
  near misses are judged on the workspace, per chunk (a pixel in thousands is invisible in y); the others on y;
* the algorithm evaluated in fp32 in the kernels' summation order is inside every bound: the bounds are reachable.

The refill case is treated with ONE sample of its shape here (its chunks and row blocks are per sample)."""
import pytest
import torch

import norm_ref as N
import range_ref as R

F64 = torch.float64
d64 = lambda t: t.to(F64)
D = N.REFILL


def _gn_shapes():
    """name -> (c1, c2, hw, B, groups) of every GroupNorm case of the tables."""
    out = {k: v[:5] for k, v in N.STATS_CASES.items()}
    out.update({k: v[:5] for k, v in N.ONEPASS_CASES.items()})
    out.update({k: v[:5] for k, v in N.MODE2_CASES.items()})
    out.update({k: (v[0], 0, v[1], 1, v[3]) for k, v in N.FINALIZE_CASES.items()})
    out["refill"] = (D["c"], 0, D["hw"], 1, D["groups"])
    return out


GN_SHAPES = _gn_shapes()
SMALL = [k for k, v in GN_SHAPES.items() if v[2] * (v[0] + v[1]) <= 2 ** 20]  # the cases whose y is judged as a whole
_cache = {}


def case(name, s):
    """(x16, x fp64, gamma, beta) of a GroupNorm case; the last one is kept (the tests of a case run back to back)."""
    if _cache.get("key") != (name, s):
        c1, c2, hw, B, _ = GN_SHAPES[name]
        x, g, b = N.gn_data(name, c1 + c2, hw, B, s)
        _cache.update(key=(name, s), val=(x, d64(x), d64(g), d64(b)))
    return _cache["val"]


def _chunking(hw):
    """(nchunks, pix_per_chunk) of the library for hw pixels."""
    from upgpt_amd import _lib
    nch = _lib.load_library().upk_groupnorm_chunks(hw)
    return nch, -(-hw // nch)


def test_tables_agree_with_the_library_and_with_themselves():
    from upgpt_amd import _lib
    lib = _lib.load_library()
    for name, (c1, c2, hw, B, groups, nch, ppc) in N.STATS_CASES.items():
        assert lib.upk_groupnorm_chunks(hw) == nch and (nch - 1) * ppc < hw <= nch * ppc, name
        assert (c1 + c2) % groups == 0
        assert lib.upk_groupnorm_ws_bytes(B, hw) >= B * nch * groups * 2 * 4
    assert lib.upk_groupnorm_chunks(D["hw"]) == D["nchunks"] and D["nchunks"] * D["ppc"] == D["hw"]
    # the refill loop runs when a block owns more than 4 x 256 vectors; this is the smallest such element count
    assert D["rows"] == -(-D["hw"] * D["B"] // 4096) and D["rows"] * D["c"] // 8 > 1024 >= (D["rows"] - 1) * D["c"] // 8
    assert D["blocks"] == -(-D["hw"] // D["rows"])
    assert {v[5] for v in N.ONEPASS_CASES.values()} == set(N.PATHS)
    # the loops of gn_stats_kernel each Group A case is there for
    loops = {}
    for name, (c1, c2, hw, B, groups, nch, ppc) in N.STATS_CASES.items():
        _, rpi = N.stats_geometry(c1 + c2)
        unrolled, tail = ppc // (8 * rpi), -(-(ppc - ppc // (8 * rpi) * 8 * rpi) // rpi)
        loops[name] = (unrolled > 0, tail > 0, 256 % ((c1 + c2) // 8) != 0)
    assert loops["s224_768"] == (False, True, True) and loops["s224_2400"] == (True, True, True)
    assert loops["s128_4100"] == (True, True, False) and loops["s32_65"][:2] == (False, True)
    assert loops["s896_448_192"][2] and loops["s96_64_700"][2]
    for name, v in {**N.STATS_CASES, **N.ONEPASS_CASES, **N.MODE2_CASES}.items():
        g = N.straddling_group(v[0], v[1], v[4])
        assert (g is not None) == (name in ("s96_64_700", "s896_448_192", "o896_448_64", "o896_448_16", "m896_448_b3_32"))
    for c, hw, B, groups, nblk, ld, _ in N.FINALIZE_CASES.values():
        assert hw % nblk == 0 and ld >= c
    assert [d // 8 for d in N.LN_D] == [1, 28, 64, 65, 128, 129, 256]


@pytest.mark.parametrize("name", list(GN_SHAPES))
def test_groupnorm_data_is_in_range(name):
    c1, c2, hw, B, groups = GN_SHAPES[name]
    for s in (N.SCALES if name != "refill" else (1,)):
        x16, x, _, _ = case(name, s)
        assert torch.isfinite(x16).all() and float(x16.abs().max()) < R.F16_MAX
        assert float(x16.abs().min()) >= 2.0 ** -14  # no subnormal
        if hw * (c1 + c2) // groups == 1:
            continue  # (a group of ONE value has no spread: it normalises to beta, whatever the value)
        xg = x.reshape(B, hw, groups, -1).permute(0, 2, 1, 3).reshape(B, groups, -1)
        ratio = float((xg.mean(-1).abs() / xg.std(-1, unbiased=False)).max())
        print("%-16s scale %-5g max |mu|/sigma per group %.2f" % (name, s, ratio))
        assert ratio <= 4


@pytest.mark.parametrize("d", N.LN_D)
def test_layernorm_data_is_in_range(d):
    for rows in N.LN_ROWS:
        for s in N.SCALES:
            x16 = N.ln_data(rows, d, s)[0]
            x = d64(x16)
            assert torch.isfinite(x16).all() and float(x16.abs().max()) < R.F16_MAX
            assert float((x.mean(-1).abs() / x.std(-1, unbiased=False)).max()) <= 4


def _stats_near_misses(name, x, groups, nch, ppc):
    """The statistics near misses of one case against stats_chunk_refs: each must leave its bound in every chunk it
    changes, and nowhere else."""
    B, hw, C = x.shape
    ref, bnd = N.stats_chunk_refs(x, groups, nch, ppc)
    worst = lambda got: ((got - ref).abs() / bnd).amax((0, 2, 3))  # per chunk
    assert float(worst(ref).max()) == 0
    _, rpi = N.stats_geometry(C)
    k = nch // 2
    p_last = min(hw, (k + 1) * ppc) - 1
    one = N.pixel_sums(x, [p_last], groups)
    # one pixel dropped from chunk k
    got = ref.clone()
    got[:, k] -= one
    w = worst(got)
    print("%-14s dropped pixel: %.2f bounds" % (name, float(w[k])))
    assert w[k] > 1 and float(w.sum()) == float(w[k])
    # the boundary between k and k + 1 moved by one pixel
    got[:, k + 1] += one
    w = worst(got)
    print("%-14s moved boundary: %.2f / %.2f bounds" % (name, float(w[k]), float(w[k + 1])))
    assert w[k] > 1 and w[k + 1] > 1
    # one row slot left out (the last one that holds a pixel)
    r = min(rpi, ppc) - 1
    got = ref.clone()
    got[:, k] -= N.pixel_sums(x, list(range(k * ppc + r, min(hw, (k + 1) * ppc), rpi)), groups)
    assert worst(got)[k] > 1
    return ref, bnd


@pytest.mark.parametrize("name", list(N.STATS_CASES) + ["refill"])
def test_statistics_bounds_tell_near_misses_and_hold_for_the_kernel_order(name):
    c1, c2, hw, B, groups = GN_SHAPES[name]
    nch, ppc = N.STATS_CASES[name][5:] if name != "refill" else (D["nchunks"], D["ppc"])
    for s in (N.SCALES if name != "refill" else (1,)):
        x16, x, _, _ = case(name, s)
        ref, bnd = _stats_near_misses(name, x, groups, nch, ppc)
        g = N.straddling_group(c1, c2, groups)
        if g is not None:  # the straddling group summed over the first source's channels only
            xm = x.clone()
            xm[..., c1:(g + 1) * ((c1 + c2) // groups)] = 0
            got = N.stats_chunk_refs(xm, groups, nch, ppc)[0]
            bad = ((got - ref).abs() > bnd)
            assert bad[:, :, g].any(-1).all() and not bad[:, :, :g].any() and not bad[:, :, g + 1:].any()
        r = R.ratio(N.emu_stats(x16, groups, nch, ppc), ref, bnd)
        print("%-14s scale %-5g fp32 in kernel order: %.3f of the bound" % (name, s, r))
        assert r <= 1


def _y_near_misses(name, x, tot, groups, gamma, beta, eps, silu, ref, bound):
    mk = lambda **kw: N.apply_from_totals(x, tot, groups, gamma, beta, eps, silu, **kw)
    assert R.ratio(mk(), ref, bound) < 1e-3, name
    if groups > 1:
        assert R.ratio(mk(stat_roll=1), ref, bound) > 1, name + ": the next group's statistics"
    assert R.ratio(mk(param_roll=1), ref, bound) > 1, name + ": gamma / beta of the next channel"


@pytest.mark.parametrize("name", SMALL)
def test_output_bounds_tell_near_misses_and_hold_for_the_kernel_order(name):
    c1, c2, hw, B, groups = GN_SHAPES[name]
    C = c1 + c2
    for s in N.SCALES:
        x16, x, gamma, beta = case(name, s)
        tot = N.group_totals(x, groups)
        for eps, silu in ((1e-5, False), (1e-6, True)):
            ref, bound = R.groupnorm_ref(x, groups, gamma, beta, eps, silu)
            _y_near_misses(name, x, tot, groups, gamma, beta, eps, silu, ref, bound)
            g = N.straddling_group(c1, c2, groups)
            if g is not None:
                y = N.apply_from_totals(x, N.group_totals(x, groups, c_only=(g, c1)), groups, gamma, beta, eps, silu)
                assert R.ratio(y, ref, bound) > 1, name + ": straddling group from source 1 only"
            # fp32 in the kernels' order
            if name in N.ONEPASS_CASES and N.ONEPASS_CASES[name][5] != "twopass":
                V = int(N.ONEPASS_CASES[name][5][9])
                e_tot = N.emu_onepass_totals(x16, groups, V)
            elif name in N.MODE2_CASES:
                _, _, _, _, _, nb1, nb2, ld1, ld2 = N.MODE2_CASES[name]
                parts = [N.make_partials(x16[..., :c1].contiguous(), nb1, ld1)]
                if c2:
                    parts.append(N.make_partials(x16[..., c1:].contiguous(), nb2, ld2))
                e_tot = N.emu_partial_totals(parts, (c1, c2)[:len(parts)], groups)
                # one row block left out (of the last source; a single block left out leaves nothing to normalise with)
                chs = [p[..., :c].to(F64) for p, c in zip(parts, (c1, c2))]
                if chs[-1].shape[1] > 1:
                    chs[-1] = chs[-1][:, :-1]
                    t = torch.cat([p.sum(1) for p in chs], -1).reshape(B, 2, groups, C // groups).sum(-1).transpose(1, 2)
                    y = N.apply_from_totals(x, t, groups, gamma, beta, eps, silu)
                    assert R.ratio(y, ref, bound) > 1, name + ": a row block left out"
                y = N.apply_from_totals(x, tot.flip(-1), groups, gamma, beta, eps, silu)
                assert R.ratio(y, ref, bound) > 1, name + ": planes swapped"
            else:
                nch, ppc = N.STATS_CASES[name][5:] if name in N.STATS_CASES else _chunking(hw)
                e_tot = N.emu_stats(x16, groups, nch, ppc).double().sum(1)
            r = R.ratio(N.emu_apply(x16, e_tot, groups, gamma, beta, eps, silu), ref, bound)
            print("%-16s scale %-5g eps %g silu %d fp32 in kernel order: %.3f of the bound" % (name, s, eps, silu, r))
            assert r <= 1


def test_refill_case_output_bound_on_one_sample():
    """The 8.4 M values of one sample of the refill case: the near misses of y and the kernel order."""
    x16, x, gamma, beta = case("refill", 1)
    groups, eps, silu = D["groups"], D["eps"], D["silu"]
    ref, bound = R.groupnorm_ref(x, groups, gamma, beta, eps, silu)
    tot = N.group_totals(x, groups)
    _y_near_misses("refill", x, tot, groups, gamma, beta, eps, silu, ref, bound)
    e_tot = N.emu_stats(x16, groups, D["nchunks"], D["ppc"]).double().sum(1)
    r = R.ratio(N.emu_apply(x16, e_tot, groups, gamma, beta, eps, silu), ref, bound)
    print("refill fp32 in kernel order: %.3f of the bound" % r)
    assert r <= 1


@pytest.mark.parametrize("name", list(N.FINALIZE_CASES))
def test_finalize_bound_tells_a_missing_stride(name):
    c, hw, _, groups, nblk, ld, _ = N.FINALIZE_CASES[name]
    cpg = c // groups
    for s in N.SCALES:
        x16, x, _, _ = case(name, s)
        ref, bnd = N.fold_refs(x, nblk, groups)
        part = N.make_partials(x16, nblk, ld)[..., :c]
        # what the kernel does: fp64 over the fp32 partials, one rounding
        got = N.totals(part, groups).float()
        r = R.ratio(got, ref, bnd)
        print("%-12s scale %-5g fold of fp32 partials: %.3f of the bound" % (name, s, r))
        assert r <= 1
        # the last 256-wide stride of the (block, channel) pairs e = block * cpg + channel left out
        n = nblk * cpg
        e = torch.arange(n)
        keep = (e < (n - 1) // 256 * 256).reshape(nblk, cpg)
        p = part.to(F64).reshape(1, nblk, 2, groups, cpg) * keep[None, :, None, None, :]
        mut = p.sum((1, 4)).transpose(1, 2)
        assert (((mut - ref).abs() > bnd).all()), name
        # the partials themselves are inside their bound
        pref, pbnd = N.partial_refs(x, nblk)
        assert R.ratio(part, pref, pbnd) <= 1


@pytest.mark.parametrize("d", N.LN_D)
def test_layernorm_bound_tells_near_misses_and_holds_for_the_kernel_order(d):
    nv = d // 8
    padded = 64 * (1 if nv <= 64 else 2 if nv <= 128 else 4)
    for rows in N.LN_ROWS:
        for s in N.SCALES:
            x16, gamma, beta = N.ln_data(rows, d, s)
            x, g, b = d64(x16), d64(gamma), d64(beta)
            for eps in N.EPS:
                ref, bound = R.layernorm_ref(x, g, b, eps)
                assert R.ratio(N.layernorm_mutant(x, g, b, eps), ref, bound) < 1e-3
                bad = (N.layernorm_mutant(x, g, b, eps, drop_last_vector=True) - ref).abs() > bound
                assert bad.any(), "the last vector left out of the mean"
                if padded != nv:  # (where every lane slot holds a vector the padded count IS d)
                    bad = (N.layernorm_mutant(x, g, b, eps, padded_count=True) - ref).abs() > bound
                    assert bad.any(-1).all(), "1 / d over the padded lane slots: every row shows it"
                r = R.ratio(N.emu_layernorm(x16, gamma, beta, eps), ref, bound)
                assert r <= 1, (rows, d, s, eps, r)
    print("layernorm d=%d fp32 in kernel order: inside the bound" % d)
