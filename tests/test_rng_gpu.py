"""upk_philox_u32 / upk_randn_keyed_f32 (upgpt_amd/csrc/rng.hip, include/upk.h) on a real MI355X against the numpy
restatement tests/rng_ref.py: the integer stage exactly, the normals against the fp64 value of the same formula on the
same words, that a value depends on nothing but (key, element, row, stream, draw), and the moments of 2^20 values.

Bounds.  Words: equality.  Normals: |z - z64| <= 1e-5 — |z| <= 5.77 times a few fp32 ulp of log, sqrt and sin / cos plus
the rounding of r and of the product: below 3e-6, so 1e-5 leaves a factor 3.  Moments of N = 2^20 standard normals, five
standard errors each: mean 5 / sqrt(N) = 4.9e-3, variance 5 sqrt(2 / N) = 6.9e-3, fourth moment 5 sqrt(96 / N) = 4.8e-2,
correlation 5 / sqrt(N) = 4.9e-3."""
import ctypes

import numpy as np
import pytest
import torch

import rng_ref
from upgpt_amd import _lib as L
from upgpt_amd import rng

pytestmark = pytest.mark.gpu
GUARD = 64  # sentinel elements on both sides of every output
SENT = 0x5A5A5A5A
SEED, IDS = 0x1234567890ABCDEF, [3, 1 << 33, 7]
N_LATENT = 4 * 32 * 24


@pytest.fixture(scope="module")
def ctx():
    return L.get_context(0)


def _keys(ids=IDS, seed=SEED, draw=0):
    return rng.NoiseKeys(seed, ids, device="cuda:0", draw=draw)


def _fill(ctx, keys, n, row0, rows, stream, draw, normal, offset=0, scale=None):
    """One launch into a guarded buffer whose payload starts `offset` floats behind a 16-byte boundary -> the payload
    [rows, B, n] as int32 bits (host) after checking that no sentinel was touched."""
    b, total = len(keys), rows * len(keys) * n
    buf = torch.full((GUARD + offset + total + GUARD,), SENT, dtype=torch.int32, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and GUARD % 4 == 0
    out = buf[GUARD + offset:GUARD + offset + total]
    if normal:
        ctx.randn_keyed(keys.keys, b, n, row0, rows, stream, draw, scale, out)
    else:
        ctx.philox_u32(keys.keys, b, n, row0, rows, stream, draw, out)
    host = buf.cpu().numpy()
    assert (host[:GUARD + offset] == SENT).all() and (host[GUARD + offset + total:] == SENT).all(), "wrote out of bounds"
    return host[GUARD + offset:GUARD + offset + total].reshape(rows, b, n)


@pytest.mark.parametrize("n", [1, 6, 4097, N_LATENT])
@pytest.mark.parametrize("B", [1, 3])
def test_words_equal_the_reference_exactly(ctx, n, B):
    keys = _keys(IDS[:B])
    assert np.array_equal(keys.host, rng_ref.keys_of(SEED, IDS[:B]))
    for row0, rows in ((0, 1), (5, 3)):
        for offset in (0, 1):
            for stream, draw in ((0, 0), (3, 7), (0xFFFFFFFF, 0x80000001)):
                got = _fill(ctx, keys, n, row0, rows, stream, draw, False, offset).view(np.uint32)
                want = rng_ref.words(keys.host, n, row0, rows, stream, draw)
                assert np.array_equal(got, want), (n, B, row0, rows, offset, stream, draw)


@pytest.mark.parametrize("n", [1, 6, 4097, N_LATENT])
def test_normals_against_the_fp64_formula(ctx, n):
    keys = _keys()
    for offset in (0, 1):
        got = _fill(ctx, keys, n, 5, 3, rng.STREAM_STEP, 2, True, offset).view(np.float32).astype(np.float64)
        want = rng_ref.normals(keys.host, n, 5, 3, rng.STREAM_STEP, 2)
        err = float(np.abs(got - want).max())
        print("n = %d offset %d: max |z - z64| = %.3e, max |z| = %.3f" % (n, offset, err, np.abs(got).max()))
        assert err <= 1e-5
        assert np.abs(got).max() <= np.sqrt(48 * np.log(2.0)) + 1e-5


def test_extreme_words_give_the_bounded_tail():
    """The transform's corners in fp64: u1 = 2^-24 gives r = sqrt(48 ln 2); u1 = 1 gives 0."""
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - np.sqrt(48 * np.log(2.0))) < 1e-12


def test_row_scale_and_zero_rows(ctx):
    keys = _keys()
    n, row0, rows = 4097, 2, 4
    scale = torch.tensor([9.0, 9.0, 0.5, 0.0, -2.0, 1.0, 9.0], device="cuda:0")  # indexed by the ABSOLUTE row
    plain = _fill(ctx, keys, n, row0, rows, 1, 0, True).view(np.float32)
    got = _fill(ctx, keys, n, row0, rows, 1, 0, True, scale=scale).view(np.float32)
    sc = scale.cpu().numpy()[row0:row0 + rows]
    assert np.array_equal(got, plain * sc[:, None, None])  # one fp32 product per element
    assert (got[1].view(np.uint32) == 0).all()  # a zero row is +0, bit for bit
    assert np.abs(got[0]).max() > 1.0


def test_a_value_depends_on_key_element_row_stream_draw_only(ctx):
    keys = _keys()
    n, S = N_LATENT + 2, 6  # (n % 4 == 2: the samples of a row start at every alignment)
    full = _fill(ctx, keys, n, 0, S, 1, 4, True)
    # two windows of the table
    assert np.array_equal(_fill(ctx, keys, n, 0, 2, 1, 4, True), full[:2])
    assert np.array_equal(_fill(ctx, keys, n, 2, 4, 1, 4, True, offset=3), full[2:])
    # every sample alone, and at another position of another batch
    for b in range(3):
        assert np.array_equal(_fill(ctx, keys[b:b + 1], n, 0, S, 1, 4, True)[:, 0], full[:, b])
    rev = rng.NoiseKeys(SEED, IDS[::-1], device="cuda:0")
    assert np.array_equal(_fill(ctx, rev, n, 0, S, 1, 4, True)[:, ::-1], full)
    # (rng.randn, the package's wrapper, is the same launch)
    t = rng.randn(keys.fork(4), (3, n), rng.STREAM_STEP, row0=0, rows=S)
    assert np.array_equal(t.cpu().numpy().view(np.int32).reshape(S, 3, n), full)
    one = rng.randn(keys.fork(4), (3, 2, n // 2), rng.STREAM_STEP, row0=3)
    assert tuple(one.shape) == (3, 2, n // 2) and np.array_equal(one.cpu().numpy().view(np.int32).reshape(3, n), full[3])
    # another stream, draw, row or key is another table
    base = full[0, 0].view(np.float32)
    others = {"stream": _fill(ctx, keys, n, 0, 1, 2, 4, True)[0, 0], "draw": _fill(ctx, keys, n, 0, 1, 1, 5, True)[0, 0],
              "row": full[1, 0], "key": full[0, 1]}
    for what, o in others.items():
        assert (o.view(np.float32) != base).mean() > 0.99, what


def test_many_tiles_go_grid_stride(ctx):
    """More tiles than workgroups of a launch (2^16): the words past the first sweep are still the reference's."""
    keys = _keys(IDS[:1])
    n, rows = 1030, 40000  # 2 tiles a row -> 80000 tiles
    out = torch.empty(rows * n, dtype=torch.int32, device="cuda:0")
    ctx.philox_u32(keys.keys, 1, n, 0, rows, 1, 0, out)
    got = out.view(rows, n)[[0, 32767, 32768, 39999]].cpu().numpy().view(np.uint32)
    for g, r in zip(got, (0, 32767, 32768, 39999)):
        assert np.array_equal(g, rng_ref.words(keys.host, n, r, 1, 1, 0)[0, 0]), r


def test_moments_of_2_pow_20_values(ctx):
    keys = rng.NoiseKeys(1234, [0, 1], device="cuda:0")
    N = 1 << 20
    z = rng.randn(keys, (2, N), rng.STREAM_STEP, row0=0, rows=2).view(2, 2, N).double().cpu().numpy()
    a = z[0, 0]
    corr = lambda u, v: float(np.mean((u - u.mean()) * (v - v.mean())) / (u.std() * v.std()))
    mean, var, m4 = float(a.mean()), float(a.var()), float(np.mean(a ** 4))
    c_row, c_key = corr(a, z[1, 0]), corr(a, z[0, 1])
    print("mean %.3e  var - 1 %.3e  E z^4 - 3 %.3e  corr(next row) %.3e  corr(other key) %.3e" % (
        mean, var - 1, m4 - 3, c_row, c_key))
    assert abs(mean) < 4.9e-3 and abs(var - 1) < 6.9e-3 and abs(m4 - 3) < 4.8e-2
    assert abs(c_row) < 4.9e-3 and abs(c_key) < 4.9e-3


def test_argument_errors(ctx):
    keys = _keys()
    out = torch.empty(64, dtype=torch.float32, device="cuda:0")
    lib, h, s = ctx.lib, ctx.h, ctypes.c_void_p(ctx._s())
    k, o = keys.keys.data_ptr(), out.data_ptr()
    bad = [dict(keys=None), dict(out=None), dict(batch=0), dict(n=0), dict(rows=0), dict(row0=-1), dict(n=(1 << 34) + 1),
           dict(batch=-1), dict(n=-5), dict(rows=-2)]
    for kw in bad:
        a = dict(keys=k, batch=3, n=4, row0=0, rows=1, out=o)
        a.update(kw)
        assert lib.upk_randn_keyed_f32(h, a["keys"], a["batch"], a["n"], a["row0"], a["rows"], 1, 0, None, a["out"], s) == -1, kw
        assert lib.upk_philox_u32(h, a["keys"], a["batch"], a["n"], a["row0"], a["rows"], 1, 0, a["out"], s) == -1, kw
    torch.cuda.synchronize()
