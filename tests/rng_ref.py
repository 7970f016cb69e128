"""Independent numpy restatement of the keyed noise of include/upk.h (upk_randn_keyed_f32 / upk_philox_u32): Philox4x32-10
in uint64 arithmetic, the key derivation of upgpt_amd.rng.NoiseKeys, the words of a [rows, batch, n] table and the fp64
value of the normal transform.  Nothing here imports the code under test."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)


def philox(ctr, key):
    """ctr: uint64 [..., 4] of 32-bit words, key: uint64 [..., 2] -> the four output words, uint64 [..., 4]."""
    ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i].copy() for i in range(4))
    k0, k1 = key[..., 0].copy(), key[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & LO
        hi1, lo1 = p1 >> np.uint64(32), p1 & LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & LO
        k1 = (k1 + np.uint64(W1)) & LO
    return np.stack([c0, c1, c2, c3], axis=-1)


def keys_of(seed, ids):
    """uint32 [B, 2]: words 0, 1 of philox(ctr = (id_lo, id_hi, 0, 0), key = (seed_lo, seed_hi))."""
    ctr = np.array([[i & 0xFFFFFFFF, i >> 32, 0, 0] for i in ids], dtype=np.uint64)
    key = np.array([[seed & 0xFFFFFFFF, seed >> 32]] * len(ids), dtype=np.uint64)
    return philox(ctr, key)[:, :2].astype(np.uint32)


def quads(keys, n, row0, rows, stream, draw):
    """uint64 [rows, B, ceil(n / 4), 4]: the Philox call of every quad of every (row, sample)."""
    keys = np.asarray(keys, dtype=np.uint64)
    b, nq = keys.shape[0], (n + 3) // 4
    ctr = np.zeros((rows, b, nq, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nq, dtype=np.uint64)
    ctr[..., 1] = (np.arange(rows, dtype=np.uint64) + np.uint64(row0))[:, None, None]
    ctr[..., 2] = np.uint64(stream)
    ctr[..., 3] = np.uint64(draw)
    return philox(ctr, np.broadcast_to(keys[None, :, None, :], (rows, b, nq, 2)))


def words(keys, n, row0=0, rows=1, stream=0, draw=0):
    """uint32 [rows, B, n]: word e & 3 of quad e >> 2."""
    w = quads(keys, n, row0, rows, stream, draw)
    return w.reshape(rows, w.shape[1], -1)[:, :, :n].astype(np.uint32)


def normals(keys, n, row0=0, rows=1, stream=0, draw=0):
    """float64 [rows, B, n]: Box-Muller of the word pairs (w0, w1) and (w2, w3) evaluated in fp64."""
    w = quads(keys, n, row0, rows, stream, draw)
    z = np.empty(w.shape, dtype=np.float64)
    for a in (0, 2):
        u1 = ((w[..., a] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        u2 = (w[..., a + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[..., a] = r * np.cos(2.0 * np.pi * u2)
        z[..., a + 1] = r * np.sin(2.0 * np.pi * u2)
    return z.reshape(rows, z.shape[1], -1)[:, :, :n]
