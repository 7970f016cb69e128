"""Keyed device noise: every normal is a pure function of (seed, sample id, draw, stream, row, element).

A sample's noise no longer depends on where it sits in a batch, on the batch size, on the order of the batches or on the
rank: NoiseKeys(seed, ids) gives every sample a 64-bit Philox key derived from (seed, id), and upk_randn_keyed_f32
(include/upk.h: Philox4x32-10, counter (element >> 2, row, stream, draw), Box-Muller) fills a whole [rows, B, n] noise
table in ONE launch on the caller's own stream — no torch generator, no generator state, no lock.  The samplers take
the keys as `noise_keys=` (ddim.py, plms.py, ancestral.py), log_images forwards them, evaluate.run_test builds them from
`noise_seed`.  DESIGN.md 28.  The loss surface takes them too (p_losses / forward / shared_step / validation_step,
evaluate.run_validation(noise_seed=)): there the timestep and the noise are drawn inside upk_q_sample_keyed_f32.  DESIGN.md 29.

The key derivation runs on the host in numpy and is restated independently in tests/rng_ref.py.
"""
import numpy as np
import torch

from ._check import require
from ._lib import get_context

# the counter's `stream` word: one value per USE of the noise, so x_T, the step noise and the q_sample noise of one
# sample never share a Philox call
STREAM_XT, STREAM_STEP, STREAM_QSAMPLE = 0, 1, 2
STREAM_POSTERIOR = 3  # the first stage's posterior sample of an encoded batch (LatentDiffusion.get_input)
# the two draws of a loss evaluation, made inside upk_q_sample_keyed_f32 (UPK_STREAM_TIMESTEP, UPK_STREAM_LOSS_NOISE)
STREAM_TIMESTEP, STREAM_LOSS_NOISE = 4, 5

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit words: ctr [..., 4], key [..., 2] -> [..., 4]."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & _MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & _MASK for i in range(2)]
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]  # (32 x 32 bit: no overflow in uint64)
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> s32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(c, axis=-1)


def derive_keys(seed, ids):
    """uint32 [B, 2]: key_i = Philox4x32-10(ctr = (id_lo, id_hi, 0, 0), key = (seed_lo, seed_hi))[0:2]."""
    seed = int(seed)
    ids = [int(i) for i in ids]
    require(0 <= seed < 1 << 64, "seed must be in [0, 2^64)", ValueError)
    require(all(0 <= i < 1 << 64 for i in ids), "sample ids must be in [0, 2^64)", ValueError)
    ctr = np.zeros((len(ids), 4), dtype=np.uint64)
    ctr[:, 0] = [i & 0xFFFFFFFF for i in ids]
    ctr[:, 1] = [i >> 32 for i in ids]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (len(ids), 2)))[:, :2].astype(np.uint32)


class NoiseKeys:
    """The Philox keys of a batch: one per sample, derived from (seed, sample id) on the host and kept as a device uint32
    [B, 2] tensor (`keys`; `host` is the numpy copy), plus `draw`, the counter word that separates sampling calls which
    share the keys.  len(), slicing (keys[:n], a view of the same device tensor) and fork(j) (the same keys with
    draw = j) make no device work."""

    def __init__(self, seed, ids, device=None, draw=0):
        self.seed = int(seed)
        self.ids = [int(i) for i in ids]
        self.host = derive_keys(self.seed, self.ids)
        require(0 <= int(draw) < 1 << 32, "draw must be in [0, 2^32)", ValueError)
        self.draw = int(draw)
        self.device = None if device is None else torch.device(device)
        self._keys = None

    @property
    def keys(self):
        """Device uint32 [B, 2] (stored as int32 bits), uploaded on first use."""
        if self._keys is None:
            dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            self._keys = torch.from_numpy(self.host.view(np.int32).copy()).to(dev)
            self.device = self._keys.device
        return self._keys

    def __len__(self):
        return len(self.ids)

    def _like(self, ids, host, keys, draw):
        new = object.__new__(NoiseKeys)
        new.seed, new.ids, new.host, new.draw, new.device, new._keys = self.seed, ids, host, draw, self.device, keys
        return new

    def __getitem__(self, sl):
        require(isinstance(sl, slice) and sl.step in (None, 1), "NoiseKeys supports contiguous slices only", TypeError)
        return self._like(self.ids[sl], self.host[sl], None if self._keys is None else self._keys[sl], self.draw)

    def fork(self, j):
        """The same keys with draw = j: another sampling call over the same samples."""
        require(0 <= int(j) < 1 << 32, "draw must be in [0, 2^32)", ValueError)
        return self._like(self.ids, self.host, self._keys, int(j))


def check_keys(noise_keys, batch_size, normals_sequence=None, repeat_noise=False):
    """The argument rules every sampler applies to `noise_keys` (None passes)."""
    if noise_keys is None:
        return
    require(isinstance(noise_keys, NoiseKeys), "noise_keys must be an upgpt_amd.rng.NoiseKeys", TypeError)
    require(len(noise_keys) == int(batch_size), lambda: "noise_keys holds %d keys for a batch of %d" % (
        len(noise_keys), int(batch_size)), ValueError)
    require(normals_sequence is None, "noise_keys and normals_sequence both name the chain's noise: give one", ValueError)
    require(not repeat_noise, "repeat_noise shares one draw over the batch; noise_keys gives every sample its own", ValueError)


def randn(keys, shape, stream, row0=0, rows=None, scale=None, out=None):
    """Keyed standard normals through upk_randn_keyed_f32 on the calling lane's context and current stream.
    shape = (B, ...) with B == len(keys): the per-sample shape is shape[1:].
    rows None: ONE row, `row0`, returned as a tensor of `shape` (x_T, one step's noise).
    rows = R:  rows row0 .. row0 + R - 1, returned as [R, B * n] (a sampler's table, or a slice of one as `out`).
    scale: a device fp32 tensor indexed by the ABSOLUTE row (>= row0 + rows entries): row r is multiplied by scale[r].
    out: a contiguous fp32 device tensor of the result's size to fill instead of a fresh one."""
    require(isinstance(keys, NoiseKeys), "randn needs NoiseKeys", TypeError)
    shape = tuple(int(s) for s in shape)
    require(len(shape) >= 1 and shape[0] == len(keys), lambda: "shape %s does not start with the %d keys" % (
        shape, len(keys)), ValueError)
    b, n = shape[0], int(np.prod(shape[1:], dtype=np.int64))
    kt = keys.keys
    dev = kt.device
    r = 1 if rows is None else int(rows)
    want = shape if rows is None else (r, b * n)
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    require(out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == r * b * n,
            "randn: out must be a contiguous fp32 device tensor of %d elements" % (r * b * n), ValueError)
    if scale is not None:
        require(scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() >= int(row0) + r,
                "randn: scale must be a contiguous fp32 device tensor with an entry for every absolute row", ValueError)
    with torch.cuda.device(dev):
        get_context(dev).randn_keyed(kt, b, n, int(row0), r, int(stream), keys.draw, scale, out)
    return out
