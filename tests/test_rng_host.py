"""Host side of the keyed noise (upgpt_amd/rng.py, include/upk.h upk_randn_keyed_f32): the numpy reference against the
Random123 known answers, NoiseKeys against the reference's derivation, the samplers' argument checks, the declarations."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rng_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_reference_known_answers(ctr, key, want):
    assert rng_ref.philox(ctr, key).tolist() == want


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_package_philox_known_answers(ctr, key, want):
    from upgpt_amd import rng
    assert rng.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64)).tolist() == want


def test_noise_keys_derivation():
    from upgpt_amd import rng
    k = rng.NoiseKeys(0, range(4))
    assert k.host.dtype == np.uint32 and k.host.shape == (4, 2)
    assert [int(v) for v in k.host[:, 0]] == [0x6627e8d5, 0xf8e4cca4, 0x04faa329, 0xc990ef29]
    seed, ids = 0xfedcba9876543210, [0, 1, 7, (1 << 40) + 3, (1 << 64) - 1]
    assert np.array_equal(rng.NoiseKeys(seed, ids).host, rng_ref.keys_of(seed, ids))
    # a sample's key does not depend on the batch it is derived in
    assert np.array_equal(rng.NoiseKeys(seed, ids[3:4]).host, rng_ref.keys_of(seed, ids)[3:4])
    for bad in (dict(seed=-1, ids=[0]), dict(seed=1 << 64, ids=[0]), dict(seed=0, ids=[1 << 64]), dict(seed=0, ids=[-1])):
        with pytest.raises(ValueError):
            rng.NoiseKeys(**bad)


def test_fork_and_slice():
    from upgpt_amd import rng
    k = rng.NoiseKeys(5, [10, 11, 12], draw=0)
    f = k.fork(3)
    assert (f.draw, k.draw) == (3, 0) and f.ids == k.ids and f.seed == k.seed and np.array_equal(f.host, k.host)
    s = k[:2]
    assert len(k) == 3 and len(s) == 2 and s.ids == [10, 11] and np.array_equal(s.host, k.host[:2]) and s.draw == 0
    assert len(f[1:]) == 2 and f[1:].draw == 3 and f[1:].ids == [11, 12]
    assert (rng.STREAM_XT, rng.STREAM_STEP, rng.STREAM_QSAMPLE) == (0, 1, 2)


def test_argument_checks():
    from upgpt_amd import rng
    k = rng.NoiseKeys(1, [0, 1])
    rng.check_keys(None, 5)
    rng.check_keys(k, 2)
    with pytest.raises(ValueError, match="2 keys for a batch of 3"):
        rng.check_keys(k, 3)
    with pytest.raises(ValueError, match="normals_sequence"):
        rng.check_keys(k, 2, normals_sequence=[None])
    with pytest.raises(ValueError, match="repeat_noise"):
        rng.check_keys(k, 2, repeat_noise=True)


def test_samplers_refuse_bad_keys_before_any_device_work():
    """The checks come first: they raise on a machine without a GPU, before the sampler touches the model."""
    import upgpt_amd
    from upgpt_amd import rng
    from upgpt_amd.ddim import DDIMSampler
    from upgpt_amd.plms import PLMSSampler
    m = upgpt_amd.build_model("tiny")
    k = rng.NoiseKeys(1, [0, 1, 2])
    shape = (m.channels, *m.image_size)
    for sampler in (DDIMSampler(m), PLMSSampler(m)):
        with pytest.raises(ValueError, match="3 keys for a batch of 2"):
            sampler.sample(4, 2, shape, conditioning=None, verbose=False, noise_keys=k)
    with pytest.raises(ValueError, match="normals_sequence"):
        DDIMSampler(m).sample(4, 3, shape, conditioning=None, verbose=False, noise_keys=k, normals_sequence=[0] * 4)
    with pytest.raises(ValueError, match="3 keys for a batch of 2"):
        m.p_sample_loop(None, (2,) + shape, noise_keys=k)
    with pytest.raises(ValueError, match="repeat_noise"):
        DDIMSampler(m)._ddim_update(None, None, 0, repeat_noise=True, noise_keys=k)
    with pytest.raises(ValueError, match="repeat_noise"):
        m.p_sample(None, None, None, repeat_noise=True, noise_keys=k)


def test_run_test_refuses_lanes_without_seed(tmp_path):
    import upgpt_amd
    from upgpt_amd import evaluate
    m = upgpt_amd.build_model("tiny")
    with pytest.raises(ValueError, match="noise_seed"):
        evaluate.run_test(m, [], str(tmp_path), lanes=2)
    assert "logger" not in vars(m)


def test_symbols_declared_and_built():
    from upgpt_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "upk.h")).read()
    declared = set(re.findall(r"\b(upk_[a-z0-9_]+)\s*\(", header))
    for name in ("upk_randn_keyed_f32", "upk_philox_u32"):
        assert name in declared and name in _lib.SYMBOLS
    assert "0xD2511F53" in header and "0xCD9E8D57" in header and "0x9E3779B9" in header and "0xBB67AE85" in header
    assert "rng.hip" in build.SOURCES and build.FILE_FLAGS["rng.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(build.CSRC, "rng.hip"))
