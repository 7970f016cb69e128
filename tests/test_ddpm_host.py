"""CPU checks of the DDPM ancestral sampler's host side: the fused coefficient table against the reference's update
rule and its recorded values (tests/golden/ddpm.npz), make_grid's layout, the new ABI entry and the validation of
injected normals."""
import os

import numpy as np
import pytest
import torch

import upgpt_amd
from upgpt_amd import _lib, schedule
from upgpt_amd.grid import make_grid

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _reference_step(m, x, eps, noise, t):
    """ddpm.py:224-237, 1157-1187 evaluated the reference's way (fp32 torch, its op order)."""
    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    x_recon = m.predict_start_from_noise(x, tt, eps)
    mean, _, logvar = m.q_posterior(x_recon, x, tt)
    nonzero = (1 - (tt == 0).float()).reshape(-1, 1, 1, 1)
    return mean + nonzero * (0.5 * logvar).exp() * noise, x_recon


def test_ddpm_coefficient_table_matches_update_rule_and_reference():
    m = upgpt_amd.build_model("tiny")
    order = np.arange(1000)[::-1].copy()
    tab = schedule.ddpm_coefficient_table(m, order)
    assert tab.shape == (1000, 8) and tab.dtype == torch.float32
    assert float(tab[-1, 4]) == 0.0 and float(tab[:-1, 4].min()) > 0.0  # no noise at t = 0 only
    assert float(tab[:, 7].abs().max()) == 0.0
    g = np.load(os.path.join(G, "ddpm.npz"))
    ref = torch.as_tensor(g["table"])  # the reference model's buffers, combined as ddpm.py does, timesteps 999 ... 0
    assert torch.equal(tab, ref)
    gen = torch.Generator().manual_seed(0)
    x, e, n, x0 = (torch.randn(2, 4, 4, 3, generator=gen) for _ in range(4))
    for k in (0, 1, 500, 998, 999):
        t = int(order[k])
        want, want_x0 = _reference_step(m, x, e, n, t)
        row = tab[k]
        xr = row[0] * x - row[1] * e
        got = row[2] * xr + row[3] * x + row[4] * n
        assert torch.allclose(xr, want_x0, rtol=1e-6, atol=1e-6)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), t
        tt = torch.full((2,), t, dtype=torch.long)
        assert torch.allclose(row[5] * x0 + row[6] * n, m.q_sample(x0, tt, noise=n), rtol=1e-6, atol=1e-6)


def test_make_grid_layout_hand_checked():
    """torchvision's layout: xmaps = min(nrow, N), ymaps = ceil(N / xmaps), (H + 2) x (W + 2) cells, a 2-pixel outer
    pad, one channel repeated to three."""
    imgs = torch.arange(1, 6, dtype=torch.float32).reshape(5, 1, 1, 1).expand(5, 1, 2, 3).contiguous()
    grid = make_grid(imgs, nrow=2)
    assert grid.shape == (3, 3 * 4 + 2, 2 * 5 + 2)
    want = torch.zeros(14, 12)
    for k in range(5):
        y, x = divmod(k, 2)
        want[y * 4 + 2:y * 4 + 4, x * 5 + 2:x * 5 + 5] = k + 1
    for c in range(3):
        assert torch.equal(grid[c], want)
    assert torch.equal(make_grid(imgs[:1], nrow=2), imgs[0].expand(3, 2, 3))  # a single image comes back unpadded
    assert make_grid(list(imgs[:3].expand(3, 3, 2, 3)), nrow=8, pad_value=0.5).shape == (3, 6, 17)


def test_ddpm_step_is_exported():
    assert "upk_ddpm_step_f32" in _lib.SYMBOLS
    assert hasattr(_lib.load_library(), "upk_ddpm_step_f32")


def test_normals_sequence_is_validated():
    """One standard normal per draw of the reference, in its order: T posterior draws, 2T with a mask."""
    m = upgpt_amd.build_model("tiny")
    cond = {"c_crossattn": torch.zeros(2, 87, 768), "c_concat": [torch.zeros(2, 1, 32, 24)]}
    shape = (2, 4, 32, 24)
    with pytest.raises(ValueError, match="normals_sequence"):
        m.p_sample_loop(cond, shape, timesteps=3, normals_sequence=torch.zeros(2, *shape))
    with pytest.raises(ValueError, match="normals_sequence"):
        m.p_sample_loop(cond, shape, timesteps=3, normals_sequence=[torch.zeros(1, 4, 32, 24)] * 3)
    with pytest.raises(ValueError, match="normals_sequence"):  # with a mask: posterior, q_sample per step
        m.p_sample_loop(cond, shape, timesteps=3, mask=torch.ones(2, 1, 32, 24), x0=torch.zeros(shape),
                        normals_sequence=torch.zeros(3, *shape))
    with pytest.raises(NotImplementedError):
        m.sample(cond, batch_size=2, quantize_denoised=True)
