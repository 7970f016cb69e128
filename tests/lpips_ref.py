"""CPU restatement of lpips.LPIPS(net='vgg', version='0.1', lpips=True, spatial=False) in eval mode (lpips 0.1.4), in
torch; neither lpips nor torchvision is needed.  The algorithm is the one stated in include/upk.h:

  scaling   x' = (x - shift) / scale            (normalize: x = 2 x - 1 first)
  features  13 x (conv 3x3 pad 1 + bias, ReLU) in slices of 2, 2, 3, 3, 3; MaxPool2d(2, 2) (floor) in front of slices 2..5
  taps      after the last ReLU of every slice
  distance  f^ = f / (sqrt(sum_c f_c^2) + 1e-10); d_l = mean over pixels of sum_c w_l[c] (f^0_c - f^1_c)^2

Modes: "ref64" everything in fp64; "emu16" what the device pipeline stores, apart from summation order: weights rounded to
fp16, the scaled input computed in fp32 and rounded to fp16, every conv + bias computed in fp32 and rounded to fp16 before
its ReLU, taps in fp16, the distance in fp64.

Near misses (keyword switches, all off by default): pm1 (input mapped to [-1, 1]), no_scaling, pre_relu (taps before the
ReLU), ceil_pool, eps_inside (the normalisation's eps inside the square root).
"""
import numpy as np
import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHANNELS = (64, 128, 256, 512, 512)
EPS = 1e-10
NEAR_MISSES = ("pm1", "no_scaling", "pre_relu", "ceil_pool", "eps_inside")


def layer_distance(f0, f1, w, eps_inside=False):
    """d_l [N] fp64 of features f0, f1 [N, C, h, w] (any dtype, taken to fp64) and lin weight w [C]."""
    f0, f1, w = f0.double(), f1.double(), w.double().reshape(1, -1, 1, 1)

    def unit(f):
        s = (f * f).sum(1, keepdim=True)
        return f / (torch.sqrt(s + EPS) if eps_inside else torch.sqrt(s) + EPS)

    d = (unit(f0) - unit(f1)) ** 2
    return (w * d).sum(1).mean((1, 2))


def lpips_layers(sd, in0, in1, mode="ref64", normalize=False, pm1=False, no_scaling=False, pre_relu=False, ceil_pool=False,
                 eps_inside=False):
    """[N, 5] fp64: d_l of every pair.  in0, in1: [N, 3, H, W] in [0, 1] (fp64 for ref64; emu16 takes them to fp32, as the
    device's u / 255 is), sd: an lpips-style state dict."""
    assert mode in ("ref64", "emu16")
    emu = mode == "emu16"
    wd = torch.float32 if emu else torch.float64

    def rnd(t):  # what is stored in fp16 on the device
        return t.half().to(wd) if emu else t

    shift, scale = sd["scaling_layer.shift"].to(wd).view(1, 3, 1, 1), sd["scaling_layer.scale"].to(wd).view(1, 3, 1, 1)
    feats = []
    for x in (in0, in1):
        x = x.to(wd)
        if normalize or pm1:
            x = 2 * x - 1
        if not no_scaling:
            x = (x - shift) / scale
        x = rnd(x)
        taps = []
        for s, idxs in enumerate(SLICES, 1):
            if s > 1:
                x = F.max_pool2d(x, 2, 2, ceil_mode=ceil_pool)
            for j, i in enumerate(idxs):
                w, b = sd["net.slice%d.%d.weight" % (s, i)], sd["net.slice%d.%d.bias" % (s, i)]
                pre = rnd(F.conv2d(x, rnd(w.to(wd)), b.to(wd), padding=1))
                x = F.relu(pre)
            taps.append(pre if pre_relu else x)
        feats.append(taps)
    return torch.stack([layer_distance(a, b, sd["lin%d.model.1.weight" % l].reshape(-1), eps_inside)
                        for l, (a, b) in enumerate(zip(*feats))], 1)


def lpips(sd, in0, in1, **kw):
    """[N] fp64: the sum of the five layer values."""
    return lpips_layers(sd, in0, in1, **kw).sum(1)


# ---- the cases of the end-to-end tests (tests/test_lpips_gpu.py; tests/test_lpips_host.py shows that they separate)
CASES = ((6, 44, 28), (2, 16, 16))  # 44x28 -> 22x14 -> 11x7 -> 5x3 -> 2x1: odd floors and a one-pixel-row tail


def make_pairs(n, h, w, seed=0):
    """uint8 [n, h, w, 3] x 2: a random picture (smooth colour field + texture) and a blurred, noised copy of it."""
    rng = np.random.RandomState(1000 * seed + 7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 6.28, (n, 1, 1, 3))
    fr = rng.uniform(3.0, 9.0, (n, 1, 1, 3))
    base = 128 + 70 * np.sin(yy[None, :, :, None] / fr + ph) * np.cos(xx[None, :, :, None] / (0.7 * fr) + 2 * ph)
    a = base + 40 * rng.standard_normal((n, h, w, 3))
    a = np.clip(np.rint(a), 0, 255)
    t = torch.from_numpy(a).permute(0, 3, 1, 2)
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    k = (k[:, None] * k[None, :] / 16).view(1, 1, 3, 3).repeat(3, 1, 1, 1)
    blur = F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), k, groups=3).permute(0, 2, 3, 1).numpy()
    b = np.clip(np.rint(blur + 12 * rng.standard_normal((n, h, w, 3))), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def to_unit(u8, dtype=torch.float64):
    """uint8 [N, H, W, 3] -> [N, 3, H, W] = u / 255 (T.ToTensor)."""
    return torch.from_numpy(u8).permute(0, 3, 1, 2).to(dtype) / 255


_CACHE = {}


def case_refs(sd, key="default"):
    """[(a, b, ref64 [n, 5], emu16 [n, 5])] of CASES and gap = max |emu16 - ref64| / ref64 over every pair and layer;
    computed once per state dict `key` and shared."""
    if key not in _CACHE:
        out, gap = [], 0.0
        for n, h, w in CASES:
            a, b = make_pairs(n, h, w)
            r = lpips_layers(sd, to_unit(a), to_unit(b))
            e = lpips_layers(sd, to_unit(a, torch.float32), to_unit(b, torch.float32), mode="emu16")
            gap = max(gap, float(((e - r).abs() / r).max()))
            out.append((a, b, r, e))
        _CACHE[key] = (out, gap)
    return _CACHE[key]


# ---- the layer kernel's cases: C x hw, N = 3
LAYER_C = (64, 128, 256, 512)
LAYER_HW = (1, 2, 15, 176)


def layer_features(c, hw, n=3, seed=0):
    """fp16 [n, hw, c] x 2 post-ReLU-like features (about half of the entries zero) and w [c] fp32.  From two pixels on,
    pixel 1 is all zero in both pictures (it must add 0, not NaN); from 15 pixels on a quarter of the pixels (index % 4
    == 2) hold multiples of 2^-24 below 2^-21, fp16 subnormals that are exact inputs: their norms are of the order of
    the eps, which is what tells `sqrt(s) + eps` from `sqrt(s + eps)`."""
    g = torch.Generator().manual_seed(97 * c + hw + 7919 * seed)
    f = [torch.relu(torch.randn(n, hw, c, generator=g)) * 1.5 for _ in range(2)]
    if hw >= 15:
        tiny = torch.arange(hw) % 4 == 2
        for t in f:
            t[:, tiny] = torch.randint(0, 8, (n, int(tiny.sum()), c), generator=g).float() * 2.0 ** -24
    if hw >= 2:
        for t in f:
            t[:, 1] = 0
    w = torch.rand(c, generator=g) / c
    return f[0].half(), f[1].half(), w


def layer_ref(f0, f1, w, **kw):
    """[n] fp64 from [n, hw, c] fp16 features."""
    return layer_distance(f0.permute(0, 2, 1).unsqueeze(-1), f1.permute(0, 2, 1).unsqueeze(-1), w, **kw)


def layer_bound(c, hw):
    """Relative: every term is non-negative, so any fp32 summation order of the c * hw terms stays within (c hw) 2^-23 of
    their exact sum, plus 16 roundings for the element-wise operations of a term."""
    return (c * hw + 16) * 2.0 ** -23
