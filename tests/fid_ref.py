"""CPU restatement of pytorch_fid 0.3.0's InceptionV3 (dims = 2048, eval mode) in torch; neither pytorch_fid, torchvision nor
scipy is needed.  The algorithm is the one stated in include/upk.h:

  input     u / 255 -> bilinear resize to 299 x 299 (align_corners=False, no antialias) -> 2 x - 1
  unit      Conv2d(bias=False) -> BatchNorm2d(eps=1e-3, eval) -> ReLU
  trunk     Conv2d_1a/2a/2b, max pool, Conv2d_3b/4a, max pool, Mixed_5b..5d (A), 6a (B), 6b..6e (C), 7a (D), 7b (E, avg pool),
            7c (E, MAX pool), mean over the pixels
  avg       avg_pool2d(3, 1, 1, count_include_pad=False)

Modes: "ref64" everything in fp64, the BatchNorm unfolded; "emu16" what the device pipeline stores, apart from summation
order: BatchNorm folded in fp64 with the weight rounded to fp16 and the bias to fp32, the input computed in fp32 and rounded to
fp16, every conv + bias + ReLU computed in fp32 and rounded to fp16, every pool output rounded to fp16, the global mean taken
in fp64 from the fp16 values.

Near misses (keyword switches, all off by default): include_pad (count_include_pad=True), avg_7c (average instead of max
pooling in Mixed_7c), align_corners, no_pm1 (no 2 x - 1), bn_eps (BatchNorm eps 1e-5 via bn_eps=1e-5).
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
A_BLOCKS = (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64))
C_BLOCKS = (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192))
E_BLOCKS = (("Mixed_7b", 1280, "avg"), ("Mixed_7c", 2048, "max"))
NEAR_MISSES = (("include_pad", dict(include_pad=True)), ("avg_7c", dict(avg_7c=True)), ("align_corners", dict(align_corners=True)),
               ("no_pm1", dict(no_pm1=True)), ("bn_eps", dict(bn_eps=1e-5)))


def units():
    """{name: (cin, cout, (kh, kw), stride, (ph, pw))}: the tables of the issue, written out on their own."""
    u = {"Conv2d_1a_3x3": (3, 32, (3, 3), 2, (0, 0)), "Conv2d_2a_3x3": (32, 32, (3, 3), 1, (0, 0)),
         "Conv2d_2b_3x3": (32, 64, (3, 3), 1, (1, 1)), "Conv2d_3b_1x1": (64, 80, (1, 1), 1, (0, 0)),
         "Conv2d_4a_3x3": (80, 192, (3, 3), 1, (0, 0))}
    for n, cin, pf in A_BLOCKS:
        u[n + ".branch1x1"] = (cin, 64, (1, 1), 1, (0, 0))
        u[n + ".branch5x5_1"] = (cin, 48, (1, 1), 1, (0, 0))
        u[n + ".branch5x5_2"] = (48, 64, (5, 5), 1, (2, 2))
        u[n + ".branch3x3dbl_1"] = (cin, 64, (1, 1), 1, (0, 0))
        u[n + ".branch3x3dbl_2"] = (64, 96, (3, 3), 1, (1, 1))
        u[n + ".branch3x3dbl_3"] = (96, 96, (3, 3), 1, (1, 1))
        u[n + ".branch_pool"] = (cin, pf, (1, 1), 1, (0, 0))
    u["Mixed_6a.branch3x3"] = (288, 384, (3, 3), 2, (0, 0))
    u["Mixed_6a.branch3x3dbl_1"] = (288, 64, (1, 1), 1, (0, 0))
    u["Mixed_6a.branch3x3dbl_2"] = (64, 96, (3, 3), 1, (1, 1))
    u["Mixed_6a.branch3x3dbl_3"] = (96, 96, (3, 3), 2, (0, 0))
    h7, v7 = ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0))
    for n, c in C_BLOCKS:
        u[n + ".branch1x1"] = (768, 192, (1, 1), 1, (0, 0))
        u[n + ".branch7x7_1"] = (768, c, (1, 1), 1, (0, 0))
        u[n + ".branch7x7_2"] = (c, c) + h7
        u[n + ".branch7x7_3"] = (c, 192) + v7
        u[n + ".branch7x7dbl_1"] = (768, c, (1, 1), 1, (0, 0))
        u[n + ".branch7x7dbl_2"] = (c, c) + v7
        u[n + ".branch7x7dbl_3"] = (c, c) + h7
        u[n + ".branch7x7dbl_4"] = (c, c) + v7
        u[n + ".branch7x7dbl_5"] = (c, 192) + h7
        u[n + ".branch_pool"] = (768, 192, (1, 1), 1, (0, 0))
    u["Mixed_7a.branch3x3_1"] = (768, 192, (1, 1), 1, (0, 0))
    u["Mixed_7a.branch3x3_2"] = (192, 320, (3, 3), 2, (0, 0))
    u["Mixed_7a.branch7x7x3_1"] = (768, 192, (1, 1), 1, (0, 0))
    u["Mixed_7a.branch7x7x3_2"] = (192, 192) + h7
    u["Mixed_7a.branch7x7x3_3"] = (192, 192) + v7
    u["Mixed_7a.branch7x7x3_4"] = (192, 192, (3, 3), 2, (0, 0))
    h3, v3 = ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))
    for n, cin, _ in E_BLOCKS:
        u[n + ".branch1x1"] = (cin, 320, (1, 1), 1, (0, 0))
        u[n + ".branch3x3_1"] = (cin, 384, (1, 1), 1, (0, 0))
        u[n + ".branch3x3_2a"] = (384, 384) + h3
        u[n + ".branch3x3_2b"] = (384, 384) + v3
        u[n + ".branch3x3dbl_1"] = (cin, 448, (1, 1), 1, (0, 0))
        u[n + ".branch3x3dbl_2"] = (448, 384, (3, 3), 1, (1, 1))
        u[n + ".branch3x3dbl_3a"] = (384, 384) + h3
        u[n + ".branch3x3dbl_3b"] = (384, 384) + v3
        u[n + ".branch_pool"] = (cin, 192, (1, 1), 1, (0, 0))
    return u


UNITS = units()


def expected_shapes():
    """{state-dict key: shape} of the public file's leaves this network reads."""
    out = {}
    for n, (cin, cout, (kh, kw), _, _) in UNITS.items():
        out[n + ".conv.weight"] = (cout, cin, kh, kw)
        for leaf in ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
            out[n + "." + leaf] = (cout,)
    return out


def resize_bilinear(x, oh, ow, align_corners=False):
    """F.interpolate(x, (oh, ow), mode='bilinear') written out: x [N, C, H, W] in its own dtype; the source coordinates and
    weights are formed in fp64 and cast to x's dtype."""
    def axis(n_in, n_out):
        d = torch.arange(n_out, dtype=torch.float64)
        if align_corners:
            s = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else torch.zeros_like(d)
        else:
            s = ((d + 0.5) * n_in / n_out - 0.5).clamp(min=0)
        i0 = s.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return i0, i1, (s - i0).to(x.dtype)

    y0, y1, ly = axis(x.shape[2], oh)
    x0, x1, lx = axis(x.shape[3], ow)
    ly, lx = ly.view(1, 1, -1, 1), lx.view(1, 1, 1, -1)
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def fold(sd, name, eps=BN_EPS):
    """(w', b') in fp64: w g / sqrt(var + eps), beta - mean g / sqrt(var + eps)."""
    s = sd[name + ".bn.weight"].double() / torch.sqrt(sd[name + ".bn.running_var"].double() + eps)
    return sd[name + ".conv.weight"].double() * s.view(-1, 1, 1, 1), sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * s


def features(sd, x, mode="ref64", resize=True, normalize=True, folded=False, include_pad=False, avg_7c=False,
             align_corners=False, no_pm1=False, bn_eps=BN_EPS, trace=None):
    """[N, 2048] fp64.  x: [N, 3, H, W] in [0, 1] (fp64 for ref64; emu16 takes it to fp32, as the device's u / 255 is).
    trace: a dict that receives "sizes" (map side after every trunk stage) and "max" (the largest activation)."""
    assert mode in ("ref64", "emu16")
    emu = mode == "emu16"
    wd = torch.float32 if emu else torch.float64
    sizes, amax = [], [0.0]

    def rnd(t):  # what is stored in fp16 on the device
        amax[0] = max(amax[0], float(t.abs().max()))
        return t.half().to(wd) if emu else t

    def conv(x, name):
        cin, cout, k, s, p = UNITS[name]
        if emu or folded:
            w, b = fold(sd, name, bn_eps)
            w, b = (w.half().to(wd), b.float()) if emu else (w, b)
            return rnd(F.relu(F.conv2d(x, w, b, stride=s, padding=p)))
        y = F.conv2d(x, sd[name + ".conv.weight"].double(), None, stride=s, padding=p)
        y = F.batch_norm(y, sd[name + ".bn.running_mean"].double(), sd[name + ".bn.running_var"].double(),
                         sd[name + ".bn.weight"].double(), sd[name + ".bn.bias"].double(), False, 0.0, bn_eps)
        return rnd(F.relu(y))

    def maxp(x, s, p=0):
        return F.max_pool2d(x, 3, s, p)

    def avgp(x):
        return rnd(F.avg_pool2d(x, 3, 1, 1, count_include_pad=include_pad))

    x = x.to(wd)
    if resize:
        x = resize_bilinear(x, 299, 299, align_corners)
    if normalize and not no_pm1:
        x = 2 * x - 1
    x = rnd(x)
    x = conv(x, "Conv2d_1a_3x3"); sizes.append(x.shape[-1])
    x = conv(x, "Conv2d_2a_3x3"); sizes.append(x.shape[-1])
    x = conv(x, "Conv2d_2b_3x3"); sizes.append(x.shape[-1])
    x = maxp(x, 2); sizes.append(x.shape[-1])
    x = conv(x, "Conv2d_3b_1x1"); sizes.append(x.shape[-1])
    x = conv(x, "Conv2d_4a_3x3"); sizes.append(x.shape[-1])
    x = maxp(x, 2); sizes.append(x.shape[-1])
    for n, _, _ in A_BLOCKS:
        x = torch.cat([conv(x, n + ".branch1x1"),
                       conv(conv(x, n + ".branch5x5_1"), n + ".branch5x5_2"),
                       conv(conv(conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2"), n + ".branch3x3dbl_3"),
                       conv(avgp(x), n + ".branch_pool")], 1)
        sizes.append(x.shape[-1])
    n = "Mixed_6a"
    x = torch.cat([conv(x, n + ".branch3x3"),
                   conv(conv(conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2"), n + ".branch3x3dbl_3"),
                   maxp(x, 2)], 1)
    sizes.append(x.shape[-1])
    for n, _ in C_BLOCKS:
        t = x
        for k in (1, 2, 3, 4, 5):
            t = conv(t, n + ".branch7x7dbl_%d" % k)
        x = torch.cat([conv(x, n + ".branch1x1"),
                       conv(conv(conv(x, n + ".branch7x7_1"), n + ".branch7x7_2"), n + ".branch7x7_3"),
                       t, conv(avgp(x), n + ".branch_pool")], 1)
        sizes.append(x.shape[-1])
    n = "Mixed_7a"
    t = x
    for k in (1, 2, 3, 4):
        t = conv(t, n + ".branch7x7x3_%d" % k)
    x = torch.cat([conv(conv(x, n + ".branch3x3_1"), n + ".branch3x3_2"), t, maxp(x, 2)], 1)
    sizes.append(x.shape[-1])
    for n, _, kind in E_BLOCKS:
        a = conv(x, n + ".branch3x3_1")
        b = conv(conv(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2")
        pooled = avgp(x) if kind == "avg" or avg_7c else maxp(x, 1, 1)
        x = torch.cat([conv(x, n + ".branch1x1"), conv(a, n + ".branch3x3_2a"), conv(a, n + ".branch3x3_2b"),
                       conv(b, n + ".branch3x3dbl_3a"), conv(b, n + ".branch3x3dbl_3b"), conv(pooled, n + ".branch_pool")], 1)
        sizes.append(x.shape[-1])
    if trace is not None:
        trace["sizes"], trace["max"] = sizes, amax[0]
    return x.double().mean((2, 3))


def picture_error(got, ref):
    """e [N] = max_c |got - ref| / max_c |ref| per picture (a ReLU network's single features can be 0)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return (got - ref).abs().amax(1) / ref.abs().amax(1)


# ---- the cases of the end-to-end tests: (name, pictures, H, W, resize)
CASES = (("44x28_resized", 3, 44, 28, True), ("91x83", 2, 91, 83, False), ("75x75", 2, 75, 75, False))
MARGIN = 4  # e(device) <= MARGIN * gap


def make_pictures(n, h, w, seed=0):
    """uint8 [n, h, w, 3]: a smooth colour field plus texture."""
    rng = np.random.RandomState(1000 * seed + 7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 6.28, (n, 1, 1, 3))
    fr = rng.uniform(3.0, 9.0, (n, 1, 1, 3))
    base = 128 + 70 * np.sin(yy[None, :, :, None] / fr + ph) * np.cos(xx[None, :, :, None] / (0.7 * fr) + 2 * ph)
    a = base + 40 * rng.standard_normal((n, h, w, 3))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def to_unit(u8, dtype=torch.float64):
    """uint8 [N, H, W, 3] -> [N, 3, H, W] = u / 255 (T.ToTensor)."""
    return torch.from_numpy(u8).permute(0, 3, 1, 2).to(dtype) / 255


_CACHE = {}


def case_refs(sd, key="default"):
    """({case name: (pictures u8, ref64 [n, 2048], emu16 [n, 2048], largest ref64 activation)}, gap) with gap = the largest
    picture_error(emu16, ref64) over every picture of every case; computed once per state dict `key` and shared."""
    if key not in _CACHE:
        out, gap = {}, 0.0
        with torch.no_grad():
            for name, n, h, w, resize in CASES:
                u8 = make_pictures(n, h, w)
                tr = {}
                r = features(sd, to_unit(u8), resize=resize, trace=tr)
                e = features(sd, to_unit(u8, torch.float32), mode="emu16", resize=resize)
                gap = max(gap, float(picture_error(e, r).max()))
                out[name] = (u8, r, e, tr["max"])
        _CACHE[key] = (out, gap)
    return _CACHE[key]


# ---- bounds of the kernel tests
def conv_bound(ref, absref, k):
    """|device - ref64| <= 2^-11 |ref64| + K 2^-24 conv(|x|, |w|): one fp16 rounding plus fp32 accumulation of K terms."""
    return 2.0 ** -11 * ref.abs() + k * 2.0 ** -24 * absref


CONV_GEOMS = ((3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (1, 1, 1, 0, 0), (5, 5, 1, 2, 2), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0),
              (1, 3, 1, 0, 1), (3, 1, 1, 1, 0))
CONV_CHANNELS = ((3, 32), (48, 64), (80, 192), (160, 160), (448, 384))
CONV_MAPS = ((9, 7), (17, 17))


def conv_cases():
    """[(kh, kw, stride, ph, pw, h, w, batch, cin, cout)]: every geometry with two channel pairs, maps and batches
    alternating, so that every geometry, channel pair, map and batch occurs (18 cases)."""
    out = []
    for g, geom in enumerate(CONV_GEOMS):
        for r in range(2):
            ch = CONV_CHANNELS[(2 * g + r) % len(CONV_CHANNELS)]
            h, w = CONV_MAPS[(g + r) % 2]
            out.append(geom + (h, w, 2 + (g + r + 1) % 2) + ch)
    return out
