"""LPIPS (VGG16) on the device: lpips.LPIPS(net='vgg', version='0.1') in eval mode, the model behind the LPIPS column of
scripts/eval_metrics.py (its line 112).  The algorithm is stated in include/upk.h and DESIGN.md 18.

The weights are the user's: neither file is shipped.  LPIPS.from_files(vgg16_path, lin_path) reads the two public files
(torchvision's vgg16 state dict with features.<i>.{weight,bias}, and lpips' weights/v0.1/vgg.pth with
lin<l>.model.1.weight); load_state_dict takes the full state dict of an lpips.LPIPS module.  The state dict of this class
has exactly lpips' keys:
    scaling_layer.shift, scaling_layer.scale                  [1, 3, 1, 1] buffers
    net.slice<s>.<i>.weight / .bias                           the 13 convolutions, i = torchvision's features index
    lin<l>.model.1.weight                                     [1, C_l, 1, 1], l = 0..4 (lpips' alias lins.<l>.* is accepted)

Compute is libupk.so only (engine.LpipsPlan): host tensors raise, there is no CPU fallback.
"""
import torch

from . import _lib
from ._check import require
from .packing import VGG16_TAP_CHANNELS, vgg16_convs
from .params import ParamNode, ParamTree, weights_fingerprint
from .plancache import PlanCache

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIDE = 16  # 2^4: the fifth tap must have a pixel
N_TAPS = len(VGG16_TAP_CHANNELS)


def param_shapes():
    shapes = {}
    for s, i, cin, cout in vgg16_convs():
        shapes["net.slice%d.%d.weight" % (s, i)] = (cout, cin, 3, 3)
        shapes["net.slice%d.%d.bias" % (s, i)] = (cout,)
    for l, c in enumerate(VGG16_TAP_CHANNELS):
        shapes["lin%d.model.1.weight" % l] = (1, c, 1, 1)
    return shapes


def state_from_files(vgg16_path, lin_path):
    """The lpips-style state dict from torchvision's vgg16 file and lpips' vgg.pth.  classifier.* (and anything else the
    first file holds) is ignored; a missing convolution or lin weight raises KeyError."""
    vgg = torch.load(str(vgg16_path), map_location="cpu", weights_only=True)
    lin = torch.load(str(lin_path), map_location="cpu", weights_only=True)
    sd = {}
    for s, i, _, _ in vgg16_convs():
        for leaf in ("weight", "bias"):
            key = "features.%d.%s" % (i, leaf)
            if key not in vgg:
                raise KeyError("%s: no %r (a torchvision vgg16 state dict is needed)" % (vgg16_path, key))
            sd["net.slice%d.%d.%s" % (s, i, leaf)] = vgg[key]
    for l in range(N_TAPS):
        key, alias = "lin%d.model.1.weight" % l, "lins.%d.model.1.weight" % l
        if key not in lin and alias not in lin:
            raise KeyError("%s: no %r (lpips' weights/v0.1/vgg.pth is needed)" % (lin_path, key))
        sd[key] = lin[key] if key in lin else lin[alias]
    return sd


class LPIPS(ParamTree):
    """pairs_per_pass: a batch is processed in passes of at most that many pairs (activations of one pass: about 60 MB per
    pair of 256 x 176 pictures; every row offset stays inside 32 bits)."""

    def __init__(self, pairs_per_pass=16):
        super().__init__(param_shapes())
        require(int(pairs_per_pass) >= 1, "pairs_per_pass must be positive", ValueError)
        self.pairs_per_pass = int(pairs_per_pass)
        node = ParamNode()
        node.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1))
        node.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1))
        self.add_module("scaling_layer", node)
        self._packed = None
        self._plans = PlanCache(4, tuned=False)

    @classmethod
    def from_files(cls, vgg16_path, lin_path, pairs_per_pass=16):
        m = cls(pairs_per_pass)
        m.load_state_dict(state_from_files(vgg16_path, lin_path), strict=False)  # (the files hold no scaling layer)
        return m

    def load_state_dict(self, state_dict, strict=True, **kw):
        """lpips' own state dict: the `lins.<l>.*` entries are its ModuleList alias of `lin<l>.*` and are folded onto
        them.  strict (default): every key of this module must be there and nothing else; the scaling layer's two
        buffers may be absent only with strict=False."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("lins."):
                l, rest = k[len("lins."):].split(".", 1)
                k = "lin%s.%s" % (l, rest)
                if k in state_dict:
                    continue
            sd[k] = v
        if not strict:  # (a conv or lin weight may never be missing: a metric from half-initialised weights is worthless)
            missing = [k for k in param_shapes() if k not in sd]
            if missing:
                raise KeyError("LPIPS.load_state_dict: missing %s" % ", ".join(missing))
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- plans
    def _plan(self, pairs, H, W):
        from .engine import LpipsPlan, PackedVGG16
        with _lib.PLAN_LOCK:
            p = next(self.parameters())
            require(p.device.type == "cuda", "upgpt_amd.LPIPS runs only on the MI355X HIP path (parameters are on %s); there "
                    "is no CPU fallback" % p.device, RuntimeError)
            ctx = _lib.get_context(p.device)
            fp = weights_fingerprint(self)
            if self._packed is None or self._packed[0] != fp:
                tensors = dict(self.named_parameters())
                tensors.update(dict(self.named_buffers()))
                with torch.cuda.device(p.device), _lib.host_io():
                    self._packed = (fp, PackedVGG16(ctx, lambda n: tensors[n].data))
                    torch.cuda.current_stream(p.device).synchronize()  # (packed on this lane's stream, read from every lane's)
                self._plans.drop(device=p.device)
            return self._plans.get((pairs, H, W), lambda: LpipsPlan(ctx, self._packed[1], pairs, H, W), p.device)

    def _layers(self, name, a, b, n, h, w, f32, normalize):
        """[n, 5] fp32: a, b as _check_pictures / forward validated them."""
        require(min(h, w) >= MIN_SIDE, "%s: LPIPS needs min(H, W) >= %d, got %d x %d" % (name, MIN_SIDE, h, w), ValueError)
        p = next(self.parameters())
        require(p.device == a.device, "%s: the pictures are on %s, the weights on %s" % (name, a.device, p.device), ValueError)
        out = torch.empty((n, N_TAPS), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            for i in range(0, n, self.pairs_per_pass):
                k = min(self.pairs_per_pass, n - i)
                plan = self._plan(k, h, w)
                if f32:
                    srcs = [(t[i:i + k], 0, t.stride(0)) for t in (a, b)]
                else:
                    srcs = [(t[i:i + k], t.stride(1), t.stride(0)) for t in (a, b)]
                out[i:i + k].copy_(plan.run(srcs[0], srcs[1], f32, normalize))
        return out

    @torch.no_grad()
    def pairs_u8(self, a, b):
        """[N, 5] fp32 on the pictures' device: d_l of every pair and tap.  a, b: uint8 device tensors [N, H, W, 3], pixels
        dense inside a row, any row pitch / sample stride (a window of a strip is read in place), read as u / 255: what
        scripts/eval_metrics.py feeds.  Launches on the current stream, no synchronisation."""
        from .metrics import _check_pictures
        n, h, w = _check_pictures("LPIPS.pairs_u8", a, b)
        return self._layers("LPIPS.pairs_u8", a, b, n, h, w, False, False)

    @torch.no_grad()
    def layers(self, in0, in1, normalize=False):
        """[N, 5] fp32: the per-tap values of forward()."""
        require(torch.is_tensor(in0) and torch.is_tensor(in1) and in0.is_cuda and in1.is_cuda,
                "LPIPS needs device tensors: there is no CPU fallback for the HIP path", RuntimeError)
        require(in0.dim() == 4 and in0.shape[1] == 3 and in0.shape == in1.shape and in0.shape[0] >= 1,
                "LPIPS: inputs must be two [N, 3, H, W] tensors of one shape, got %s and %s" % (tuple(in0.shape), tuple(in1.shape)),
                ValueError)
        require(in0.is_floating_point() and in1.is_floating_point(), "LPIPS.forward takes float images (pairs_u8 takes bytes)", TypeError)
        require(in0.device == in1.device, "LPIPS: both inputs must be on one device", ValueError)
        in0, in1 = in0.float().contiguous(), in1.float().contiguous()
        n, _, h, w = in0.shape
        return self._layers("LPIPS.forward", in0, in1, n, h, w, True, bool(normalize))

    def forward(self, in0, in1, normalize=False):
        """lpips.LPIPS.forward(in0, in1, normalize=normalize): float [N, 3, H, W] device tensors -> [N, 1, 1, 1] fp32 (the five
        tap values summed in fp64, rounded once).  normalize=True maps [0, 1] inputs to [-1, 1] first, as lpips does."""
        return self.layers(in0, in1, normalize).double().sum(1).float().view(-1, 1, 1, 1)
