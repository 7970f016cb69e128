"""FID's InceptionV3 on the device: the [N, 2048] pool3 features of pytorch_fid 0.3.0 (`python -m pytorch_fid`, dims = 2048),
the network behind the first line of scripts/eval_metrics.py's metrics.txt (its line 102).  The algorithm is stated in
include/upk.h and DESIGN.md 19.

The weights are the user's: pytorch_fid's pt_inception-2015-12-05-6726825d.pth is not shipped.  FIDInception.from_file(path)
reads it; the state dict of this class has its keys, <Block>.<unit>.conv.weight and <Block>.<unit>.bn.{weight, bias,
running_mean, running_var} for the 94 BasicConv2d units; fc.*, AuxLogits.* and *.num_batches_tracked are ignored where
present, a missing leaf raises KeyError.

Compute is libupk.so only (engine.FidPlan): host tensors raise, there is no CPU fallback.
"""
import torch

from . import _lib
from ._check import require
from .packing import BN_LEAVES, FID_DIMS, inception_units
from .params import ParamTree, weights_fingerprint
from .plancache import PlanCache

RESIZE = 299
MIN_SIDE = 75  # without resizing: the smallest input that leaves a pixel after Mixed_7a
IGNORED_PREFIXES = ("fc.", "AuxLogits.")


def param_shapes():
    shapes = {}
    for name, (cin, cout, kh, kw, _, _, _) in inception_units().items():
        shapes[name + ".conv.weight"] = (cout, cin, kh, kw)
        for leaf in BN_LEAVES:
            shapes[name + "." + leaf] = (cout,)
    return shapes


def filter_state(state_dict):
    """The entries of a pytorch_fid / torchvision-style state dict that this class holds; a missing one raises KeyError."""
    sd = {k: v for k, v in state_dict.items() if not k.startswith(IGNORED_PREFIXES) and not k.endswith(".num_batches_tracked")}
    missing = [k for k in param_shapes() if k not in sd]
    if missing:
        raise KeyError("FIDInception: missing %s" % ", ".join(missing[:8]) + (" ... (%d in all)" % len(missing) if len(missing) > 8 else ""))
    return sd


class FIDInception(ParamTree):
    """pictures_per_pass: a batch is processed in passes of at most that many pictures (activations of one pass: about 25 MB
    per picture at 299 x 299; every row offset stays inside 32 bits)."""

    def __init__(self, pictures_per_pass=32):
        super().__init__(param_shapes())
        require(int(pictures_per_pass) >= 1, "pictures_per_pass must be positive", ValueError)
        self.pictures_per_pass = int(pictures_per_pass)
        self._packed = None
        self._plans = PlanCache(4, tuned=False)

    @classmethod
    def from_file(cls, path, pictures_per_pass=32):
        m = cls(pictures_per_pass)
        m.load_state_dict(torch.load(str(path), map_location="cpu", weights_only=True))
        return m

    def load_state_dict(self, state_dict, strict=True, **kw):
        """pytorch_fid's FIDInceptionV3 state dict (or torchvision's inception_v3 keys): fc.*, AuxLogits.* and
        *.num_batches_tracked are dropped; every leaf of param_shapes() must be there (KeyError), whatever `strict` says: a
        metric from half-initialised weights is worthless."""
        return super().load_state_dict(filter_state(state_dict), strict=strict, **kw)

    # ---- plans
    def _plan(self, pictures, H, W, resize):
        from .engine import FidPlan
        from .packing import PackedInception
        with _lib.PLAN_LOCK:
            p = next(self.parameters())
            require(p.device.type == "cuda", "upgpt_amd.FIDInception runs only on the MI355X HIP path (parameters are on %s); "
                    "there is no CPU fallback" % p.device, RuntimeError)
            ctx = _lib.get_context(p.device)
            fp = weights_fingerprint(self)
            if self._packed is None or self._packed[0] != fp:
                tensors = dict(self.named_parameters())
                with torch.cuda.device(p.device), _lib.host_io():
                    self._packed = (fp, PackedInception(ctx, lambda n: tensors[n].data))
                    torch.cuda.current_stream(p.device).synchronize()  # (packed on this lane's stream, read from every lane's)
                self._plans.drop(device=p.device)
            return self._plans.get((pictures, H, W, bool(resize)),
                                   lambda: FidPlan(ctx, self._packed[1], pictures, H, W, resize), p.device)

    def _features(self, name, x, n, h, w, f32, resize, normalize):
        p = next(self.parameters())
        require(p.device == x.device, "%s: the pictures are on %s, the weights on %s" % (name, x.device, p.device), ValueError)
        out = torch.empty((n, FID_DIMS), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            for i in range(0, n, self.pictures_per_pass):
                k = min(self.pictures_per_pass, n - i)
                plan = self._plan(k, h, w, resize)
                t = x[i:i + k]
                out[i:i + k].copy_(plan.run(t, f32, 0 if f32 else t.stride(1), t.stride(0), normalize))
        return out

    @torch.no_grad()
    def features_u8(self, x):
        """[N, 2048] fp32 on the pictures' device: what pytorch_fid computes for these pictures (read as u / 255, resized to 299
        x 299, 2 x - 1).  x: uint8 device tensor [N, H, W, 3], pixels dense inside a row, any row pitch / sample stride (a
        window of a strip is read in place).  Launches on the current stream, no synchronisation."""
        from .metrics import _check_picture
        n, h, w = _check_picture("FIDInception.features_u8", x)
        return self._features("FIDInception.features_u8", x, n, h, w, False, True, True)

    @torch.no_grad()
    def forward(self, x, resize_input=True, normalize_input=True):
        """pytorch_fid's InceptionV3([3], resize_input, normalize_input)(x)[0], flattened: float [N, 3, H, W] device tensor ->
        [N, 2048] fp32.  resize_input=False needs min(H, W) >= 75."""
        require(torch.is_tensor(x) and x.is_cuda, "FIDInception needs device tensors: there is no CPU fallback for the HIP path",
                RuntimeError)
        require(x.dim() == 4 and x.shape[1] == 3 and x.shape[0] >= 1 and min(x.shape[2:]) >= 1,
                "FIDInception: input must be [N, 3, H, W], got %s" % (tuple(x.shape),), ValueError)
        require(x.is_floating_point(), "FIDInception.forward takes float images (features_u8 takes bytes)", TypeError)
        n, _, h, w = x.shape
        require(resize_input or min(h, w) >= MIN_SIDE, "FIDInception: without resizing min(H, W) must be >= %d, got %d x %d" % (
            MIN_SIDE, h, w), ValueError)
        x = x.float().contiguous()
        return self._features("FIDInception.forward", x, n, h, w, True, bool(resize_input), bool(normalize_input))
