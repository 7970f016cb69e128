"""DDPM / LatentDiffusion / DiffusionWrapper — the inference and validation call surface of
ldm/models/diffusion/ddpm.py.

What is CONTRACT here (and therefore kept name for name): the constructor keyword arguments, so that the `model:`
block of configs/deepfashion/bbox.yaml instantiates unchanged; the module / buffer names that make reference
checkpoints load (model.diffusion_model.*, model_ema.*, first_stage_model.*, cond_stage_model.*, extra_cond_models.*,
the schedule buffers); the methods the named callers use (apply_model, decode_first_stage, get_learned_conditioning,
ema_scope, q_sample, sample_log, log_images, test_step, get_input, get_loss, p_losses, forward, shared_step,
validation_step) with their argument order and return shapes.  Everything else is this package's own: the schedule
buffers come out of one table, conditioning assembly lives in one place (`_conditioning`), EMA evaluation packs the
shadow weights instead of copying them over the live ones.

The LOSS side exists as far as evaluating it goes: loss_type, l_simple_weight, original_elbo_weight,
learn_logvar and logvar_init are honoured, `lvlb_weights` and `logvar` exist as in the reference, and p_losses / forward /
shared_step / validation_step compute the reference's loss_dict — forward only, through upk_q_sample_f32 and
upk_p_losses_f32 around the UNet forward.  There is no backward pass, no optimizer and no EMA update: training_step and
configure_optimizers raise, scheduler_config is accepted and ignored.

Plain torch.nn.Modules (no pytorch_lightning); every FLOP of the denoiser / first stage runs in the HIP engine.
"""
import threading
from contextlib import contextmanager

import numpy as np
import torch
from torch import nn

from .ancestral import AncestralSampling
from .config import count_params, instantiate_from_config, to_plain
from .ddim import DDIMSampler
from .ema import LitEma
from .grid import make_grid
from .schedule import extract_into_tensor, make_beta_schedule
from .vae import AutoencoderKL
from . import _lib
from ._check import require


_EMA_LOCK = threading.Lock()
_LAST_KEYED = threading.local()  # .terms: (t, loss_terms) of the calling thread's last keyed p_losses (lanes share the model)


def disabled_train(self, mode=True):
    return self


class DiffusionWrapper(nn.Module):
    """ddpm.py:1550-1577."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        require(self.conditioning_key in [None, "concat", "crossattn", "hybrid", "adm"], "unknown conditioning_key %r" % (self.conditioning_key,), ValueError)

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None):
        key = self.conditioning_key
        if key is None:
            return self.diffusion_model(x, t)
        if key == "concat":
            return self.diffusion_model(torch.cat([x] + c_concat, dim=1), t)
        if key == "crossattn":
            return self.diffusion_model(x, t, context=torch.cat(c_crossattn, 1))
        if key == "hybrid":
            # c_crossattn is a TENSOR in the hybrid branch (ddpm.py:1569): a None c_concat
            # raises TypeError exactly like the reference
            return self.diffusion_model(torch.cat([x] + c_concat, dim=1), t, context=torch.cat([c_crossattn], 1))
        if key == "adm":
            return self.diffusion_model(x, t, y=c_crossattn[0])
        raise NotImplementedError()


# Persistent schedule buffers (checkpoint keys, ddpm.py:125-146) as functions of (betas, alphas_cumprod,
# alphas_cumprod_prev), evaluated in float64 and stored as fp32 like the reference does.
_SCHEDULE = (
    ("betas", lambda b, a, p: b),
    ("alphas_cumprod", lambda b, a, p: a),
    ("alphas_cumprod_prev", lambda b, a, p: p),
    ("sqrt_alphas_cumprod", lambda b, a, p: np.sqrt(a)),
    ("sqrt_one_minus_alphas_cumprod", lambda b, a, p: np.sqrt(1.0 - a)),
    ("log_one_minus_alphas_cumprod", lambda b, a, p: np.log(1.0 - a)),
    ("sqrt_recip_alphas_cumprod", lambda b, a, p: np.sqrt(1.0 / a)),
    ("sqrt_recipm1_alphas_cumprod", lambda b, a, p: np.sqrt(1.0 / a - 1)),
    ("posterior_variance", lambda b, a, p: b * (1.0 - p) / (1.0 - a)),
    ("posterior_log_variance_clipped", lambda b, a, p: np.log(np.maximum(b * (1.0 - p) / (1.0 - a), 1e-20))),
    ("posterior_mean_coef1", lambda b, a, p: b * np.sqrt(p) / (1.0 - a)),
    ("posterior_mean_coef2", lambda b, a, p: (1.0 - p) * np.sqrt(1.0 - b) / (1.0 - a)),
)


def _load_weights(module, path, drop_prefixes=(), what="checkpoint"):
    """Reads a (Lightning) checkpoint, drops keys by prefix, loads non-strictly and reports what did not match.
    The files are trusted pickles with hparams / callback objects inside, hence weights_only=False."""
    blob = torch.load(path, map_location="cpu", weights_only=False)
    state = blob.get("state_dict", blob) if isinstance(blob, dict) else blob
    kept = {}
    for name, tensor in state.items():
        if name.startswith(tuple(drop_prefixes)) and drop_prefixes:
            print("Deleting key {} from state_dict.".format(name))
        else:
            kept[name] = tensor
    result = module.load_state_dict(kept, strict=False)
    print(f"Restored {what} from {path} with {len(result.missing_keys)} missing and "
          f"{len(result.unexpected_keys)} unexpected keys")
    for label, keys in (("Missing", result.missing_keys), ("Unexpected", result.unexpected_keys)):
        if keys:
            print(f"{label} Keys: {list(keys)}")
    return result


class DDPM(nn.Module):
    """ddpm.py:50-210: denoiser wrapper + EMA shadow + noise schedule."""

    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", loss_type="l2", ckpt_path=None,
                 ignore_keys=[], load_only_unet=False, monitor="val/loss", use_ema=True, first_stage_key="image",
                 image_size=256, crop_size=[256, 176], channels=3, log_every_t=100, clip_denoised=True,
                 linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3, given_betas=None, original_elbo_weight=0.,
                 v_posterior=0., l_simple_weight=1., conditioning_key=None, parameterization="eps",
                 scheduler_config=None, use_positional_encodings=False, learn_logvar=False, logvar_init=0.):
        super().__init__()
        if parameterization not in ("eps", "x0"):
            raise AssertionError('currently only supporting "eps" and "x0"')
        if v_posterior:
            raise NotImplementedError("v_posterior != 0 changes the posterior variance buffers; not used by UPGPT")
        # loss_type, original_elbo_weight, l_simple_weight, learn_logvar and logvar_init shape the loss values of
        # p_losses / validation_step; scheduler_config configures the training loop of the reference and does nothing
        # here; monitor and log_every_t are the plain attributes its scripts read (main.py:653 model.monitor,
        # classifier.py:204 diffusion_model.log_every_t)
        self.loss_type, self.monitor, self.log_every_t = loss_type, monitor, log_every_t
        self.v_posterior, self.original_elbo_weight, self.l_simple_weight = v_posterior, original_elbo_weight, l_simple_weight
        self.use_scheduler, self.learn_logvar = scheduler_config is not None, learn_logvar
        if self.use_scheduler:
            self.scheduler_config = scheduler_config
        self.parameterization, self.first_stage_key = parameterization, first_stage_key
        self.channels, self.crop_size = channels, crop_size
        self.clip_denoised, self.use_positional_encodings = clip_denoised, use_positional_encodings
        self.image_size = [int(v) for v in image_size] if np.ndim(image_size) else [int(image_size)] * 2
        self.cond_stage_model, self.use_ema = None, bool(use_ema)
        print(f"{type(self).__name__}: Running in {parameterization}-prediction mode")
        self.model = denoiser = DiffusionWrapper(unet_config, conditioning_key)
        count_params(denoiser, verbose=True)
        if use_ema:
            self.model_ema = LitEma(denoiser)  # shadow buffers `model_ema.*` of the checkpoints
            print(f"Keeping EMAs of {sum(1 for _ in self.model_ema.buffers())}.")
        self.register_schedule(given_betas, beta_schedule, timesteps, linear_start, linear_end, cosine_s)
        # (ddpm.py:120-122) a checkpoint key only when it is learned; a plain CPU tensor otherwise, as in the reference
        self.logvar = torch.full(fill_value=float(logvar_init), size=(self.num_timesteps,))
        if self.learn_logvar:
            self.logvar = nn.Parameter(self.logvar, requires_grad=True)
        if ckpt_path is not None and type(self) is DDPM:
            self.init_from_ckpt(ckpt_path, ignore_keys, only_model=load_only_unet)

    @property
    def device(self):
        return next(self.parameters()).device

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        betas = np.asarray(given_betas if given_betas is not None else make_beta_schedule(
            beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s),
            dtype=np.float64)
        acp = np.cumprod(1.0 - betas, axis=0)
        acp_prev = np.concatenate([[1.0], acp[:-1]])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        for name, fn in _SCHEDULE:
            self.register_buffer(name, torch.tensor(fn(betas, acp, acp_prev), dtype=torch.float32))
        # (ddpm.py:167-176) the weights of the variational-bound term, formed from the fp32 BUFFERS in fp32, in the
        # reference's operation order, not in float64; entry 0 (posterior_variance[0] = 0: a division by zero) is
        # replaced by entry 1
        if self.parameterization == "eps":
            alphas = torch.tensor(1.0 - betas, dtype=torch.float32)
            lvlb = self.betas ** 2 / (2 * self.posterior_variance * alphas * (1 - self.alphas_cumprod))
        else:
            lvlb = 0.5 * torch.sqrt(self.alphas_cumprod) / (2. * 1 - self.alphas_cumprod)
        lvlb[0] = lvlb[1]
        self.register_buffer("lvlb_weights", lvlb, persistent=False)
        require(not torch.isnan(self.lvlb_weights).all(), "lvlb_weights are all NaN", AssertionError)

    @contextmanager
    def ema_scope(self, context=None, local=False):
        """ddpm.py:179-192.  Inside the scope the denoiser COMPUTES with the LitEma shadow
        weights; they are packed straight from the shadow buffers instead of being copied
        over the live parameters (same results, no 1.7 GB copy + repack per call).
        local=True (an extension): the selection holds for the CALLING THREAD alone and takes precedence over the
        process-wide one (UNetModel.set_weight_local) — a lane thread in the EMA pass of its validation batch leaves the
        other lanes on the weight set they are on.  No lock and no count: the previous selection of the thread is put back."""
        if not self.use_ema:
            yield None
            return
        unet, ema = self.model.diffusion_model, self.model_ema
        sel = ("ema", lambda n: ema.shadow("diffusion_model." + n).data,
               lambda: (sum(b._version for b in ema.buffers()), ema.decay.data_ptr()))
        if local:
            prev = unet.set_weight_local(sel)
            try:
                yield None
            finally:
                unet.set_weight_local(prev)
            return
        # the scope nests and may be entered from several host threads at once (one per execution lane): the override
        # goes in with the first entrant and out with the last
        with _EMA_LOCK:
            n = self.__dict__.get("_ema_depth", 0)
            if n == 0:
                unet.set_weight_override(*sel)
            self.__dict__["_ema_depth"] = n + 1
        if context is not None:
            print(f"{context}: Switched to EMA weights")
        try:
            yield None
        finally:
            with _EMA_LOCK:
                n = self.__dict__["_ema_depth"] = self.__dict__["_ema_depth"] - 1
                if n == 0:
                    unet.set_weight_override(None)
            if context is not None:
                print(f"{context}: Restored training weights")

    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False):
        """ddpm.py:194-210: the whole module, or only the denoiser wrapper."""
        _load_weights(self.model if only_model else self, path, tuple(ignore_keys))

    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:271-274: sqrt(a_t) x0 + sqrt(1 - a_t) noise."""
        if noise is None:
            noise = torch.randn_like(x_start)
        return (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def get_input(self, batch, k):
        """ddpm.py:331-338: NHWC (or HW-only) float image -> contiguous NCHW fp32."""
        x = batch[k]
        if x.dim() == 3:
            x = x.unsqueeze(-1)
        return x.movedim(-1, 1).contiguous().float()

    def get_loss(self, pred, target, mean=True):
        """ddpm.py:276-290: |target - pred| (l1) or (target - pred)^2 (l2), per element or its mean.  Plain tensor
        arithmetic on whatever device the arguments are on; p_losses does not call it (upk_p_losses_f32 forms the
        same terms)."""
        if self.loss_type == "l1":
            loss = (target - pred).abs()
        elif self.loss_type == "l2":
            loss = (target - pred) ** 2
        else:
            raise NotImplementedError("unknown loss type '%s'" % (self.loss_type,))
        return loss.mean() if mean else loss

    def _logvar_table(self, dev):
        """logvar as an fp32 table on `dev`: the Parameter itself when it lives there, else a copy made once per
        (device, version) — the plain tensor stays on the host when the module moves, as in the reference."""
        lv = self.logvar
        if lv.device == dev and lv.dtype == torch.float32:
            return lv.detach()
        key = (dev, lv._version, lv.data_ptr())
        ent = self.__dict__.get("_logvar_dev")
        if ent is None or ent[0] != key:
            ent = self.__dict__["_logvar_dev"] = (key, lv.detach().to(dev, torch.float32))
        return ent[1]

    def training_step(self, *a, **k):
        raise NotImplementedError("training is out of scope of upgpt_amd: the loss is evaluated (p_losses, "
                                  "validation_step), there is no backward pass and no optimizer")

    configure_optimizers = training_step

    def p_losses(self, *a, **k):
        raise NotImplementedError("DDPM.p_losses without conditioning: the UNet here requires a context "
                                  "(LatentDiffusion.p_losses)")

    validation_step = p_losses


class LatentDiffusion(AncestralSampling, DDPM):
    """ddpm.py:433-1547, inference surface; the DDPM ancestral sampler comes from AncestralSampling."""

    def __init__(self, first_stage_config, cond_stage_config, num_timesteps_cond=None, cond_stage_key="image",
                 cond_stage_trainable=False, concat_mode=True, cond_stage_forward=None, conditioning_key=None,
                 scale_factor=1.0, scale_by_std=False, concat_key=None, *args, **kwargs):
        if (num_timesteps_cond or 1) > 1:
            raise NotImplementedError("num_timesteps_cond > 1 (shortened cond schedule) is not on the UPGPT path")
        self.num_timesteps_cond = 1
        require(self.num_timesteps_cond <= kwargs["timesteps"], "num_timesteps_cond > timesteps", ValueError)
        opts = {k: to_plain(v) for k, v in kwargs.items()}
        ckpt_path = opts.pop("ckpt_path", None)
        ignore_keys = opts.pop("ignore_keys", [])
        extra = to_plain(opts.pop("extra_cond_stages", None)) or {}
        key2 = opts.pop("cond_stage_key_2", None)
        first_stage_config, cond_stage_config = to_plain(first_stage_config), to_plain(cond_stage_config)
        if cond_stage_config == "__is_unconditional__":
            conditioning_key = None
        elif conditioning_key is None:
            conditioning_key = "concat" if concat_mode else "crossattn"
        super().__init__(conditioning_key=conditioning_key, *args, **opts)
        self.cond_stage_key, self.cond_stage_key_2 = cond_stage_key, key2
        self.cond_stage_trainable, self.cond_stage_forward = cond_stage_trainable, cond_stage_forward
        self.concat_mode, self.concat_key = concat_mode, concat_key
        self.scale_by_std = scale_by_std
        self.clip_denoised = False
        self.bbox_tokenizer = None  # (ddpm.py:489; only the patch-split first stage, out of scope, would set it)
        try:  # (ddpm.py:476-479)
            self.num_downs = len(first_stage_config["params"]["ddconfig"]["ch_mult"]) - 1
        except (KeyError, TypeError):
            self.num_downs = 0
        if scale_by_std:  # (a buffer then: it is a checkpoint key)
            self.register_buffer("scale_factor", torch.tensor(scale_factor))
        if not scale_by_std:
            self.scale_factor = scale_factor
        # extra conditioning encoders (SMPL / pose projections): module list + the batch key each one reads
        self.extra_cond_keys = [cfg["cond_stage_key"] for cfg in extra.values()]
        self.extra_cond_models = nn.ModuleList(instantiate_from_config(cfg) for cfg in extra.values()) if extra else []
        for build, cfg in ((self.instantiate_first_stage, first_stage_config),
                           (self.instantiate_cond_stage, cond_stage_config)):
            build(cfg)
        self.restarted_from_ckpt = ckpt_path is not None
        if self.restarted_from_ckpt:
            self.init_from_ckpt(ckpt_path, ignore_keys)

    # ---- construction
    @staticmethod
    def _frozen(module, freeze_params):
        module = module.eval()
        module.train = disabled_train
        if freeze_params:
            for p in module.parameters():
                p.requires_grad = False
        return module

    def instantiate_first_stage(self, config):
        self.first_stage_model = self._frozen(instantiate_from_config(config), False)

    def instantiate_cond_stage(self, config):
        """ddpm.py:531-549: a config node, or one of the two sentinels."""
        if config == "__is_unconditional__":
            print(f"Training {type(self).__name__} as an unconditional model.")
            self.cond_stage_model = None
        elif config == "__is_first_stage__":
            print("Using first stage also as cond stage.")
            self.cond_stage_model = self.first_stage_model
        elif self.cond_stage_trainable:
            self.cond_stage_model = instantiate_from_config(config).eval()
        else:
            self.cond_stage_model = self._frozen(instantiate_from_config(config), True)

    # ---- conditioning
    def get_learned_conditioning(self, c):
        """ddpm.py:577-592: run the conditioning stage on `c` — a named method when cond_stage_forward is set,
        else .encode() when the stage has one (a returned distribution is replaced by its mode), else a plain call
        (keyword call for dict input)."""
        stage = self.cond_stage_model
        if self.cond_stage_forward is not None:
            return getattr(stage, self.cond_stage_forward)(c)
        encode = getattr(stage, "encode", None)
        if callable(encode):
            out = encode(c)
            mode = getattr(out, "mode", None)
            return mode() if callable(mode) and not torch.is_tensor(out) else out
        return stage(**c) if isinstance(c, dict) else stage(c)

    def _as_cond_dict(self, cond):
        """tensor / list / dict conditioning -> {'c_concat' | 'c_crossattn': ...} (ddpm.py:962-966)."""
        if isinstance(cond, dict):
            return cond
        slot = "c_concat" if self.model.conditioning_key == "concat" else "c_crossattn"
        return {slot: cond if isinstance(cond, list) else [cond]}

    def _split_cond(self, cond):
        """Any conditioning the callers pass -> (c_concat tensor | None, c_crossattn tensor) for the fused sampler
        path — the rules of apply_model + DiffusionWrapper (ddpm.py:962-971, 1557-1570)."""
        key = self.model.conditioning_key
        cond = self._as_cond_dict(cond)
        cc, ca = cond.get("c_concat"), cond.get("c_crossattn")
        if key == "hybrid":
            if cc is None or any(v is None for v in cc):
                raise TypeError('can only concatenate list (not "NoneType") to list')  # as the reference
            return torch.cat(list(cc), 1), (ca if torch.is_tensor(ca) else torch.cat(ca, 1))
        if key == "crossattn":
            return None, (ca if torch.is_tensor(ca) else torch.cat(ca, 1))
        raise NotImplementedError("fused sampler path for conditioning_key=%r" % key)

    # ---- first stage
    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """ddpm.py:566-575: a posterior is sampled, a tensor is taken as is; both scaled by scale_factor.  `noise` (an
        extension): the standard normals of the posterior sample instead of a generator draw."""
        if torch.is_tensor(encoder_posterior):
            z = encoder_posterior
        elif callable(getattr(encoder_posterior, "sample", None)):
            z = encoder_posterior.sample() if noise is None else encoder_posterior.sample(noise)
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    @torch.no_grad()
    def encode_first_stage(self, x):
        if hasattr(self, "split_input_params"):
            raise NotImplementedError("patch-split first stage (split_input_params) is not used by UPGPT configs")
        return self.first_stage_model.encode(x)

    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        """ddpm.py:771-829, plain branch: (1/scale_factor) * z -> first_stage_model.decode."""
        if predict_cids or hasattr(self, "split_input_params"):
            raise NotImplementedError("predict_cids / split_input_params are not used by UPGPT configs")
        sf = float(self.scale_factor)
        if hasattr(self.first_stage_model, "_decode_plan"):
            return self.first_stage_model.decode(z, scale_factor=sf)  # scaling fused into the input kernel
        return self.first_stage_model.decode(1. / sf * z)

    # ---- denoiser
    def apply_model(self, x_noisy, t, cond, return_ids=False):
        """ddpm.py:962-966, 1057-1063 (non-split branch)."""
        if hasattr(self, "split_input_params"):
            raise NotImplementedError("split_input_params")
        out = self.model(x_noisy, t, **self._as_cond_dict(cond))
        return out[0] if isinstance(out, tuple) and not return_ids else out

    # ---- sampling / logging
    def _conditioning(self, batch, x, cond_key, force_c_encode, bs):
        """(c, original conditioning input): the cross-attention sequence of ddpm.py:718-752 — the main stage on
        batch[cond_key] (text, optionally a {key, key_2} pair), then every extra stage's tokens appended along the
        token axis (styles | smpl for bbox.yaml)."""
        dev = self.device
        on_dev = lambda v: v.to(dev) if torch.is_tensor(v) else v
        cond_key = cond_key or self.cond_stage_key
        if cond_key == self.first_stage_key:
            xc = x
        elif cond_key == "class_label":
            xc = batch
        elif cond_key in ("caption", "coordinates_bbox", "txt"):
            xc = batch[cond_key]
            if self.cond_stage_key_2:
                xc = {cond_key: xc, self.cond_stage_key_2: on_dev(batch[self.cond_stage_key_2])}
        else:
            xc = DDPM.get_input(self, batch, cond_key).to(dev)
        if self.cond_stage_trainable and not force_c_encode:
            c = self.cond_stage_model(**xc)
        else:
            c = self.get_learned_conditioning(on_dev(xc))
        for key, stage in zip(self.extra_cond_keys, self.extra_cond_models):
            c = torch.cat((c, stage.forward(on_dev(batch.get(key)))), 1)
        return (c if bs is None else c[:bs]), xc

    def get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None,
                  return_original_cond=False, bs=None, return_loss_w=False, encode_image=True, noise_keys=None):
        """ddpm.py:684-769 -> [z, {'c_crossattn': c, 'c_concat': [mask]}, (x, xrec)?, (xc)?, (loss_w)?].
        The image is encoded only when an encoder is available.
        noise_keys (upgpt_amd.rng.NoiseKeys, in batch order, at least as many as samples are taken): the posterior sample
        behind z (and with it the reconstruction) is the keyed draw rng.STREAM_POSTERIOR instead of the generator's."""
        dev = self.device
        head = (lambda v: v) if bs is None else (lambda v: v[:bs])
        x = head(DDPM.get_input(self, batch, k)).to(dev)
        z = None
        if encode_image:
            try:
                post = self.encode_first_stage(x)
                if noise_keys is not None and callable(getattr(post, "sample", None)):
                    from . import rng
                    nz = rng.randn(noise_keys[:x.shape[0]], tuple(post.mean.shape), rng.STREAM_POSTERIOR)
                    z = self.get_first_stage_encoding(post, noise=nz).detach()
                else:
                    z = self.get_first_stage_encoding(post).detach()
            except NotImplementedError:
                pass
        c = xc = mask = None
        if self.model.conditioning_key is not None:
            if self.concat_key:
                mask = head(batch[self.concat_key]).to(dev)
            c, xc = self._conditioning(batch, x, cond_key, force_c_encode, bs)
        out = [z, {"c_crossattn": c, "c_concat": [mask]}]
        if return_first_stage_outputs:
            out += [x, None if z is None else self.decode_first_stage(z)]
        if return_original_cond:
            out.append(xc)
        if return_loss_w:
            out.append(batch.get("loss_w", None))
        return out

    # ---- the validation loss
    @torch.no_grad()
    def p_losses(self, x_start, cond, t, noise=None, loss_w=None, noise_keys=None):
        """ddpm.py:1083-1123 -> (loss, loss_dict), forward only.  loss_dict has the reference's keys under its prefix
        ('train' if self.training else 'val'): <prefix>/loss_simple, <prefix>/loss_vlb, <prefix>/loss, and with
        learn_logvar also <prefix>/loss_gamma and 'logvar'; the values are 0-dim fp32 device tensors.
        x_start [B, C, H, W]; t [B] integer timesteps; noise defaults to randn_like(x_start) on the device; loss_w is
        None, [B, 1, H, W] (what the loader makes) or [B, C, H, W].  Target: noise ('eps') or x_start ('x0').
        Path: upk_q_sample_f32 writes a_t x0 + s_t noise straight into the forward plan's stem input (fp16 NHWC, no
        fp32 x_noisy is kept), the plan's loader puts the concat channels behind it, the UNet runs with one timestep
        per sample, and upk_p_losses_f32 reduces its fp32 output against the target (fixed-order fp64 sums, no
        atomics): three launches around the forward and no host synchronisation.  self.loss_terms keeps the kernel's
        whole output of the last call: {loss, loss_simple, loss_gamma, loss_vlb}, then {simple, plain} per sample.
        noise_keys (upgpt_amd.rng.NoiseKeys, one key per sample, in batch order; an extension): the noise is the keyed
        draw rng.STREAM_LOSS_NOISE made INSIDE upk_q_sample_keyed_f32, which takes the place of randn_like and
        upk_q_sample_f32 — no noise table, no generator.  t may then be None: the timesteps are the keyed draw
        rng.STREAM_TIMESTEP of the same launch; a given t is honoured.  self.loss_t keeps the int32 [B] timesteps of the
        last keyed call.  Keys together with noise= (both name the noise) or in another number than B: ValueError.
        NOT reproduced: the reference's `image = self.decode_first_stage(model_output)` (its line 1089) decodes the
        model output to a picture and drops it; nothing is decoded here."""
        from . import rng
        require(x_start.dim() == 4, "p_losses: x_start [B, C, H, W] and t [B]", ValueError)
        rng.check_keys(noise_keys, x_start.shape[0])  # (the argument checks come before any device work)
        require(noise_keys is None or noise is None, "noise_keys and noise both name the noise: give one", ValueError)
        unet = self.model.diffusion_model
        dev = unet._device()  # (RuntimeError on a CPU model: there is no CPU fallback)
        require(t is not None or noise_keys is not None, "p_losses: t may be None only with noise_keys", ValueError)
        require(t is None or t.shape[0] == x_start.shape[0], "p_losses: x_start [B, C, H, W] and t [B]", ValueError)
        require(self.loss_type in ("l1", "l2"), "unknown loss type '%s'" % (self.loss_type,), NotImplementedError)
        B, C, H, W = x_start.shape
        cc, ca = self._split_cond(cond)
        ncat = 0 if cc is None else cc.shape[1]
        require(C + ncat == unet.in_channels and C == unet.out_channels, lambda: "latent %d + concat %d channels against "
                "a UNet of %d in, %d out" % (C, ncat, unet.in_channels, unet.out_channels), ValueError)
        pl = unet.plan(B, H, W, ca.shape[1], B, "forward")
        ctx, n_t = pl.ctx, self.num_timesteps
        with torch.cuda.device(dev):
            x_start = x_start.to(dev, torch.float32).contiguous()
            wc = 0
            if loss_w is not None:
                wc = 1 if loss_w.dim() == 4 and loss_w.shape[1] == 1 else C
                loss_w = loss_w.to(dev, torch.float32).expand(B, wc, H, W).contiguous()
            if noise_keys is None:
                noise = torch.randn_like(x_start) if noise is None else noise.to(dev, torch.float32).contiguous()
                require(noise.shape == x_start.shape, "p_losses: noise and x_start differ in shape", ValueError)
                t32 = t.to(dev, torch.int32).contiguous()
                ctx.q_sample(x_start, noise, t32, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, n_t, None,
                             pl.xin.t, pl.xin.ld, B, C, H * W)
            else:
                eps = self.parameterization == "eps"
                noise = torch.empty_like(x_start) if eps else None  # (an x0 model has no use for the noise itself)
                t32 = torch.empty(B, dtype=torch.int32, device=dev)
                t_in = None if t is None else t.to(dev, torch.int32).contiguous()
                ctx.q_sample_keyed(noise_keys.keys, noise_keys.draw, x_start, t_in, self.sqrt_alphas_cumprod,
                                   self.sqrt_one_minus_alphas_cumprod, n_t, t32, noise, None, pl.xin.t, pl.xin.ld, B, C, H * W)
                self.__dict__["loss_t"] = t32
                _LAST_KEYED.terms = None
            if cc is not None:
                pl.load_x_nchw(cc, C, pl.cin_pad)
            pl.t_rows.copy_(t32)
            pl._t_rows_key = None  # (a sampler sharing this plan re-uploads its rows)
            pl.load_context(ca)
            pl.prep.run()
            pl.body.run()
            target = noise if self.parameterization == "eps" else x_start
            nbytes = ctx.p_losses_ws_bytes(B, C, H * W)
            require(nbytes > 0, "upk_p_losses_ws_bytes refused (%d, %d, %d)" % (B, C, H * W), RuntimeError)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(4 + 2 * B, dtype=torch.float32, device=dev)
            logvar = self._logvar_table(dev)
            ctx.p_losses(pl.eps, target, loss_w, wc, t32, logvar, self.lvlb_weights, n_t,
                         _lib.LOSS_L1 if self.loss_type == "l1" else _lib.LOSS_L2, self.l_simple_weight,
                         self.original_elbo_weight, out, B, C, H * W, ws, nbytes)
            prefix = "train" if self.training else "val"
            loss_dict = {prefix + "/loss_simple": out[1]}
            if self.learn_logvar:
                loss_dict[prefix + "/loss_gamma"] = out[2]
                loss_dict["logvar"] = logvar.mean()
            loss_dict[prefix + "/loss_vlb"] = out[3]
            loss_dict[prefix + "/loss"] = out[0]
            self.__dict__["loss_terms"] = out  # (the kernel's whole output of the last call, for diagnostics)
            if noise_keys is not None:
                _LAST_KEYED.terms = (t32, out)
        return out[0], loss_dict

    def forward(self, x, c, *args, noise_keys=None, **kwargs):
        """ddpm.py:941-950: one uniformly drawn timestep per sample (on the device), then p_losses.  With noise_keys the
        timesteps are the keyed draw of p_losses' own launch and the torch generator is not read."""
        if self.model.conditioning_key is not None:
            require(c is not None, "a conditional model needs its conditioning", AssertionError)
        if noise_keys is not None:
            return self.p_losses(x, c, None, *args, noise_keys=noise_keys, **kwargs)
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=self.device).long()
        return self.p_losses(x, c, t, *args, **kwargs)

    def shared_step(self, batch, noise_keys=None, **kwargs):
        """ddpm.py:931-939.  noise_keys: the posterior sample, the timesteps and the noise are keyed draws."""
        if noise_keys is None:
            x, c, w = self.get_input(batch, self.first_stage_key, return_loss_w=True)
            return self(x, c, loss_w=w)
        x, c, w = self.get_input(batch, self.first_stage_key, return_loss_w=True, noise_keys=noise_keys)
        return self(x, c, loss_w=w, noise_keys=noise_keys)

    PER_SAMPLE = "per_sample"  # validation_step(noise_keys=): the key of the per-sample table in the returned dict

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, noise_keys=None):
        """ddpm.py:364-371: the loss_dict of the live weights and, under the suffix '_ema', of the EMA weights (inside
        ema_scope()).  The reference hands both to Lightning's log_dict (on_epoch means); here the merged dict is
        RETURNED (evaluate.run_validation forms the epoch means) and also passed to self.log_dict when the instance
        has one.  The encoder moments and the conditioning are computed once and shared by the two passes; each pass
        draws its own posterior sample, timesteps and noise, in the reference's order (live first).
        noise_keys (upgpt_amd.rng.NoiseKeys, one key per sample, in batch order): the three draws of a pass are keyed —
        the posterior sample (rng.STREAM_POSTERIOR), the timesteps and the noise (upk_q_sample_keyed_f32) — with
        noise_keys.fork(0) for the live pass and fork(1) for the EMA pass, so a sample meets the same draws whatever
        batch it falls into, and the torch generator is not read.  The EMA pass selects the shadow weights for the
        calling thread alone (ema_scope(local=True)): lanes may sit on different weight sets.  The returned dict then
        ALSO holds, under the key 'per_sample' (LatentDiffusion.PER_SAMPLE), a device fp64 tensor [B, 6] with the columns
        t, simple, plain, t_ema, simple_ema, plain_ema of every sample; that entry is NOT a loss, is not handed to
        log_dict and is left out of the epoch reduction (evaluate.run_validation forms the epoch means FROM it)."""
        from . import rng
        rng.check_keys(noise_keys, batch[self.first_stage_key].shape[0])
        dev = self.model.diffusion_model._device()
        x = DDPM.get_input(self, batch, self.first_stage_key).to(dev)
        posterior = self.encode_first_stage(x)
        _, c, w = self.get_input(batch, self.first_stage_key, return_loss_w=True, encode_image=False)
        if noise_keys is None:
            _, merged = self(self.get_first_stage_encoding(posterior).detach(), c, loss_w=w)
            with self.ema_scope():
                _, ema = self(self.get_first_stage_encoding(posterior).detach(), c, loss_w=w)
            rows = None
        else:
            unet = self.model.diffusion_model
            B = x.shape[0]
            rows = torch.empty(B, 6, dtype=torch.float64, device=dev)

            def one_pass(j):
                keys = noise_keys.fork(j)
                nz = rng.randn(keys, tuple(posterior.mean.shape), rng.STREAM_POSTERIOR)
                _, d = self(self.get_first_stage_encoding(posterior, noise=nz).detach(), c, loss_w=w, noise_keys=keys)
                t32, terms = _LAST_KEYED.terms  # (this thread's: self.loss_terms may be another lane's by now)
                rows[:, 3 * j] = t32
                rows[:, 3 * j + 1:3 * j + 3] = terms[4:].view(B, 2)
                return d

            prev = unet.set_weight_local("live")  # (the live pass is live whatever scope the caller sits in)
            try:
                merged = one_pass(0)
            finally:
                unet.set_weight_local(prev)
            with self.ema_scope(local=True):
                ema = one_pass(1)
        merged = dict(merged)
        merged.update({k + "_ema": v for k, v in ema.items()})
        log_dict = getattr(self, "log_dict", None)
        if callable(log_dict):
            log_dict(merged, prog_bar=False, logger=True, on_step=False, on_epoch=True)
        if rows is not None:
            merged[self.PER_SAMPLE] = rows
        return merged

    # ---- sampling / logging (continued)
    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, sampler="ddim", **kwargs):
        """ddpm.py:1312-1325.  sampler (this package's extension; it arrives through log_images' **kwargs, so test_step,
        evaluate.run_test / run_upscale and InferenceModel.generate take it too): "ddim", "dpmpp_2m" for
        DPM-Solver++(2M) on its logSNR grid (dpm_solver.py) or "unipc" for UniPC on the same grid (unipc.py; its order /
        variant / corrector arguments pass through **kwargs, and it refuses a masked chain) — ddim_steps is then the step
        count, and `eta`, DDIM's knob (log_images passes its ddim_eta default of 1), does not apply to the deterministic
        solvers and is dropped.  "dpmpp_2m_sde" is SDE-DPM-Solver++(2M) (dpm_sde.py), which takes `eta` (0 .. 1) and masked
        chains, both on its captured path."""
        require(sampler in ("ddim", "dpmpp_2m", "unipc", "dpmpp_2m_sde"),
                lambda: "sampler %r (ddim, dpmpp_2m, unipc or dpmpp_2m_sde)" % (sampler,), ValueError)
        if not ddim:
            return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)
        shape = (self.channels, *self.image_size)
        if sampler == "dpmpp_2m":
            from .dpm_solver import DPMSolverSampler
            kwargs.pop("eta", None)
            return DPMSolverSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        if sampler == "unipc":
            from .unipc import UniPCSampler
            kwargs.pop("eta", None)
            return UniPCSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        if sampler == "dpmpp_2m_sde":
            from .dpm_sde import DPMSolverSDESampler
            return DPMSolverSDESampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        return DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)

    def _get_denoise_row_from_list(self, samples, desc="", force_no_decoder_quantization=False):
        """ddpm.py:557-567: decode the logged latents, one grid row per sample.  `samples` is DDIM's intermediates dict
        or the list the DDPM loops return (the reference indexes both with 'x_inter' and fails on the list)."""
        zs = samples["x_inter"] if isinstance(samples, dict) else samples
        row = torch.stack([self.decode_first_stage(z.to(self.device)) for z in zs])  # n_log_step, n_row, C, H, W
        return make_grid(row.transpose(0, 1).flatten(0, 1), nrow=row.shape[0])

    @torch.no_grad()
    def log_images(self, batch, N=8, n_row=4, sample=True, ddim_steps=200, ddim_eta=1., return_keys=None,
                   quantize_denoised=False, inpaint=False, plot_denoise_rows=False, plot_progressive_rows=False,
                   plot_diffusion_rows=False, seed=None, noise_keys=None, **kwargs):
        """ddpm.py:1380-1499 — the path InferenceModel.generate drives (generate_utils.py:159-169): conditioning
        assembly -> EMA scope -> DDIM (ddim_steps=None: the DDPM chain) -> decode, and the reference's plotting rows.
        Returns {'reconstruction'?, 'samples', ...}.
        noise_keys (upgpt_amd.rng.NoiseKeys, one key per sample of the batch, in batch order): every sampling call below
        draws keyed noise instead of the device generator's — the keys are cut to the n samples produced, 'samples' uses
        draw 0 (fork(0)), the in- and outpainting draws 1 and 2, the progressive row draw 3.  `seed` keeps its meaning
        (one x_T shared by the batch, from the torch generator); the keys then give the step noise only.  The posterior
        sample of the encoded batch (z: the reconstruction, the inpainting's x0) is keyed as well (rng.STREAM_POSTERIOR,
        draw 0), so with keys log_images reads the torch generator nowhere but in plot_diffusion_rows, which stays on it."""
        use_ddim = ddim_steps is not None
        z, cond, x, xrec, _ = self.get_input(batch, self.first_stage_key, return_first_stage_outputs=True,
                                             force_c_encode=True, return_original_cond=True, bs=N,
                                             **({} if noise_keys is None else {"noise_keys": noise_keys}))
        n = min(x.shape[0], N)
        n_row = min(x.shape[0], n_row)
        keyed = (lambda j: {}) if noise_keys is None else (lambda j: {"noise_keys": noise_keys[:n].fork(j)})
        log = {} if xrec is None else {"reconstruction": xrec}
        require(z is not None or not (plot_diffusion_rows or inpaint),
                "diffusion rows and inpainting need the first stage's encoder", NotImplementedError)
        if plot_diffusion_rows:  # q_sample of the encoded batch along the schedule (ddpm.py:1405-1420)
            z_start = z[:n_row]
            rows = []
            for t in range(self.num_timesteps):
                if t % self.log_every_t == 0 or t == self.num_timesteps - 1:
                    tt = torch.full((n_row,), t, device=self.device, dtype=torch.long)
                    rows.append(self.decode_first_stage(self.q_sample(z_start, tt, noise=torch.randn_like(z_start))))
            rows = torch.stack(rows)  # n_log_step, n_row, C, H, W
            log["diffusion_row"] = make_grid(rows.transpose(0, 1).flatten(0, 1), nrow=rows.shape[0])
        if sample:
            x_T = None
            if seed:  # one seeded latent shared by the batch (ddpm.py:1422-1426)
                torch.manual_seed(seed)
                x_T = torch.randn((1, self.channels, *self.image_size), device=self.device).repeat(n, 1, 1, 1)
            with self.ema_scope("Plotting"):
                samples, z_denoise_row = self.sample_log(cond=cond, batch_size=n, ddim=use_ddim, ddim_steps=ddim_steps,
                                                         eta=ddim_eta, x_T=x_T, **keyed(0), **kwargs)
            log["samples"] = self.decode_first_stage(samples)
            if plot_denoise_rows:
                log["denoise_row"] = self._get_denoise_row_from_list(z_denoise_row)
            # an AutoencoderKL first stage has nothing to quantize: the reference skips the branch (ddpm.py:1452-1454)
            require(not quantize_denoised or isinstance(self.first_stage_model, AutoencoderKL),
                    "quantize_denoised needs a VQ first stage (not on the UPGPT path)", NotImplementedError)
            if inpaint:  # a centre square is filled in (mask 0), the rest is kept (ddpm.py:1463-1484)
                h, w = z.shape[2], z.shape[3]
                mask = torch.ones(n, h, w, device=self.device)
                mask[:, h // 4:3 * h // 4, w // 4:3 * w // 4] = 0.
                mask = mask[:, None, ...]
                # (the masked rows are DDIM's, as the reference's, also under sampler="dpmpp_2m" / "unipc"; the solver with
                # masked chains of its own on the captured path draws them itself)
                own = {"sampler": "dpmpp_2m_sde"} if kwargs.get("sampler") == "dpmpp_2m_sde" else {}
                with self.ema_scope("Plotting Inpaint"):
                    samples, _ = self.sample_log(cond=cond, batch_size=n, ddim=use_ddim, eta=ddim_eta,
                                                 ddim_steps=ddim_steps, x0=z[:n], mask=mask, **keyed(1), **own)
                log["samples_inpainting"] = self.decode_first_stage(samples.to(self.device))
                log["mask"] = mask
                # "outpainting" runs with the SAME mask as the inpainting, as the reference does: a second draw of
                # the same task (its own x_T), not the complementary one
                with self.ema_scope("Plotting Outpaint"):
                    samples, _ = self.sample_log(cond=cond, batch_size=n, ddim=use_ddim, eta=ddim_eta,
                                                 ddim_steps=ddim_steps, x0=z[:n], mask=mask, **keyed(2), **own)
                log["samples_outpainting"] = self.decode_first_stage(samples.to(self.device))
        if plot_progressive_rows:
            with self.ema_scope("Plotting Progressives"):
                _, progressives = self.progressive_denoising(cond, shape=(self.channels, *self.image_size),
                                                             batch_size=n, **keyed(3))
            log["progressive_row"] = self._get_denoise_row_from_list(progressives, desc="Progressive Generation")
        if return_keys and any(k in log for k in return_keys):
            return {k: log[k] for k in return_keys}
        return log

    @torch.no_grad()
    def edit_images(self, batch, keep, N=8, ddim_steps=200, ddim_eta=1., noise_keys=None, **kwargs):
        """Region-locked editing (this package's extension): the batch's pictures are encoded and sampled
        again under the latent keep-mask `keep` [>= n, 1, *image_size] (1 keeps x0, 0 is generated: edit.region_mask's
        second result), with the batch's conditioning -> {'reconstruction', 'samples'} like log_images.  get_input as
        log_images calls it, then the masked chain of sample_log(x0=z, mask=keep) under the EMA scope, then the decoder;
        `kwargs` carry sampler=, the guidance arguments and so on, as in log_images.  noise_keys: draw 4 (fork(4); draws
        0 to 3 belong to log_images), the posterior sample behind z is keyed as there.  The decoded picture differs from
        the input OUTSIDE the region as well (the VAE round trip, and the last step's result is never blended): the
        byte-exact guarantee is edit.composite's, in pixel space."""
        z, cond, x, xrec, _ = self.get_input(batch, self.first_stage_key, return_first_stage_outputs=True,
                                             force_c_encode=True, return_original_cond=True, bs=N,
                                             **({} if noise_keys is None else {"noise_keys": noise_keys}))
        n = min(x.shape[0], N)
        require(z is not None, "region editing needs the first stage's encoder", NotImplementedError)
        require(torch.is_tensor(keep) and keep.dim() == 4 and keep.shape[0] >= n and keep.shape[1] == 1 and
                tuple(keep.shape[2:]) == tuple(self.image_size),
                lambda: "keep must be [>= %d, 1, %d, %d], got %s" % (n, self.image_size[0], self.image_size[1], tuple(
                    keep.shape) if torch.is_tensor(keep) else type(keep).__name__), ValueError)
        keyed = {} if noise_keys is None else {"noise_keys": noise_keys[:n].fork(4)}
        with self.ema_scope("Plotting Edit"):
            samples, _ = self.sample_log(cond=cond, batch_size=n, ddim=ddim_steps is not None, ddim_steps=ddim_steps,
                                         eta=ddim_eta, x0=z[:n], mask=keep[:n].to(self.device, torch.float32), **keyed, **kwargs)
        return {"reconstruction": xrec, "samples": self.decode_first_stage(samples.to(self.device))}

    @torch.no_grad()
    def test_step(self, batch, batch_idx, **log_kwargs):
        """ddpm.py:1327-1377 — what trainer.test runs per batch (main.py:798): sample the batch through log_images and
        write results/{samples,concats,styles,gt,recon,src,smpl}/<fname>.jpg under self.logger.save_dir (a Lightning
        logger, or evaluate.ResultDir(path); without one: ValueError).  Per sample: the generated image, the
        reconstruction, the target, source and SMPL images, all centre-cropped to crop_size (an image smaller than
        crop_size: ValueError, torchvision would zero-pad), their strip src | sample | recon | smpl, and the strip of the
        sample's CLIP-de-normalised style crops (not cropped).  The pictures are finished on the device
        (evaluate.finished_arrays: upk_image_finish_u8 into one uint8 buffer, one copy, one synchronise) and encoded by
        PIL with its default JPEG settings.  Returns None.
        log_images is called with N=len(batch), as the reference calls it: len of the batch DICT, the number of its
        KEYS, not of its samples — that many samples are produced at most, and (through zip) that many per-sample files
        written; the styles strips are written for every fname.  Kept as it is.  `log_kwargs` (ddim_steps=50,
        ddim_eta=0., seed=...) is this package's extension, laid over the reference's arguments
        (unconditional_guidance_scale=3.0, unconditional_guidance_label=["txt"], use_ema=self.use_ema); without it
        log_images' defaults apply, 200 DDIM steps at eta 1, as in the reference.
        NOT reproduced: the reference replaces batch["image" / "src_image" / "smpl_image"] by their cropped, rescaled
        NCHW tensors in place; the batch is left as it came."""
        from . import evaluate
        return evaluate.test_step(self, batch, batch_idx, **log_kwargs)
