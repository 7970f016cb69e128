"""DDPM ancestral sampling on LatentDiffusion (ddpm.py:224-237, 1125-1310): the single-step methods
(predict_start_from_noise, q_posterior, p_mean_variance, p_sample) and the loops (p_sample_loop, sample,
progressive_denoising) with the reference's signatures and return values.

Fast path: the chain runs on a sampler-mode UNetPlan with one timestep-embedding row per DDPM step; each step — UNet
forward, posterior update (upk_ddpm_step_f32), optional q_sample blend of a mask, refresh of the stem input, step
counter — is replayed from captured HIP graphs (engine.SamplerState kind "ddpm", launched by chain.run: up to
ddim.STEPS_PER_GRAPH steps per graph).  All random draws happen before the loop, one call per draw in the reference's order,
so the device generator ends where the reference leaves it.  Everything the fast path cannot take (tensor conditioning,
score_corrector, noise_dropout) goes step by step through p_sample.
"""
import numbers

import numpy as np
import torch

from . import chain, rng
from . import ddim as _ddim
from ._check import require
from ._lib import DDPM_CLIP, DDPM_X0, get_context
from .ddim import noise_like
from .schedule import ddpm_coefficient_table, extract_into_tensor


def _slice_cond(cond, batch_size):
    """ddpm.py:1208-1212 / 1297-1301: conditioning cut to the batch."""
    if cond is None:
        return None
    if isinstance(cond, dict):
        return {k: cond[k][:batch_size] if not isinstance(cond[k], list) else [c[:batch_size] for c in cond[k]]
                for k in cond}
    return [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]


class AncestralSampling:
    """Mixed into LatentDiffusion: needs apply_model, q_sample, _split_cond and the schedule buffers."""

    # ---- single steps (fp32 torch, the reference's op order)
    def predict_start_from_noise(self, x_t, t, noise):
        """ddpm.py:224-228."""
        return (extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t -
                extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        """ddpm.py:230-237 -> (mean, variance, log_variance_clipped)."""
        mean = (extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start +
                extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return (mean, extract_into_tensor(self.posterior_variance, t, x_t.shape),
                extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape))

    def _model_out(self, x, c, t, score_corrector, corrector_kwargs):
        out = self.apply_model(x, t, c)
        if score_corrector is not None:
            require(self.parameterization == "eps", "score correction needs an eps-parameterised model", AssertionError)
            out = score_corrector.modify_score(self, out, x, t, c, **(corrector_kwargs or {}))
        return out

    @staticmethod
    def _no_quantize(quantize_denoised, return_codebook_ids=False):
        if return_codebook_ids:
            raise DeprecationWarning("Support dropped.")
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs a VQ first stage (not on the UPGPT path)")

    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False,
                        return_x0=False, score_corrector=None, corrector_kwargs=None):
        """ddpm.py:1125-1155."""
        self._no_quantize(quantize_denoised, return_codebook_ids)
        model_out = self._model_out(x, c, t, score_corrector, corrector_kwargs)
        x_recon = self.predict_start_from_noise(x, t=t, noise=model_out) if self.parameterization == "eps" else model_out
        if clip_denoised:
            x_recon.clamp_(-1., 1.)
        mean, var, logvar = self.q_posterior(x_start=x_recon, x_t=x, t=t)
        return (mean, var, logvar, x_recon) if return_x0 else (mean, var, logvar)

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_codebook_ids=False,
                 quantize_denoised=False, return_x0=False, temperature=1., noise_dropout=0., score_corrector=None,
                 corrector_kwargs=None, noise=None, noise_keys=None):
        """ddpm.py:1157-1187.  `noise` (an extension): the standard normals of this step instead of a draw.  With one
        t for the whole batch the update is one upk_ddpm_step_f32 launch; per-sample t go through torch.
        noise_keys (without `noise`; one t for the batch): the keyed normals of the step at timestep t, row
        num_timesteps - 1 - t of rng.STREAM_STEP — the row the full chain uses for it."""
        require(noise_keys is None or not repeat_noise,
                "repeat_noise shares one draw over the batch; noise_keys gives every sample its own", ValueError)
        self._no_quantize(quantize_denoised, return_codebook_ids)
        b = x.shape[0]
        if noise is None and noise_keys is not None:
            rng.check_keys(noise_keys, b)
            require(bool((t == t[0]).all()), "noise_keys needs one timestep for the whole batch", ValueError)
            noise = rng.randn(noise_keys, tuple(x.shape), rng.STREAM_STEP, row0=self.num_timesteps - 1 - int(t[0]))
        if bool((t == t[0]).all()):
            model_out = self._model_out(x, c, t, score_corrector, corrector_kwargs)
            if noise is None:
                noise = noise_like(x.shape, x.device, repeat_noise)
            noise = noise.to(x.device) * temperature
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            coefs = ddpm_coefficient_table(self, [int(t[0])]).to(x.device)
            x_prev = x.detach().clone().float().contiguous()
            x0 = torch.empty_like(x_prev)
            flags = (DDPM_X0 if self.parameterization == "x0" else 0) | (DDPM_CLIP if clip_denoised else 0)
            with torch.cuda.device(x.device):
                get_context(x.device).ddpm_step(x_prev, model_out.float().contiguous(), coefs,
                                                noise.float().contiguous(), None, None, None, None, x0, None, 0, b,
                                                x.shape[1], x.shape[2] * x.shape[3], flags)
            return (x_prev, x0) if return_x0 else x_prev
        mean, _, logvar, x0 = self.p_mean_variance(x=x, c=c, t=t, clip_denoised=clip_denoised, return_x0=True,
                                                   score_corrector=score_corrector, corrector_kwargs=corrector_kwargs)
        if noise is None:
            noise = noise_like(x.shape, x.device, repeat_noise)
        noise = noise.to(x.device) * temperature
        if noise_dropout > 0.:
            noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        nonzero_mask = (1 - (t == 0).float()).reshape(b, *((1,) * (len(x.shape) - 1)))
        out = mean + nonzero_mask * (0.5 * logvar).exp() * noise
        return (out, x0) if return_x0 else out

    # ---- loops
    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False,
                              img_callback=None, mask=None, x0=None, temperature=1., noise_dropout=0.,
                              score_corrector=None, corrector_kwargs=None, batch_size=None, x_T=None, start_T=None,
                              log_every_t=None, normals_sequence=None, noise_keys=None):
        """ddpm.py:1189-1244 -> (x, [x0_partial at the logged steps]).  noise_keys: see p_sample_loop."""
        rng.check_keys(noise_keys, shape[0] if batch_size is None else batch_size, normals_sequence)
        if not log_every_t:
            log_every_t = self.log_every_t
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        cond = _slice_cond(cond, batch_size)
        T = self.num_timesteps if start_T is None else min(self.num_timesteps, start_T)
        return self._ancestral(cond, tuple(shape), x_T, T, temperature, mask, x0, normals_sequence, callback,
                               img_callback, log_every_t, True, quantize_denoised, noise_dropout, score_corrector,
                               corrector_kwargs, noise_keys)

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None,
                      timesteps=None, quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None,
                      log_every_t=None, normals_sequence=None, noise_keys=None):
        """ddpm.py:1246-1291 -> x, or (x, [x_T] + [x at the logged steps]).
        noise_keys (upgpt_amd.rng.NoiseKeys, one key per sample): x_T when not given (rng.STREAM_XT, row 0), the
        posterior noise of loop position k (STREAM_STEP, row k) and a mask's q_sample noise (STREAM_QSAMPLE, row k) are
        keyed normals; the torch generator is neither read nor advanced.  Not combinable with normals_sequence."""
        rng.check_keys(noise_keys, shape[0], normals_sequence)
        if not log_every_t:
            log_every_t = self.log_every_t
        T = self.num_timesteps if timesteps is None else timesteps
        if start_T is not None:
            T = min(T, start_T)
        if mask is not None:
            require(x0 is not None, "mask given without x0", AssertionError)
            require(x0.shape[2:3] == mask.shape[2:3], "spatial size has to match", AssertionError)
        img, inter = self._ancestral(cond, tuple(shape), x_T, T, 1., mask, x0, normals_sequence, callback,
                                     img_callback, log_every_t, False, quantize_denoised, 0., None, None, noise_keys)
        return (img, inter) if return_intermediates else img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
               quantize_denoised=False, mask=None, x0=None, shape=None, normals_sequence=None, **kwargs):
        """ddpm.py:1293-1310.  Like the reference, every other keyword (eta, unconditional_guidance_*, callbacks that
        log_images forwards) is dropped — except `noise_keys` (p_sample_loop)."""
        noise_keys = kwargs.get("noise_keys")
        rng.check_keys(noise_keys, batch_size, normals_sequence)
        if shape is None:
            shape = (batch_size, self.channels, *self.image_size)
        return self.p_sample_loop(_slice_cond(cond, batch_size), shape, return_intermediates=return_intermediates,
                                  x_T=x_T, verbose=verbose, timesteps=timesteps, quantize_denoised=quantize_denoised,
                                  mask=mask, x0=x0, normals_sequence=normals_sequence, noise_keys=noise_keys)

    # ---- the chain
    @staticmethod
    def _normals(normals_sequence, T, masked, shape):
        """`normals_sequence`: the standard normals of the chain in the reference's draw order — per step the posterior
        noise, then (with a mask) the q_sample noise: T or 2T tensors of the latent's shape, as a list or one tensor."""
        if normals_sequence is None:
            return None
        ns = normals_sequence if torch.is_tensor(normals_sequence) else torch.stack(list(normals_sequence))
        want = (T * (2 if masked else 1),) + tuple(shape)
        if tuple(ns.shape) != want:
            raise ValueError("normals_sequence must hold %d normals of shape %s (one per draw: %s), got %s"
                             % (want[0], tuple(shape), "posterior, q_sample per step" if masked else "posterior per step",
                                tuple(ns.shape)))
        return ns

    def _fast_ok(self, cond, quantize_denoised, noise_dropout, score_corrector):
        return (cond is not None and isinstance(cond, dict) and not quantize_denoised and noise_dropout <= 0.
                and score_corrector is None and self.model.conditioning_key in ("hybrid", "crossattn")
                and self.device.type == "cuda")

    def _ancestral(self, cond, shape, x_T, T, temperature, mask, x0, normals_sequence, callback, img_callback,
                   log_every_t, log_x0, quantize_denoised, noise_dropout, score_corrector, corrector_kwargs,
                   noise_keys=None):
        """The loop of p_sample_loop (log_x0=False: intermediates [x_T] + x) and progressive_denoising (log_x0=True:
        intermediates x0_partial).  Timesteps T-1 ... 0."""
        self._no_quantize(quantize_denoised)
        T = int(T)
        require(T >= 1, "the chain needs at least one timestep", ValueError)
        temps = [temperature] * T if isinstance(temperature, numbers.Number) else list(temperature)
        require(len(temps) >= T, "temperature: one value per timestep", ValueError)
        masked = mask is not None
        if masked:
            require(x0 is not None, "mask given without x0", AssertionError)
        ns = self._normals(normals_sequence, T, masked, shape)
        if self._fast_ok(cond, quantize_denoised, noise_dropout, score_corrector):
            return self._fast_chain(cond, shape, x_T, T, temps, mask, x0, ns, callback, img_callback, log_every_t,
                                    log_x0, noise_keys)
        device = self.betas.device
        b = shape[0]
        keyed = noise_keys is not None
        img = x_T if x_T is not None else chain.start_latent(None, noise_keys, shape, device)  # (a given x_T stays where it is)
        intermediates = [] if log_x0 else [img]
        for k, i in enumerate(reversed(range(0, T))):
            ts = torch.full((b,), i, device=device, dtype=torch.long)
            nz = None if ns is None else ns[(2 if masked else 1) * k]
            if keyed:
                nz = rng.randn(noise_keys, shape, rng.STREAM_STEP, row0=k)
            img, x0_partial = self.p_sample(img, cond, ts, clip_denoised=self.clip_denoised, return_x0=True,
                                            temperature=temps[i], noise_dropout=noise_dropout,
                                            score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                            noise=nz)
            if masked:
                if keyed:
                    nq = rng.randn(noise_keys, shape, rng.STREAM_QSAMPLE, row0=k)
                else:
                    nq = None if ns is None else ns[2 * k + 1].to(device)
                img_orig = self.q_sample(x0, ts, noise=nq)
                img = img_orig * mask + (1. - mask) * img
            if i % log_every_t == 0 or i == T - 1:
                intermediates.append(x0_partial if log_x0 else img)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        return img, intermediates

    def _fast_chain(self, cond, shape, x_T, T, temps, mask, x0, ns, callback, img_callback, log_every_t, log_x0,
                    noise_keys=None):
        unet = self.model.diffusion_model
        b, C, H, W = shape
        c_concat, c_cross = self._split_cond(cond)
        plan = unet.plan(b, H, W, c_cross.shape[1], T, "sampler")
        dev = plan.dev
        masked = mask is not None
        keyed = noise_keys is not None
        with torch.cuda.device(dev):
            st = plan.sampler_state("ddpm", C)
            st.set_variant(((DDPM_X0 if self.parameterization == "x0" else 0) | (DDPM_CLIP if self.clip_denoised else 0),
                            masked))
            order = np.arange(T)[::-1].copy()  # loop order: timesteps T-1 ... 0 (no +1 as in DDIM)
            rkey = ("ddpm", order.astype(np.float32).tobytes())
            with chain.upload_lock(True):  # (always: T rows of noise, or with keys still the coefficient and temperature rows)
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                plan.load_sampler_inputs(st.x, c_concat, c_cross, unet.in_channels, rkey, order.astype(np.float32))
                st.coefs.copy_(ddpm_coefficient_table(self, order))
                # the draws of the reference, in its order: per step noise_like(x.shape) (also at t = 0, where the row
                # zeroes it), then with a mask q_sample's randn_like(x0).  One call per draw, before the loop.
                nz = st.ensure_noise()
                nz2 = None
                if masked:
                    nz2, sx0, smask = st.ensure_mask()
                    x0d = x0.to(dev, torch.float32)
                    sx0.copy_(x0d.expand(shape).reshape(-1))
                    smask.copy_(mask.to(dev, torch.float32).expand(shape).reshape(-1))
                tv = torch.as_tensor([float(temps[i]) for i in order], dtype=torch.float32)
                if keyed:  # one launch per table; noise_like(...) * temperature[i] is the launch's row scale
                    rng.randn(noise_keys, shape, rng.STREAM_STEP, rows=T, out=nz,
                              scale=tv.to(dev) if bool((tv != 1.).any()) else None)
                    if masked:
                        rng.randn(noise_keys, shape, rng.STREAM_QSAMPLE, rows=T, out=nz2)
                for k in ([] if keyed else range(T)):
                    if ns is not None:
                        nz[k].copy_(ns[2 * k if masked else k].to(dev, torch.float32).reshape(-1))
                        if masked:
                            nz2[k].copy_(ns[2 * k + 1].to(dev, torch.float32).reshape(-1))
                    else:
                        nz[k].copy_(torch.randn(shape, device=dev).reshape(-1))
                        if masked:
                            nz2[k].copy_(torch.randn_like(x0d).expand(shape).reshape(-1))
                # noise_like(...) * temperature[i] (ddpm.py:1174), i = T-1-k
                if not keyed and bool((tv != 1.).any()):
                    nz.mul_(tv.to(dev)[:, None])
                plan.step.zero_()
                plan.prep.run()
            intermediates = [] if log_x0 else [st.x.clone()]
            watched = callback is not None or img_callback is not None
            logged = chain.logged_at(T, log_every_t)
            for k in chain.run(st, T, _ddim.STEPS_PER_GRAPH, watched, logged, True):
                i = T - 1 - k  # (the reference's loop variable is the timestep: what it logs by and hands to the callbacks)
                if logged(k):
                    intermediates.append((st.pred_x0 if log_x0 else st.x).clone())
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(st.x.clone(), i)
            return st.x.clone(), intermediates
