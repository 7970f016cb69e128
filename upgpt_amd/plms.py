"""PLMSSampler — drop-in for ldm.models.diffusion.plms.PLMSSampler: pseudo
linear multistep (Adams-Bashforth on eps) over the same schedule tables as DDIM (eta must be 0).

Fast path (same conditions as DDIMSampler's): ONE captured HIP graph = UNet body + upk_plms_step_f32 +
upk_advance_step, replayed S + 1 times (the first step evaluates the model twice); the eps history ring,
the Adams-Bashforth combination and classifier-free guidance live in the update kernel, the timestep
embeddings of all evaluations are precomputed like DDIM's.  The launches go through chain.run like the other samplers'
(engine.SamplerState kind "plms"), one evaluation per launch: PLMS steps are not grouped.  Anything else (masks, score
correctors, noise dropout) runs on the general path: one UNetModel.forward per model evaluation driven from Python.
"""
import numpy as np
import torch

from . import chain, rng
from ._check import require
from .ddim import DDIMSampler
from .schedule import ddim_coefficient_table

# Adams-Bashforth weights on [e_t, e_{t-1}, e_{t-2}, e_{t-3}] by available history (plms.py:224-234)
_AB = {1: (3 / 2, -1 / 2), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


class PLMSSampler(DDIMSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, **kwargs):
        """`noise_keys=` (through **kwargs; upgpt_amd.rng.NoiseKeys): x_T, when not given, is the keyed draw (STREAM_XT,
        row 0) — the only normals PLMS uses (eta = 0).  The fast path then leaves the torch generator alone: the S + 1
        draws the reference makes and discards are not made."""
        noise_keys = kwargs.get("noise_keys")
        rng.check_keys(noise_keys, batch_size, normals_sequence)
        self._ensure_schedule((int(S), float(eta)), lambda: self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose),
                              verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f"Data shape for PLMS sampling is {size}")
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, noise_dropout=noise_dropout,
                                  temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, noise_keys=noise_keys)

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, noise_keys=None):
        rng.check_keys(noise_keys, shape[0])
        if ddim_use_original_steps or quantize_denoised:
            raise NotImplementedError("PLMS with the original 1000 steps / quantized x0 is not on the UPGPT path")
        device = self.model.betas.device
        b = shape[0]
        timesteps = self._subset(timesteps)
        if self._fast_ok(cond, ddim_use_original_steps, quantize_denoised, mask, noise_dropout, score_corrector,
                         unconditional_guidance_scale, unconditional_conditioning) \
                and len(timesteps) == len(self.ddim_timesteps) and temperature == 1.:
            return self._fast_plms(cond, shape, x_T, timesteps, callback, img_callback, log_every_t,
                                   unconditional_guidance_scale, unconditional_conditioning, noise_keys)
        img = chain.start_latent(x_T, noise_keys, shape, device)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        time_range = np.flip(timesteps)
        total = timesteps.shape[0]
        print(f"Running PLMS Sampling with {total} timesteps")
        history = []  # newest last, at most 3 entries
        for i, step in enumerate(time_range):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=device,
                                 dtype=torch.long)
            if mask is not None:
                require(x0 is not None, "mask given without x0", ValueError)
                img = self.model.q_sample(x0, ts) * mask + (1. - mask) * img
            img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, temperature=temperature,
                                                   noise_dropout=noise_dropout, score_corrector=score_corrector,
                                                   corrector_kwargs=corrector_kwargs,
                                                   unconditional_guidance_scale=unconditional_guidance_scale,
                                                   unconditional_conditioning=unconditional_conditioning,
                                                   old_eps=history, t_next=ts_next)
            history = (history + [e_t])[-3:]
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates

    def _fast_plms(self, cond, shape, x_T, timesteps, callback, img_callback, log_every_t, cfg_scale, uc,
                   noise_keys=None):
        S = int(timesteps.shape[0])
        plan, st, c_concat, c_cross, cfg = self._open_fast("plms", cond, shape, cfg_scale, uc, rows=S + 1)  # rows = model evaluations
        dev = plan.dev
        with torch.cuda.device(dev):
            order = np.arange(S)[::-1].copy()
            t_desc = np.asarray(timesteps)[order].astype(np.float32)
            # evaluation k runs at: t_0, then (x~, t_next = t_1) for the Euler corrector, then t_1, t_2, ...
            t_eval = np.concatenate([t_desc[:1], t_desc[min(1, S - 1):min(1, S - 1) + 1], t_desc[1:]])
            require(t_eval.shape[0] == S + 1, "PLMS evaluates S + 1 times", RuntimeError)
            f64b = lambda v: np.asarray(v, dtype=np.float64).tobytes()
            rkey = ("plms", t_eval.tobytes())  # (the rows belong to the plan, the coefficients to this state: ddim.py)
            ckey = (f64b(self.ddim_alphas), f64b(self.ddim_alphas_prev), f64b(self.ddim_sigmas))
            fresh_coefs = st.coefs_fresh(ckey)
            fresh = plan.rows_fresh(rkey) or fresh_coefs
            on_host = chain.on_host(x_T, c_concat, c_cross)
            with chain.upload_lock(fresh or on_host):
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                plan.load_sampler_inputs(torch.cat([st.x, st.x]) if cfg else st.x, c_concat, c_cross,
                                         plan.arch.in_channels, rkey, t_eval)
                if fresh_coefs:
                    st.load_coefs(ckey, ddim_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas,
                                                               self.ddim_sqrt_one_minus_alphas, order))
                for _ in range(S + 1 if noise_keys is None else 0):  # the reference draws (and, eta being 0, discards) one noise tensor per update:
                    torch.randn(shape, device=dev)  # plms.py get_x_prev_and_pred_x0 — same generator state afterwards
                plan.step.zero_()
                plan.prep.run()
            print(f"Running PLMS Sampling with {S} timesteps")
            # one model evaluation per graph launch: S + 1 launches from position -1, the predictor evaluation of the first step
            intermediates = chain.run_observed(st, st.x.clone(), S, 1, callback, img_callback, log_every_t, False,
                                               cfg_scale, first=-1)
            return st.x.clone(), intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None):
        def model_eps(xx, tt):
            return self._guided_eps(xx, tt, c, unconditional_guidance_scale, unconditional_conditioning, score_corrector,
                                    corrector_kwargs)

        def update(e):  # the DDIM update with sigma = 0 (eta is forced to 0), fused kernel
            return self._ddim_update(x, e, index, temperature=temperature, noise_dropout=noise_dropout,
                                     repeat_noise=repeat_noise)

        old_eps = old_eps or []
        e_t = model_eps(x, t)
        if len(old_eps) == 0:  # pseudo improved Euler: one extra evaluation at (x_prev, t_next)
            x_prev, _ = update(e_t)
            e_prime = (e_t + model_eps(x_prev, t_next)) / 2
        else:
            w = _AB[min(len(old_eps), 3)]
            e_prime = w[0] * e_t
            for k in range(1, len(w)):
                e_prime = e_prime + w[k] * old_eps[-k]
        x_prev, pred_x0 = update(e_prime)
        return x_prev, pred_x0, e_t
