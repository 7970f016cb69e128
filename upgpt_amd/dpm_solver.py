"""DPMSolverSampler — DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095, algorithm 2): the second-order multistep solver
on the data prediction, eta = 0.  One model evaluation per step, one tensor of history (the data prediction of the step
before), no noise after x_T.  The reference project has no such sampler; the class keeps DDIMSampler's surface (same
constructor, sample / decode signatures and return values) so that it drops in wherever DDIMSampler does.

The step grid is uniform in lambda = log(alpha / sigma) (schedule.make_logsnr_timesteps): on the reference's `uniform`
grid the last steps jump so far in logSNR that the second-order term gains nothing.  `discretize="uniform"`
and `"quad"` still take the reference's grids.

Fast path (DDIMSampler._fast_ok's conditions, no mask, the whole chain): the captured HIP graph UNet body ->
upk_dpmpp_2m_step_f32 of engine.SamplerState kind "dpm", launched by chain.run: up to ddim.STEPS_PER_GRAPH steps per graph,
S replays in all; guidance is combined inside the step kernel.  Anything else (mask / x0, decode, a shortened chain, a score
corrector, noise dropout) runs on the general path: one apply_model per step from Python and the same kernel launched eagerly.
"""
import numpy as np
import torch

from . import chain, rng
from . import ddim as _ddim
from ._check import require
from ._lib import get_context, host_io
from .ddim import DDIMSampler
from .schedule import dpm_coefficient_table, make_logsnr_timesteps


class DPMSolverSampler(DDIMSampler):
    def _make_timesteps(self, discretize, num_steps, verbose):
        if discretize != "logsnr":
            return super()._make_timesteps(discretize, num_steps, verbose)
        steps = make_logsnr_timesteps(self.model.alphas_cumprod, num_steps)[1:]
        if verbose:
            print("logSNR timesteps:", steps)
        return steps

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=0., verbose=True, order=2,
                      lower_order_final=None):
        """DDIMSampler's tables on the chosen grid (alphas_prev[0] = alphas_cumprod[0] is the chain's last target on every
        grid) and the [S, 8] coefficient rows of the step kernel in loop order (schedule.dpm_coefficient_table)."""
        if ddim_eta != 0:
            raise ValueError("DPM-Solver++(2M) is deterministic: eta must be 0 (got %r)" % (ddim_eta,))
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.dpm_coefs = dpm_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, order, lower_order_final)
        self._dpm_dev = None  # (the general path's device copy of the table)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, order=2, discretize="logsnr",
               lower_order_final=None, **kwargs):
        """DDIMSampler.sample's arguments, plus order (2, or 1 = DDIM at eta 0), discretize ("logsnr" / "uniform" / "quad")
        and lower_order_final (None: S < 15 — the last step of a short chain is first-order).  The solver draws no noise:
        temperature, noise_dropout and normals_sequence have nothing to act on; `noise_keys=` gives x_T (rng.STREAM_XT)."""
        noise_keys = kwargs.get("noise_keys")
        rng.check_keys(noise_keys, batch_size, normals_sequence)
        if eta != 0:
            raise ValueError("DPM-Solver++(2M) is deterministic: eta must be 0 (got %r)" % (eta,))
        require(getattr(self.model, "parameterization", "eps") == "eps",
                "DPM-Solver++(2M) here takes an eps-parameterised model", NotImplementedError)
        self._ensure_schedule((int(S), str(discretize), int(order), lower_order_final), lambda: self.make_schedule(
            S, discretize, 0., verbose, order=order, lower_order_final=lower_order_final), verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f"Data shape for DPM-Solver++(2M) sampling is {size}")
        return self.dpm_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                 quantize_denoised=quantize_x0, mask=mask, x0=x0, noise_dropout=noise_dropout,
                                 score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                 log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning, noise_keys=noise_keys)

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                     x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                     corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                     noise_keys=None):
        """`timesteps` (a count, as in ddim_sampling): a chain over the last rows of the schedule."""
        rng.check_keys(noise_keys, shape[0])
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs a VQ first stage (not on the UPGPT path)")
        timesteps = self._subset(timesteps)
        if mask is None and len(timesteps) == len(self.ddim_timesteps) and \
                self._fast_ok(cond, False, quantize_denoised, None, noise_dropout, score_corrector,
                              unconditional_guidance_scale, unconditional_conditioning):
            return self._fast_dpm(cond, shape, x_T, callback, img_callback, log_every_t, unconditional_guidance_scale,
                                  unconditional_conditioning, noise_keys)
        img = chain.start_latent(x_T, noise_keys, shape, self.model.betas.device)
        return self._general(img, cond, timesteps, callback, img_callback, log_every_t, mask, x0, score_corrector,
                             corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning, noise_keys)

    # ------------------------------------------------------------------ general path
    def _device_table(self, device):
        """The coefficient rows and the row indices 0 .. S-1 on `device`, uploaded once per schedule."""
        held = getattr(self, "_dpm_dev", None)
        if held is None or held[0] != str(device):
            with host_io():
                S = int(self.dpm_coefs.shape[0])
                held = self._dpm_dev = (str(device), self.dpm_coefs.to(device),
                                        torch.arange(S, dtype=torch.int32, device=device))
        return held[1], held[2]

    def _general(self, img, cond, timesteps, callback, img_callback, log_every_t, mask, x0, score_corrector,
                 corrector_kwargs, cfg_scale, uc, noise_keys):
        """One apply_model and one eager upk_dpmpp_2m_step_f32 per step.  A chain of T steps runs rows S - T .. S - 1 of the
        S-row table; its first row is first-order (first_row: the history is not this chain's).  mask / x0: the reference's
        blend with q_sample(x0, t) in front of every evaluation (ddim.py:144-147, as plms_sampling does it)."""
        device = img.device
        shape = tuple(img.shape)
        b, C, hw = shape[0], shape[1], shape[2] * shape[3]
        S, T = int(self.ddim_timesteps.shape[0]), int(timesteps.shape[0])
        k = S - T
        coefs, rows = self._device_table(device)
        ctx = get_context(device)
        guided = uc is not None and cfg_scale != 1.
        x = img.detach().clone().float().contiguous()
        x0_old = torch.empty_like(x)  # (never read on the chain's first row)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        print(f"Running DPM-Solver++(2M) Sampling with {T} timesteps")
        for i, step in enumerate(np.flip(timesteps)):
            index = T - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:
                require(x0 is not None, "mask given without x0", ValueError)
                qn = {} if noise_keys is None else {"noise": rng.randn(noise_keys, shape, rng.STREAM_QSAMPLE, row0=k + i)}
                x = (self.model.q_sample(x0, ts, **qn) * mask + (1. - mask) * x).float().contiguous()
            # ([uncond ; cond] of a guided evaluation is combined inside the step kernel, as on the fast path; a score
            # corrector needs the combined eps first)
            in_kernel = guided and score_corrector is None
            e = self._guided_eps(x, ts, cond, cfg_scale, uc, score_corrector, corrector_kwargs, combine=not in_kernel)
            pred_x0 = torch.empty_like(x)
            with torch.cuda.device(device):
                ctx.dpmpp_2m_step(x, e.float().contiguous(), coefs, rows[k + i:k + i + 1], x0_old, pred_x0, None, 0, b, C, hw,
                                  first_row=k, cfg_scale=cfg_scale if in_kernel else 1., cfg=in_kernel)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == T - 1:
                intermediates["x_inter"].append(x.clone())
                intermediates["pred_x0"].append(pred_x0)
        return x, intermediates

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, noise_keys=None):
        """The last t_start steps of the schedule from x_latent (img2img, after stochastic_encode), on the general path.
        noise_keys is DDIMSampler.decode's argument: the solver draws nothing, so it has nothing to key."""
        require(not use_original_steps, "DPM-Solver++(2M) runs on its own grid, not on the original steps", NotImplementedError)
        timesteps = self.ddim_timesteps[:t_start]
        return self._general(x_latent, cond, timesteps, None, None, 10 ** 9, None, None, None, None,
                             unconditional_guidance_scale, unconditional_conditioning, None)[0]

    # ------------------------------------------------------------------ fast path
    def _fast_dpm(self, cond, shape, x_T, callback, img_callback, log_every_t, cfg_scale, uc, noise_keys=None):
        model = self.model
        unet = model.model.diffusion_model
        b, C, H, W = shape
        cfg = uc is not None and cfg_scale != 1.
        if cfg:
            cond = self._cat_cond(uc, cond)
        c_concat, c_cross = model._split_cond(cond)
        S = int(self.ddim_timesteps.shape[0])
        plan = unet.plan(2 * b if cfg else b, H, W, c_cross.shape[1], S, "sampler")
        dev = plan.dev
        with torch.cuda.device(dev):
            st = plan.sampler_state("dpm", C, cfg)
            t_desc = np.asarray(self.ddim_timesteps)[::-1].astype(np.float32)
            # upload-once caches, as in DDIMSampler._fast_sampling: the timestep rows belong to the plan, the table to the state
            rkey = ("dpm", t_desc.tobytes())
            ckey = self.dpm_coefs.numpy().tobytes()
            fresh_coefs = getattr(st, "_coef_key", None) != ckey
            fresh = fresh_coefs or getattr(plan, "_t_rows_key", None) != rkey
            on_host = chain.on_host(x_T, c_concat, c_cross)
            keyed = noise_keys is not None
            with chain.upload_lock(fresh or on_host or (x_T is None and not keyed)):
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                if fresh_coefs:
                    st.coefs.copy_(self.dpm_coefs)
                    st._coef_key = ckey
                plan.load_sampler_inputs(torch.cat([st.x, st.x]) if cfg else st.x, c_concat, c_cross, unet.in_channels,
                                         rkey, t_desc)
                plan.step.zero_()
                plan.prep.run()
            first = st.x.clone()
            intermediates = {"x_inter": [first], "pred_x0": [first.clone()]}
            print(f"Running DPM-Solver++(2M) Sampling with {S} timesteps")
            watched = callback is not None or img_callback is not None
            logged = chain.logged_at(S, log_every_t)
            for i in chain.run(st, S, _ddim.STEPS_PER_GRAPH, watched, logged, False, cfg_scale):
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(st.pred_x0.clone(), i)
                if logged(i):
                    intermediates["x_inter"].append(st.x.clone())
                    intermediates["pred_x0"].append(st.pred_x0.clone())
            return st.x.clone(), intermediates
