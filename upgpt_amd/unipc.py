"""UniPCSampler — UniPC (Zhao et al. 2023, arXiv:2302.04867): the multistep predictor-corrector on the data prediction,
orders 1 to 3, eta = 0.  The corrector of a step reuses the model evaluation the next step needs anyway, so a chain of S
steps still costs S evaluations and gains one order of accuracy.  The reference project has no such
sampler; the class keeps DDIMSampler's surface, as DPMSolverSampler does, and runs on the same logSNR-uniform grid.

Evaluation k sees the PREDICTED latent at point k: it forms the data prediction m_k, corrects the step k-1 -> k with it
(from the last corrected latent and the history of m) and predicts the step k -> k+1 from the corrected latent — one
upk_unipc_step_f32 launch.  The final latent is the last prediction, uncorrected (the paper's default).  Callbacks and the
logged intermediates see the predicted latent and pred_x0 = m_k.

Fast path (DDIMSampler._fast_ok's conditions, no mask, the whole chain): the captured HIP graph UNet body ->
upk_unipc_step_f32 of engine.SamplerState kind "unipc", launched by chain.run: up to ddim.STEPS_PER_GRAPH steps per graph;
guidance is combined inside the step kernel.  decode, a shortened chain, a score corrector and noise dropout run on the
general path: one apply_model per step from Python and the same kernel launched eagerly, on a table built for the chain
(schedule.unipc_coefficient_table(start=...): a chain that starts inside the schedule has no history).  A masked chain
(mask= / x0=) is refused: the blend with q_sample(x0) in front of every evaluation contradicts the corrector's own latent;
DPM-Solver++(2M) (sampler="dpmpp_2m") runs such chains.
"""
import numpy as np
import torch

from . import chain, rng
from . import ddim as _ddim
from ._check import require
from ._lib import get_context, host_io
from .ddim import DDIMSampler
from .schedule import make_logsnr_timesteps, unipc_coefficient_table

_MASKED = ("UniPC has no masked chain (mask= / x0=): the q_sample blend in front of every evaluation contradicts the "
           "corrector's latent; use sampler=\"dpmpp_2m\" (DPMSolverSampler) for inpainting and region edits")


class UniPCSampler(DDIMSampler):
    def _make_timesteps(self, discretize, num_steps, verbose):
        if discretize != "logsnr":
            return super()._make_timesteps(discretize, num_steps, verbose)
        steps = make_logsnr_timesteps(self.model.alphas_cumprod, num_steps)[1:]
        if verbose:
            print("logSNR timesteps:", steps)
        return steps

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=0., verbose=True, order=2, variant="bh2",
                      corrector=True, lower_order_final=True):
        """DDIMSampler's tables on the chosen grid and the [S, 12] coefficient rows of the whole chain in loop order."""
        if ddim_eta != 0:
            raise ValueError("UniPC is deterministic: eta must be 0 (got %r)" % (ddim_eta,))
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.unipc_args = dict(order=order, variant=variant, corrector=bool(corrector),
                               lower_order_final=bool(lower_order_final))
        self.unipc_coefs = unipc_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, **self.unipc_args)
        self._unipc_dev = {}  # (the general path's device copies: start -> (device, rows, row indices))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, order=2, variant="bh2", corrector=True,
               lower_order_final=True, discretize="logsnr", **kwargs):
        """DDIMSampler.sample's arguments, plus order (1, 2 or 3), variant ("bh2": B(h) = expm1(-h), "bh1": -h), corrector
        (False: the predictor alone — at order 2 DPM-Solver++(2M)), lower_order_final and discretize ("logsnr" / "uniform" /
        "quad").  The solver draws no noise; `noise_keys=` gives x_T (rng.STREAM_XT)."""
        noise_keys = kwargs.get("noise_keys")
        rng.check_keys(noise_keys, batch_size, normals_sequence)
        if eta != 0:
            raise ValueError("UniPC is deterministic: eta must be 0 (got %r)" % (eta,))
        require(getattr(self.model, "parameterization", "eps") == "eps",
                "UniPC here takes an eps-parameterised model", NotImplementedError)
        require(mask is None and x0 is None, _MASKED, NotImplementedError)
        key = (int(S), str(discretize), order, str(variant), bool(corrector), bool(lower_order_final))
        self._ensure_schedule(key, lambda: self.make_schedule(
            S, discretize, 0., verbose, order=order, variant=variant, corrector=corrector,
            lower_order_final=lower_order_final), verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f"Data shape for UniPC sampling is {size}")
        return self.unipc_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                   quantize_denoised=quantize_x0, noise_dropout=noise_dropout,
                                   score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                   log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                   unconditional_conditioning=unconditional_conditioning, noise_keys=noise_keys)

    @torch.no_grad()
    def unipc_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                       x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                       corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                       noise_keys=None):
        """`timesteps` (a count, as in ddim_sampling): a chain over the last rows of the schedule."""
        rng.check_keys(noise_keys, shape[0])
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs a VQ first stage (not on the UPGPT path)")
        require(mask is None and x0 is None, _MASKED, NotImplementedError)
        timesteps = self._subset(timesteps)
        if len(timesteps) == len(self.ddim_timesteps) and \
                self._fast_ok(cond, False, quantize_denoised, None, noise_dropout, score_corrector,
                              unconditional_guidance_scale, unconditional_conditioning):
            return self._fast_unipc(cond, shape, x_T, callback, img_callback, log_every_t, unconditional_guidance_scale,
                                    unconditional_conditioning, noise_keys)
        img = chain.start_latent(x_T, noise_keys, shape, self.model.betas.device)
        return self._general(img, cond, timesteps, callback, img_callback, log_every_t, score_corrector,
                             corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning)

    # ------------------------------------------------------------------ general path
    def _device_table(self, device, start):
        """The coefficient rows of the chain that starts at loop position `start` and the row indices 0 .. S - start - 1
        on `device`, built and uploaded once per schedule and start."""
        held = self._unipc_dev.get(start)
        if held is None or held[0] != str(device):
            rows = self.unipc_coefs if start == 0 else unipc_coefficient_table(
                self.ddim_alphas, self.ddim_alphas_prev, start=start, **self.unipc_args)
            with host_io():
                held = self._unipc_dev[start] = (str(device), rows.to(device),
                                                 torch.arange(rows.shape[0], dtype=torch.int32, device=device))
        return held[1], held[2]

    def _general(self, img, cond, timesteps, callback, img_callback, log_every_t, score_corrector, corrector_kwargs,
                 cfg_scale, uc):
        """One apply_model and one eager upk_unipc_step_f32 per step.  A chain of T steps runs the table built with
        start = S - T: its first row has no corrector and a first-order predictor (the history is not this chain's)."""
        device = img.device
        shape = tuple(img.shape)
        b, C, hw = shape[0], shape[1], shape[2] * shape[3]
        S, T = int(self.ddim_timesteps.shape[0]), int(timesteps.shape[0])
        coefs, rows = self._device_table(device, S - T)
        ctx = get_context(device)
        guided = uc is not None and cfg_scale != 1.
        x = img.detach().clone().float().contiguous()
        hist = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=device)  # (read only where the rows say so)
        x_corr = torch.empty_like(x)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        print(f"Running UniPC Sampling with {T} timesteps")
        for i, step in enumerate(np.flip(timesteps)):
            index = T - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            # ([uncond ; cond] of a guided evaluation is combined inside the step kernel, as on the fast path; a score
            # corrector needs the combined eps first)
            in_kernel = guided and score_corrector is None
            e = self._guided_eps(x, ts, cond, cfg_scale, uc, score_corrector, corrector_kwargs, combine=not in_kernel)
            pred_x0 = torch.empty_like(x)
            with torch.cuda.device(device):
                ctx.unipc_step(x, e.float().contiguous(), coefs, rows[i:i + 1], hist, x_corr, pred_x0, None, 0, b, C, hw,
                               cfg_scale=cfg_scale if in_kernel else 1., cfg=in_kernel)
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
        require(not use_original_steps, "UniPC runs on its own grid, not on the original steps", NotImplementedError)
        timesteps = self.ddim_timesteps[:t_start]
        return self._general(x_latent, cond, timesteps, None, None, 10 ** 9, None, None,
                             unconditional_guidance_scale, unconditional_conditioning)[0]

    # ------------------------------------------------------------------ fast path
    def _fast_unipc(self, cond, shape, x_T, callback, img_callback, log_every_t, cfg_scale, uc, noise_keys=None):
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
            st = plan.sampler_state("unipc", C, cfg)
            t_desc = np.asarray(self.ddim_timesteps)[::-1].astype(np.float32)
            # upload-once caches, as in DPMSolverSampler._fast_dpm: the timestep rows belong to the plan (shared with the
            # "dpm" state of the same grid), the table to the state
            rkey = ("dpm", t_desc.tobytes())
            ckey = self.unipc_coefs.numpy().tobytes()
            fresh_coefs = getattr(st, "_coef_key", None) != ckey
            fresh = fresh_coefs or getattr(plan, "_t_rows_key", None) != rkey
            on_host = chain.on_host(x_T, c_concat, c_cross)
            keyed = noise_keys is not None
            # DPM's rule (chain.upload_lock): the only draw is x_T
            with chain.upload_lock(fresh or on_host or (x_T is None and not keyed)):
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                if fresh_coefs:
                    st.coefs.copy_(self.unipc_coefs)
                    st._coef_key = ckey
                plan.load_sampler_inputs(torch.cat([st.x, st.x]) if cfg else st.x, c_concat, c_cross, unet.in_channels,
                                         rkey, t_desc)
                plan.step.zero_()
                plan.prep.run()
            first = st.x.clone()
            intermediates = {"x_inter": [first], "pred_x0": [first.clone()]}
            print(f"Running UniPC Sampling with {S} timesteps")
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
