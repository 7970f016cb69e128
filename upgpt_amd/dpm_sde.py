"""DPMSolverSDESampler — SDE-DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095: the stochastic form of the second-order
multistep update on the data prediction).  `eta` interpolates between the ODE (eta = 0: DPM-Solver++(2M) term by term)
and the SDE (eta = 1: the sde-dpmsolver++ midpoint form); one model evaluation and one normal draw per step, one tensor
of history.  With h = lambda_t - lambda_s the step s -> t is

    x_t = (sigma_t / sigma_s) exp(-eta h) x_s - alpha_t expm1(-(1 + eta) h) D + sigma_t sqrt(-expm1(-2 eta h)) z,
    D = m_s + h / (2 h_prev) (m_s - m_{s-1})   (second order;  D = m_s first order)

(DESIGN.md 42).  The reference project has no such sampler; the class keeps DDIMSampler's surface and runs on the
logSNR-uniform grid of DPMSolverSampler.

Fast path (DDIMSampler._fast_ok's conditions, the schedule or a tail of it): the captured HIP graph UNet body ->
upk_dpmpp_2m_sde_step_f32 of engine.SamplerState kind "dpm_sde", launched by chain.run.  The whole chain, a shortened
chain and decode (a table built with start = k in rows k .. S - 1, plan.step preset to k) and masked chains (the keep
table and the blend for the next step inside the kernel, as DDIM's: the first blend is made here) all run there.  The
noise table rows k .. S - 1 (scaled by r5 * temperature) and the keep rows are filled before the loop as
DDIMSampler._fast_sampling fills them: keyed in one launch each, unkeyed one torch.randn per step in loop order with
q_sample's draw in front of it; a row whose noise scale is 0 draws nothing, eta = 0 runs without a noise table.
General path (a score corrector, noise dropout, _fast_ok false): MultistepSolverSampler._general with this solver's draw —
the same normals in the same generator order, the same kernel launched eagerly on one coefficient row and one noise row.
"""
import numpy as np
import torch

from . import chain, rng
from . import ddim as _ddim
from ._check import require
from .multistep import MultistepSolverSampler
from .schedule import dpm_sde_coefficient_table


class DPMSolverSDESampler(MultistepSolverSampler):
    NAME, KIND = "SDE-DPM-Solver++(2M)", "dpm_sde"

    def _check_eta(self, eta):
        if not 0. <= float(eta) <= 1.:
            raise ValueError("%s takes 0 <= eta <= 1 (got %r)" % (self.NAME, eta))

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=1., verbose=True, order=2,
                      lower_order_final=None):
        """DDIMSampler's tables on the chosen grid and the [S, 8] coefficient rows of the whole chain in loop order
        (schedule.dpm_sde_coefficient_table)."""
        self._make_grid(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.sde_args = dict(eta=float(ddim_eta), order=order, lower_order_final=lower_order_final)
        self.dpm_sde_coefs = dpm_sde_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, **self.sde_args)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=1., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, order=2, discretize="logsnr",
               lower_order_final=None, **kwargs):
        """DDIMSampler.sample's arguments, plus order (2 or 1), discretize ("logsnr" / "uniform" / "quad") and
        lower_order_final (None: S < 15).  eta in [0, 1]; temperature scales the step noise; normals_sequence ([S, B, C, H,
        W] standard normals in loop order) and `noise_keys=` (rng.STREAM_XT / STREAM_STEP / STREAM_QSAMPLE, the rows DDIM
        uses) are DDIMSampler.sample's."""
        return self._sample(S, batch_size, shape, discretize, dict(order=int(order), lower_order_final=lower_order_final),
                            normals_sequence, eta, verbose, kwargs.get("noise_keys"), conditioning, mask, x0,
                            callback=callback, img_callback=img_callback, quantize_denoised=quantize_x0,
                            noise_dropout=noise_dropout, score_corrector=score_corrector,
                            corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                            unconditional_guidance_scale=unconditional_guidance_scale,
                            unconditional_conditioning=unconditional_conditioning, temperature=temperature,
                            normals=normals_sequence)

    @torch.no_grad()
    def dpm_sde_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                         x0=None, img_callback=None, log_every_t=100, temperature=1., noise_dropout=0.,
                         score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                         unconditional_conditioning=None, normals_sequence=None, noise_keys=None):
        """`timesteps` (a count, as in ddim_sampling): a chain over the last rows of the schedule."""
        return self._sampling(cond, shape, x_T, callback, timesteps, quantize_denoised, mask, x0, img_callback,
                              log_every_t, noise_dropout, score_corrector, corrector_kwargs,
                              unconditional_guidance_scale, unconditional_conditioning, noise_keys, temperature,
                              normals_sequence)

    def _sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                  x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                  corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                  noise_keys=None, temperature=1., normals=None):
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs a VQ first stage (not on the UPGPT path)")
        return self._chain(self._subset(timesteps), cond, shape, x_T, callback, mask, x0, img_callback, log_every_t,
                           noise_dropout, score_corrector, corrector_kwargs, unconditional_guidance_scale,
                           unconditional_conditioning, noise_keys, temperature, normals)

    def _chain(self, timesteps, cond, shape, x_T, callback=None, mask=None, x0=None, img_callback=None, log_every_t=100,
               noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, noise_keys=None, temperature=1., normals=None):
        """The chain over `timesteps` (the schedule or a prefix of it = its last loop positions) on whichever path takes it."""
        rng.check_keys(noise_keys, shape[0], normals)
        require(mask is None or x0 is not None, "mask given without x0", ValueError)
        if self._is_tail(timesteps) and self._fast_ok(cond, False, False, mask, noise_dropout, score_corrector,
                                                      unconditional_guidance_scale, unconditional_conditioning):
            return self._fast(cond, shape, x_T, timesteps, callback, img_callback, log_every_t, temperature, normals,
                              unconditional_guidance_scale, unconditional_conditioning, mask, x0, noise_keys)
        img = chain.start_latent(x_T, noise_keys, shape, self.model.betas.device)
        k = int(self.ddim_timesteps.shape[0]) - int(timesteps.shape[0])
        log_every_t = 10 ** 9 if log_every_t is None else log_every_t  # (decode logs nothing)
        return self._general(img, cond, timesteps, callback, img_callback, log_every_t, mask, x0, score_corrector,
                             corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning, noise_keys,
                             draw=self._draw(k, shape, img.device, temperature, normals, noise_keys, noise_dropout))

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, noise_keys=None):
        """The last t_start steps of the schedule from x_latent (img2img, after stochastic_encode).  noise_keys: the step
        noise of the chain's rows (rng.STREAM_STEP), instead of one generator draw per step."""
        require(not use_original_steps, "%s runs on its own grid, not on the original steps" % self.NAME, NotImplementedError)
        return self._chain(self.ddim_timesteps[:t_start], cond, tuple(x_latent.shape), x_latent, log_every_t=None,
                           unconditional_guidance_scale=unconditional_guidance_scale,
                           unconditional_conditioning=unconditional_conditioning, noise_keys=noise_keys)[0]

    # ------------------------------------------------------------------ the solver's own
    def _table(self, k):
        """A chain that starts at loop position k runs a table built for it (start = k): its first row is first-order."""
        return k, lambda: self.dpm_sde_coefs if k == 0 else dpm_sde_coefficient_table(
            self.ddim_alphas, self.ddim_alphas_prev, start=k, **self.sde_args)

    def _history(self, x):
        return torch.empty_like(x)  # m_old (never read on a first-order row)

    def _draw(self, k, shape, device, temperature, normals, noise_keys, noise_dropout):
        """-> draw(i) of MultistepSolverSampler._general: (i, the noise row of loop position k + i scaled by r5 *
        temperature, or None where r5 is 0).  One generator draw per row with noise, where the fast path makes it."""
        scale = self._table(k)[1]()[:, 5] * float(temperature)  # (the fp32 product the fast path's table carries)

        def draw(i):
            s = float(scale[i])
            if s == 0.:
                return i, None
            if normals is not None:
                z = normals[i].to(device, torch.float32)
            elif noise_keys is not None:
                z = rng.randn(noise_keys, shape, rng.STREAM_STEP, row0=k + i)
            else:
                z = torch.randn(shape, device=device)
            nz = z * s
            if noise_dropout > 0.:
                nz = torch.nn.functional.dropout(nz, p=noise_dropout)
            return i, nz.float().contiguous().reshape(1, -1)
        return draw

    def _step(self, ctx, x, e, coefs, row, m_old, pred_x0, b, C, hw, first_row, cfg_scale, cfg, drawn):
        i, nz = drawn  # (one coefficient row and one noise row: step = NULL reads row 0 of both)
        ctx.dpmpp_2m_sde_step(x, e, coefs[i:i + 1], nz, None, None, 0, None, m_old, pred_x0, None, None, 0, b, C, hw,
                              cfg_scale=cfg_scale, cfg=cfg)

    # ------------------------------------------------------------------ fast path
    def _fast(self, cond, shape, x_T, timesteps, callback, img_callback, log_every_t, temperature, normals, cfg_scale,
              uc, mask, x0, noise_keys):
        """T = len(timesteps) steps from loop position k = S - T, as DDIMSampler._fast_sampling runs them: the noise table
        rows k .. S - 1 and, with a mask, the keep rows (row r = q_sample(x0, t_r)) are filled in front of the loop, the
        first blend is made here and the later ones by the step kernel."""
        masked, keyed = mask is not None, noise_keys is not None
        model, b = self.model, shape[0]
        plan, st, c_concat, c_cross, cfg = self._open_fast(self.KIND, cond, shape, cfg_scale, uc)
        S, T = int(self.ddim_timesteps.shape[0]), int(timesteps.shape[0])
        k = S - T
        table = self._table(k)[1]()
        dev = plan.dev
        with torch.cuda.device(dev):
            t_desc = np.asarray(self.ddim_timesteps)[::-1].astype(np.float32)
            scale = torch.zeros(S, dtype=torch.float32)  # indexed by the absolute row, as rng.randn reads it
            scale[k:] = table[:, 5] * float(temperature)
            with_noise = bool((scale != 0).any())
            st.set_variant("masked" if masked else None)
            # upload-once caches, as in DDIMSampler._fast_sampling: the timestep rows belong to the plan (the solvers' key:
            # the same grid gives the same rows), the table and the keyed chain's noise scale to the state
            rkey = ("dpm", t_desc.tobytes())
            ckey = (k, table.numpy().tobytes())
            skey = (ckey, float(temperature))
            fresh_coefs = st.coefs_fresh(ckey)
            fresh_scale = keyed and with_noise and st.scale_fresh(skey)
            fresh = plan.rows_fresh(rkey) or fresh_coefs or fresh_scale
            on_host = chain.on_host(x_T, c_concat, c_cross, mask, x0)
            with chain.upload_lock(fresh or on_host or (with_noise and not keyed)):
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                if masked:
                    keep, emask, _ = st.ensure_edit()
                    x0 = x0.to(dev)
                    mask = mask.to(dev, torch.float32)
                    emask.copy_(mask.expand(shape).reshape(-1))
                if fresh_coefs:
                    st.load_coefs(ckey, table, row0=k)
                nz = st.ensure_noise() if with_noise else None
                if with_noise and normals is not None:
                    ns = normals if torch.is_tensor(normals) else torch.stack(list(normals))
                    nz[k:].copy_(ns.to(dev, torch.float32).reshape(T, -1))
                if keyed:
                    if fresh_scale:
                        st.load_noise_scale(skey, scale)
                    if with_noise:
                        rng.randn(noise_keys, shape, rng.STREAM_STEP, row0=k, rows=T, scale=st._nscale, out=nz[k:])
                    if masked:  # the q_sample noise of every keep row in one launch, then q_sample row by row in place
                        rng.randn(noise_keys, shape, rng.STREAM_QSAMPLE, row0=k, rows=T, out=keep[k:])
                # the generator sees the general path's order: per step q_sample's draw (masked), then the step's own
                for i in range(k, S):
                    if masked:
                        ts = torch.full((b,), int(t_desc[i]), device=dev, dtype=torch.long)
                        qn = {"noise": keep[i].view(shape)} if keyed else {}
                        keep[i].copy_(model.q_sample(x0, ts, **qn).to(dev, torch.float32).reshape(-1))
                    if with_noise and normals is None and not keyed:
                        if scale[i] != 0:
                            nz[i].copy_(torch.randn(shape, device=dev).reshape(-1))
                        else:
                            nz[i].zero_()
                if with_noise and not keyed:
                    nz[k:].mul_(scale[k:].to(dev)[:, None])
                first = st.x.clone()  # (the intermediates start with the unblended start latent, as DDIM's)
                if masked:  # the blend in front of the first step; the step kernel does the later ones
                    st.x.copy_(keep[k].view(shape) * mask + (1. - mask) * st.x)
                plan.load_sampler_inputs(torch.cat([st.x, st.x]) if cfg else st.x, c_concat, c_cross,
                                         plan.arch.in_channels, rkey, t_desc)
                plan.step.fill_(k)
                plan.prep.run()
            print(f"Running {self.NAME} Sampling with {T} timesteps")
            intermediates = chain.run_observed(st, first, T, _ddim.STEPS_PER_GRAPH, callback, img_callback, log_every_t,
                                               with_noise, cfg_scale, plain=masked)
            return st.x.clone(), intermediates  # (the last step's result is never blended)
