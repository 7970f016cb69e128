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
Both paths, and everything else the solver shares with UniPC, are multistep.MultistepSolverSampler's.
"""
import torch

from .multistep import MultistepSolverSampler
from .schedule import dpm_coefficient_table


class DPMSolverSampler(MultistepSolverSampler):
    NAME, KIND = "DPM-Solver++(2M)", "dpm"

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=0., verbose=True, order=2,
                      lower_order_final=None):
        """DDIMSampler's tables on the chosen grid and the [S, 8] coefficient rows of the step kernel in loop order
        (schedule.dpm_coefficient_table)."""
        self._make_grid(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.dpm_coefs = dpm_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, order, lower_order_final)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, order=2, discretize="logsnr",
               lower_order_final=None, **kwargs):
        """DDIMSampler.sample's arguments, plus order (2, or 1 = DDIM at eta 0), discretize ("logsnr" / "uniform" / "quad")
        and lower_order_final (None: S < 15 — the last step of a short chain is first-order).  The solver draws no noise:
        temperature, noise_dropout and normals_sequence have nothing to act on; `noise_keys=` gives x_T (rng.STREAM_XT)."""
        return self._sample(S, batch_size, shape, discretize, dict(order=int(order), lower_order_final=lower_order_final),
                            normals_sequence, eta, verbose, kwargs.get("noise_keys"), conditioning, mask, x0,
                            callback=callback, img_callback=img_callback, quantize_denoised=quantize_x0,
                            noise_dropout=noise_dropout, score_corrector=score_corrector,
                            corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                            unconditional_guidance_scale=unconditional_guidance_scale,
                            unconditional_conditioning=unconditional_conditioning)

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                     x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                     corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                     noise_keys=None):
        """`timesteps` (a count, as in ddim_sampling): a chain over the last rows of the schedule."""
        return self._sampling(cond, shape, x_T, callback, timesteps, quantize_denoised, mask, x0, img_callback,
                              log_every_t, noise_dropout, score_corrector, corrector_kwargs,
                              unconditional_guidance_scale, unconditional_conditioning, noise_keys)

    def _table(self, k):
        """The one S-row table serves every chain: a chain of T steps runs its rows S - T .. S - 1 and names the first of
        them to the kernel (first_row), which takes it first-order."""
        return 0, lambda: self.dpm_coefs

    def _history(self, x):
        return torch.empty_like(x)  # x0_old (never read on the chain's first row)

    def _step(self, ctx, x, e, coefs, row, x0_old, pred_x0, b, C, hw, first_row, cfg_scale, cfg):
        ctx.dpmpp_2m_step(x, e, coefs, row, x0_old, pred_x0, None, 0, b, C, hw, first_row=first_row, cfg_scale=cfg_scale,
                          cfg=cfg)
