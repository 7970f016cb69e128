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
DPM-Solver++(2M) (sampler="dpmpp_2m") runs such chains.  Both paths, and everything else the solver shares with
DPM-Solver++(2M), are multistep.MultistepSolverSampler's.
"""
import torch

from ._check import require
from .multistep import MultistepSolverSampler
from .schedule import unipc_coefficient_table

_MASKED = ("UniPC has no masked chain (mask= / x0=): the q_sample blend in front of every evaluation contradicts the "
           "corrector's latent; use sampler=\"dpmpp_2m\" (DPMSolverSampler) for inpainting and region edits")


class UniPCSampler(MultistepSolverSampler):
    NAME, KIND = "UniPC", "unipc"

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=0., verbose=True, order=2, variant="bh2",
                      corrector=True, lower_order_final=True):
        """DDIMSampler's tables on the chosen grid and the [S, 12] coefficient rows of the whole chain in loop order."""
        self._make_grid(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.unipc_args = dict(order=order, variant=variant, corrector=bool(corrector),
                               lower_order_final=bool(lower_order_final))
        self.unipc_coefs = unipc_coefficient_table(self.ddim_alphas, self.ddim_alphas_prev, **self.unipc_args)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, order=2, variant="bh2", corrector=True,
               lower_order_final=True, discretize="logsnr", **kwargs):
        """DDIMSampler.sample's arguments, plus order (1, 2 or 3), variant ("bh2": B(h) = expm1(-h), "bh1": -h), corrector
        (False: the predictor alone — at order 2 DPM-Solver++(2M)), lower_order_final and discretize ("logsnr" / "uniform" /
        "quad").  The solver draws no noise; `noise_keys=` gives x_T (rng.STREAM_XT)."""
        solver = dict(order=order, variant=str(variant), corrector=bool(corrector),
                      lower_order_final=bool(lower_order_final))
        return self._sample(S, batch_size, shape, discretize, solver, normals_sequence, eta, verbose,
                            kwargs.get("noise_keys"), conditioning, mask, x0, callback=callback,
                            img_callback=img_callback, quantize_denoised=quantize_x0, noise_dropout=noise_dropout,
                            score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                            log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                            unconditional_conditioning=unconditional_conditioning)

    @torch.no_grad()
    def unipc_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                       x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                       corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                       noise_keys=None):
        """`timesteps` (a count, as in ddim_sampling): a chain over the last rows of the schedule."""
        return self._sampling(cond, shape, x_T, callback, timesteps, quantize_denoised, mask, x0, img_callback,
                              log_every_t, noise_dropout, score_corrector, corrector_kwargs,
                              unconditional_guidance_scale, unconditional_conditioning, noise_keys)

    def _check_mask(self, mask, x0):
        require(mask is None and x0 is None, _MASKED, NotImplementedError)

    def _table(self, k):
        """A chain that starts at loop position k runs a table built for it (start = k): its first row has no corrector
        and a first-order predictor (the history is not this chain's)."""
        return k, lambda: self.unipc_coefs if k == 0 else unipc_coefficient_table(
            self.ddim_alphas, self.ddim_alphas_prev, start=k, **self.unipc_args)

    def _history(self, x):
        hist = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=x.device)  # (read only where the rows say so)
        return hist, torch.empty_like(x)  # (... and x_corr)

    def _step(self, ctx, x, e, coefs, row, history, pred_x0, b, C, hw, first_row, cfg_scale, cfg):
        ctx.unipc_step(x, e, coefs, row, *history, pred_x0, None, 0, b, C, hw, cfg_scale=cfg_scale, cfg=cfg)
