"""MultistepSolverSampler — what DPMSolverSampler, UniPCSampler and DPMSolverSDESampler share: multistep solvers on the data
prediction of an eps-parameterised model (the first two deterministic, the third with DDIM's eta: dpm_sde.py), on a grid
uniform in lambda = log(alpha / sigma), with DDIMSampler's surface.

Here, once: the "logsnr" grid, the checks and the schedule cache of sample(), the dispatch between the two paths, the
fast path (the captured graphs of engine.SamplerState kind KIND, opened by DDIMSampler._open_fast and run by
chain.run_observed) and the general path (one apply_model and one eager step-kernel launch per step from Python).
A solver supplies NAME and KIND, _table (its coefficient rows for a chain), _history and _step (its eager buffers and
kernel call), and overrides _check_mask when it runs no masked chains and _check_eta when it takes an eta other than 0;
a solver that draws step noise hands _general its `draw` (dpm_sde.py, which also has a fast path of its own: its chains
carry a noise table and a mask).
"""
import numpy as np
import torch

from . import chain, rng
from . import ddim as _ddim
from ._check import require
from ._lib import get_context, host_io
from .ddim import DDIMSampler
from .schedule import make_logsnr_timesteps


class MultistepSolverSampler(DDIMSampler):
    NAME = KIND = None  # what the printed lines and messages call the solver; its engine.SamplerState kind

    # ------------------------------------------------------------------ the solver's own
    def _table(self, k):
        """-> (start, build): the coefficient rows a chain from loop position k reads — build() gives the host table made
        for a chain that starts at `start`; loop position k + i is its row k + i - start."""
        raise NotImplementedError

    def _history(self, x):
        """The eager step's history buffers for a latent like x (torch.empty: the rows say what is read)."""
        raise NotImplementedError

    def _step(self, ctx, x, e, coefs, row, history, pred_x0, b, C, hw, first_row, cfg_scale, cfg):
        """One eager launch of the step kernel on the table row `row`."""
        raise NotImplementedError

    def _check_eta(self, eta):
        """Raises for an eta the solver does not run."""
        if eta != 0:
            raise ValueError("%s is deterministic: eta must be 0 (got %r)" % (self.NAME, eta))

    def _check_mask(self, mask, x0):
        """Raises where the solver runs no masked chain; the general path blends q_sample(x0, t) in front of every
        evaluation otherwise."""

    # ------------------------------------------------------------------ schedule and entry
    def _make_timesteps(self, discretize, num_steps, verbose):
        if discretize != "logsnr":
            return super()._make_timesteps(discretize, num_steps, verbose)
        steps = make_logsnr_timesteps(self.model.alphas_cumprod, num_steps)[1:]
        if verbose:
            print("logSNR timesteps:", steps)
        return steps

    def _make_grid(self, ddim_num_steps, ddim_discretize, ddim_eta, verbose):
        """DDIMSampler's tables on the chosen grid (alphas_prev[0] = alphas_cumprod[0] is the chain's last target on every
        grid); drops the general path's device copies of the coefficient rows."""
        self._check_eta(ddim_eta)
        super().make_schedule(ddim_num_steps, ddim_discretize, 0., verbose)  # (DDIM's sigmas are not the solvers')
        self._dev_tables = {}  # start -> (device, rows, row indices)

    def _sample(self, S, batch_size, shape, discretize, solver, normals_sequence, eta, verbose, noise_keys, cond,
                mask=None, x0=None, **run):
        """The body of sample(): `solver` = the solver's own make_schedule arguments in its signature's order (they key
        the schedule cache), `run` = what goes on to _sampling."""
        rng.check_keys(noise_keys, batch_size, normals_sequence)
        self._check_eta(eta)
        require(getattr(self.model, "parameterization", "eps") == "eps",
                "%s here takes an eps-parameterised model" % self.NAME, NotImplementedError)
        self._check_mask(mask, x0)
        self._ensure_schedule((int(S), str(discretize), float(eta)) + tuple(solver.values()),
                              lambda: self.make_schedule(S, discretize, float(eta), verbose, **solver), verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f"Data shape for {self.NAME} sampling is {size}")
        return self._sampling(cond, size, mask=mask, x0=x0, noise_keys=noise_keys, **run)

    def _sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, quantize_denoised=False, mask=None,
                  x0=None, img_callback=None, log_every_t=100, noise_dropout=0., score_corrector=None,
                  corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                  noise_keys=None):
        rng.check_keys(noise_keys, shape[0])
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs a VQ first stage (not on the UPGPT path)")
        self._check_mask(mask, x0)
        timesteps = self._subset(timesteps)
        if mask is None and len(timesteps) == len(self.ddim_timesteps) and \
                self._fast_ok(cond, False, quantize_denoised, None, noise_dropout, score_corrector,
                              unconditional_guidance_scale, unconditional_conditioning):
            return self._fast(cond, shape, x_T, callback, img_callback, log_every_t, unconditional_guidance_scale,
                              unconditional_conditioning, noise_keys)
        img = chain.start_latent(x_T, noise_keys, shape, self.model.betas.device)
        return self._general(img, cond, timesteps, callback, img_callback, log_every_t, mask, x0, score_corrector,
                             corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning, noise_keys)

    # ------------------------------------------------------------------ general path
    def _device_table(self, device, k):
        """The coefficient rows of a chain from loop position k on `device`, the row indices 0 .. len - 1 and the row of
        position k; built and uploaded once per schedule and table."""
        start, build = self._table(k)
        held = self._dev_tables.get(start)
        if held is None or held[0] != str(device):
            rows = build()
            with host_io():
                held = self._dev_tables[start] = (str(device), rows.to(device),
                                                  torch.arange(rows.shape[0], dtype=torch.int32, device=device))
        return held[1], held[2], k - start

    def _general(self, img, cond, timesteps, callback, img_callback, log_every_t, mask, x0, score_corrector,
                 corrector_kwargs, cfg_scale, uc, noise_keys, draw=None):
        """One apply_model and one eager step per step.  A chain of T steps starts at loop position k = S - T: the first
        row it reads is first-order (the history is not this chain's).  mask / x0: the reference's blend with
        q_sample(x0, t) in front of every evaluation (ddim.py:144-147, as plms_sampling does it).  draw(i) (a solver with step
        noise): what its _step takes as last argument for loop position k + i — the step's noise, drawn after that
        position's q_sample draw."""
        device = img.device
        shape = tuple(img.shape)
        b, C, hw = shape[0], shape[1], shape[2] * shape[3]
        S, T = int(self.ddim_timesteps.shape[0]), int(timesteps.shape[0])
        k = S - T
        coefs, rows, r0 = self._device_table(device, k)
        ctx = get_context(device)
        guided = uc is not None and cfg_scale != 1.
        x = img.detach().clone().float().contiguous()
        history = self._history(x)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        print(f"Running {self.NAME} Sampling with {T} timesteps")
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
            nz = () if draw is None else (draw(i),)
            with torch.cuda.device(device):
                self._step(ctx, x, e.float().contiguous(), coefs, rows[r0 + i:r0 + i + 1], history, pred_x0, b, C, hw, r0,
                           cfg_scale if in_kernel else 1., in_kernel, *nz)
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
        require(not use_original_steps, "%s runs on its own grid, not on the original steps" % self.NAME, NotImplementedError)
        timesteps = self.ddim_timesteps[:t_start]
        return self._general(x_latent, cond, timesteps, None, None, 10 ** 9, None, None, None, None,
                             unconditional_guidance_scale, unconditional_conditioning, None)[0]

    # ------------------------------------------------------------------ fast path
    def _fast(self, cond, shape, x_T, callback, img_callback, log_every_t, cfg_scale, uc, noise_keys=None):
        plan, st, c_concat, c_cross, cfg = self._open_fast(self.KIND, cond, shape, cfg_scale, uc)
        S = int(self.ddim_timesteps.shape[0])
        table = self._table(0)[1]()
        dev = plan.dev
        with torch.cuda.device(dev):
            t_desc = np.asarray(self.ddim_timesteps)[::-1].astype(np.float32)
            # upload-once caches, as in DDIMSampler._fast_sampling: the timestep rows belong to the plan (one key for the
            # solvers: the same grid gives the same rows), the table to the state
            rkey = ("dpm", t_desc.tobytes())
            ckey = table.numpy().tobytes()
            fresh_coefs = st.coefs_fresh(ckey)
            fresh = fresh_coefs or plan.rows_fresh(rkey)
            on_host = chain.on_host(x_T, c_concat, c_cross)
            keyed = noise_keys is not None
            # (chain.upload_lock: the only draw is x_T)
            with chain.upload_lock(fresh or on_host or (x_T is None and not keyed)):
                st.x.copy_(chain.start_latent(x_T, noise_keys, shape, dev, torch.float32))
                if fresh_coefs:
                    st.load_coefs(ckey, table)
                plan.load_sampler_inputs(torch.cat([st.x, st.x]) if cfg else st.x, c_concat, c_cross,
                                         plan.arch.in_channels, rkey, t_desc)
                plan.step.zero_()
                plan.prep.run()
            first = st.x.clone()
            print(f"Running {self.NAME} Sampling with {S} timesteps")
            intermediates = chain.run_observed(st, first, S, _ddim.STEPS_PER_GRAPH, callback, img_callback, log_every_t,
                                               False, cfg_scale)
            return st.x.clone(), intermediates
