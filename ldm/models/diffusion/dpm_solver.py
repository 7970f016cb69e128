"""ldm.models.diffusion.dpm_solver -> upgpt_amd.dpm_solver, upgpt_amd.dpm_sde."""
from upgpt_amd.dpm_sde import DPMSolverSDESampler  # noqa: F401
from upgpt_amd.dpm_solver import DPMSolverSampler  # noqa: F401
