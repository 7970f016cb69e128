"""ldm.models.diffusion.dpm_solver -> upgpt_amd.dpm_solver."""
from upgpt_amd.dpm_solver import DPMSolverSampler  # noqa: F401
