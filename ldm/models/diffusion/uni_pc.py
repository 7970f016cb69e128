"""ldm.models.diffusion.uni_pc -> upgpt_amd.unipc."""
from upgpt_amd.unipc import UniPCSampler  # noqa: F401
