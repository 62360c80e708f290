"""Image filters with the names of ``medpy.filter``, computed on the device."""
from .smoothing import anisotropic_diffusion

__all__ = ["anisotropic_diffusion"]
