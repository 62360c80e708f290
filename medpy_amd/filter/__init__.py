"""Image filters with the names of ``medpy.filter``, computed on the device."""
from .smoothing import anisotropic_diffusion
from .image import local_minima, minima_markers, watershed, watershed_info

__all__ = ["anisotropic_diffusion", "local_minima", "minima_markers", "watershed", "watershed_info"]
