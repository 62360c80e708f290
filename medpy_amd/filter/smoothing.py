"""Edge-preserving smoothing with the names, argument order and defaults of ``medpy.filter.smoothing``, computed on the device
(the definition is medpy_amd/csrc/mgc_diffuse.h).

``anisotropic_diffusion`` takes two more keywords than the reference: ``graph``, a ``VoxelGraph`` (or ``EmbeddedLatticeGraph``): with
``img=None`` the image is the one the graph holds, read where it lies on the device (its feature image, else the image of its
boundary term; mgc_diffuse on the graph's handle), and an image given with a graph must have the graph's shape and is diffused on
the graph's device, without its handle; and ``device`` for the image of the caller's without a graph (mgc_diffuse_image: no handle at all).  1-D to 3-D images; more dimensions raise NotImplementedError.
"""
import ctypes as C

import numpy

__all__ = ["anisotropic_diffusion"]


def check_arguments(what, ndim, niter, kappa, gamma, voxelspacing, option):
    """(niter, kappa, gamma, spacing as a float64 array or None, option), or ValueError: before any device call"""
    try:
        n = int(niter)
        ok = n == niter and n >= 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: niter must be an integer and not negative, got %r" % (what, niter))
    if option not in (1, 2, 3):
        raise ValueError("%s: option must be 1, 2 or 3, got %r" % (what, option))
    try:
        kappa, gamma = float(kappa), float(gamma)
    except (TypeError, ValueError):
        raise ValueError("%s: kappa and gamma must be numbers, got %r and %r" % (what, kappa, gamma))
    if not (numpy.isfinite(kappa) and kappa > 0):
        raise ValueError("%s: kappa must be finite and positive, got %r" % (what, kappa))
    if not numpy.isfinite(gamma):
        raise ValueError("%s: gamma must be finite, got %r" % (what, gamma))
    sp = None
    if voxelspacing is not None:
        try:
            sp = numpy.array([float(v) for v in voxelspacing], dtype=numpy.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: voxelspacing must be one number per axis, got %r" % (what, voxelspacing))
        if sp.shape != (ndim,):
            raise ValueError("%s: voxelspacing must hold %d values (one per axis), got %r" % (what, ndim, voxelspacing))
        if not (numpy.isfinite(sp).all() and (sp > 0).all()):
            raise ValueError("%s: the voxel spacing must be finite and positive, got %r" % (what, voxelspacing))
    return n, kappa, gamma, sp, int(option)


def anisotropic_diffusion(img, niter=1, kappa=50, gamma=0.1, voxelspacing=None, option=1, graph=None, device=0):
    """Edge-preserving anisotropic diffusion of a 1-D to 3-D image: float32 array of the image's shape.  ``option`` 1 and 2 are the
    two conduction functions of Perona and Malik, 3 is Tukey's biweight; ``kappa`` the conduction coefficient, ``gamma`` the step
    (<= 0.25 for stability), ``voxelspacing`` one value per axis.  Options 2 and 3 give the reference's numbers value for value;
    option 1 takes its exponential in float64 and rounds once (within a few 1e-7 of the value range of the reference).  ``kappa``,
    ``gamma`` and the spacings go through ``float()`` first.  With ``graph=`` and ``img=None`` the graph's own image is diffused on
    its handle and nothing on the graph changes (``VoxelGraph.anisotropic_diffusion(keep=True)`` is the call that keeps the result on
    the device)."""
    from .. import _lib
    what = "anisotropic_diffusion"
    if graph is not None:
        g = getattr(graph, "_inner", graph)
        shape = tuple(g._shape)
        if img is None:
            return g.anisotropic_diffusion(niter, kappa, gamma, voxelspacing, option)
        img = numpy.asarray(img)
        if img.shape != shape:
            raise ValueError("%s: the image has shape %s, the graph %s" % (what, img.shape, shape))
        device = getattr(g, "_device", device)   # an image of the caller's runs on the graph's device
    else:
        if img is None:
            raise ValueError("%s: img=None stands for the image of graph=..., and no graph was given" % what)
        img = numpy.asarray(img)
    if img.ndim < 1 or img.ndim > 3:
        raise NotImplementedError("medpy_amd.filter.smoothing: %d-D images are not implemented (1-D..3-D are)" % img.ndim)
    n, kappa, gamma, sp, option = check_arguments(what, img.ndim, niter, kappa, gamma, voxelspacing, option)
    if img.size == 0:
        raise ValueError("%s: the image is empty" % what)
    from ..graphcut.graph import _device_image
    image = _device_image(img)
    out = numpy.empty(image.shape, dtype=numpy.float32)
    shp = (C.c_int64 * image.ndim)(*image.shape)
    rc = _lib.load().mgc_diffuse_image(int(device), image.ndim, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], n, kappa, gamma, None if sp is None else _lib.ptr(sp),
                                       option, _lib.ptr(out), None)
    _lib.check(None, rc)
    return out
