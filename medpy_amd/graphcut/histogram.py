"""The histogram regional term of interactive graph cut (Boykov & Jolly), in plain NumPy: THE definition of the term.

The intensities under the foreground and the background markers are counted per bin, and every voxel gets the t-links
``-lam * ln Pr(I_p | bkg)`` (source) and ``-lam * ln Pr(I_p | obj)`` (sink).  The device path (``mgc_marker_histograms``,
``mgc_add_tweights_binned``) counts and expands with the same rule, bit for bit; the tables in between are computed
here, on the host, by ``histogram_tables``.  Graphs that do not take the device path evaluate the whole term with these functions
(``GCGraph.record_regional_histogram``).
"""
import math

import numpy

MAX_BINS = 65536


def _check_binning(nbins, lo, width):
    if not (isinstance(nbins, (int, numpy.integer)) and not isinstance(nbins, bool) and 1 <= int(nbins) <= MAX_BINS):
        raise ValueError("nbins = %r: a whole number of 1 to %d bins" % (nbins, MAX_BINS))
    if not math.isfinite(lo):
        raise ValueError("lo = %r must be finite" % (lo,))
    if not (math.isfinite(width) and width > 0):
        raise ValueError("width = %r must be finite and > 0" % (width,))
    return int(nbins), float(lo), float(width)


def histogram_binning(image, bins=None):
    """``(nbins, lo, width)`` of an image.  An integer image with ``bins=None`` gets one bin per value: ``lo = min``,
    ``width = 1``, ``nbins = max - min + 1`` -- ValueError above 65536 of them: pass ``bins``.  Otherwise ``bins`` (1 .. 65536)
    equal bins from the minimum to the maximum: ``lo = min``, ``width = (max - min) / bins``; the maximum itself lands in the
    last bin by the clamp of ``histogram_bins``.  A constant image gets ``width = 1``.  ValueError for an empty image, a value
    that is not finite, and ``bins`` outside 1 .. 65536 (``None`` on a float image included)."""
    image = numpy.asarray(image)
    if image.size == 0:
        raise ValueError("histogram_binning of an empty image")
    if image.dtype.kind not in "biuf":
        raise ValueError("histogram_binning of an image of dtype %s" % image.dtype)
    if image.dtype.kind == "f" and not numpy.isfinite(image).all():
        raise ValueError("histogram_binning: the image holds values that are not finite")
    mn, mx = image.min(), image.max()
    lo = float(mn)
    if bins is None:
        if image.dtype.kind == "f":
            raise ValueError("histogram_binning: bins=None needs an integer image; pass bins (1 .. %d) for dtype %s" % (MAX_BINS, image.dtype))
        nbins = int(mx) - int(mn) + 1
        if nbins > MAX_BINS:
            raise ValueError("histogram_binning: the image spans %d values, more than %d bins of width 1: pass bins" % (nbins, MAX_BINS))
        return nbins, lo, 1.0
    if isinstance(bins, bool) or not isinstance(bins, (int, numpy.integer)) or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError("histogram_binning: bins = %r outside 1 .. %d" % (bins, MAX_BINS))
    bins = int(bins)
    span = float(mx) - lo
    width = span / bins if span > 0 else 1.0
    if not (math.isfinite(width) and width > 0):
        raise ValueError("histogram_binning: the range %r .. %r of the image gives no finite positive bin width" % (mn, mx))
    return bins, lo, width


def histogram_bins(image, nbins, lo, width):
    """the bin of every value, int64 in the image's shape: ``clip(floor((image.astype(float64) - lo) / width), 0, nbins - 1)`` --
    one float64 subtraction, one division, a floor and the clamp; the rule of medpy_amd/csrc/mgc_binned.h"""
    nbins, lo, width = _check_binning(nbins, lo, width)
    image = numpy.asarray(image)
    with numpy.errstate(over="ignore"):   # (a value far outside the range over a tiny width: +-inf, clamped like any other)
        return numpy.clip(numpy.floor((image.astype(numpy.float64) - lo) / width), 0, nbins - 1).astype(numpy.int64)


def histogram_tables(fg_hist, bg_hist, lam=1.0, eps=0.5):
    """``(source_table, sink_table)`` of two histograms of equal length: with ``p_fg = (fg_hist + eps) / (fg_hist.sum() + nbins * eps)``
    and ``p_bg`` likewise, ``source_table = -lam * ln p_bg`` and ``sink_table = -lam * ln p_fg`` -- the source is the foreground, as
    in ``regional_probability_map``: an intensity the background strokes never showed gets a strong link to the source.  ``eps``
    (> 0) keeps empty bins finite, ``lam`` (>= 0) weighs the term against the boundary term.  No smoothing: a caller who wants it
    smooths the histograms first.  ValueError unless ``eps > 0`` and ``lam >= 0``, both finite, and for histograms of different
    lengths, of no bins, or with negative or non-finite counts."""
    lam, eps = float(lam), float(eps)
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError("histogram_tables: eps = %r must be finite and > 0" % (eps,))
    if not (math.isfinite(lam) and lam >= 0):
        raise ValueError("histogram_tables: lam = %r must be finite and >= 0" % (lam,))
    fg = numpy.asarray(fg_hist, dtype=numpy.float64).ravel()
    bg = numpy.asarray(bg_hist, dtype=numpy.float64).ravel()
    if fg.size != bg.size or fg.size == 0:
        raise ValueError("histogram_tables: histograms of %d and %d bins" % (fg.size, bg.size))
    for h in (fg, bg):
        if not numpy.isfinite(h).all() or (h < 0).any():
            raise ValueError("histogram_tables: counts must be finite and >= 0")
    nbins = fg.size
    p_fg = (fg + eps) / (fg.sum() + nbins * eps)
    p_bg = (bg + eps) / (bg.sum() + nbins * eps)
    source_table = -lam * numpy.log(p_bg)
    sink_table = -lam * numpy.log(p_fg)
    return numpy.ascontiguousarray(source_table + 0.0), numpy.ascontiguousarray(sink_table + 0.0)   # (+ 0.0: -0.0 -> 0.0 where lam = 0 or p = 1)


def marker_histograms(image, fg, bg, nbins, lo, width):
    """``(fg_hist, bg_hist, bins)`` on the host: ``numpy.bincount`` of the bins under the two marker masks (None: no markers of that
    kind; a voxel under both counts in both), int64, and the bins of every voxel (flat) for the ``take`` that follows"""
    bins = histogram_bins(numpy.asarray(image).reshape(-1), nbins, lo, width)
    out = []
    for m in (fg, bg):
        if m is None:
            out.append(numpy.zeros(nbins, dtype=numpy.int64))
        else:
            out.append(numpy.bincount(bins[numpy.asarray(m).reshape(-1) != 0], minlength=nbins).astype(numpy.int64))
    return out[0], out[1], bins
