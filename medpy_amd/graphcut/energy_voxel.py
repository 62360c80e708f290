"""Voxel energy terms: same names, signatures and argument tuples as reference
medpy/graphcut/energy_voxel.py, usable as ``boundary_term`` / ``regional_term`` plug-ins of
``graph_from_voxels``.

The reference evaluates g(.) with NumPy and then inserts every edge with one Python call
(energy_voxel.py:660-664).  Here a term only *records* itself on the graph facade; the
weights are computed by the HIP kernel ``k_build`` (medpy_amd/csrc/mgc_kernels.hip) for all
six neighbours of every voxel while the residual lattice is laid out in HBM.
"""
import numpy

from .graph import GCGraph

__all__ = [
    "regional_probability_map",
    "boundary_maximum_linear", "boundary_difference_linear",
    "boundary_maximum_exponential", "boundary_difference_exponential",
    "boundary_maximum_division", "boundary_difference_division",
    "boundary_maximum_power", "boundary_difference_power",
    "boundary_precomputed", "regional_precomputed", "regional_histogram", "regional_geodesic",
]


def _need_facade(graph):
    if not isinstance(graph, GCGraph):
        raise TypeError("medpy_amd energy terms work on medpy_amd.graphcut.GCGraph objects "
                        "(as created by medpy_amd.graphcut.graph_from_voxels), got {}".format(type(graph)))


def regional_probability_map(graph, xxx_todo_changeme):
    """Regional term from a foreground probability map; reference energy_voxel.py:33-65.

    t-links (p*alpha, (1-p)*alpha) per voxel, evaluated in the dtype of the map as NumPy does.
    """
    (probability_map, alpha) = xxx_todo_changeme
    _need_facade(graph)
    graph.record_regional(numpy.asarray(probability_map), alpha)


def boundary_maximum_linear(graph, xxx_todo_changeme1):
    """w = 1 - max(|Ip|,|Iq|) / max|I|; reference energy_voxel.py:68-114."""
    (gradient_image, spacing) = xxx_todo_changeme1
    _need_facade(graph)
    graph.record_boundary("maximum_linear", gradient_image, None, spacing)


def boundary_difference_linear(graph, xxx_todo_changeme2):
    """w = 1 - |Ip-Iq| / |max I - min I|; reference energy_voxel.py:117-191."""
    (original_image, spacing) = xxx_todo_changeme2
    _need_facade(graph)
    graph.record_boundary("difference_linear", original_image, None, spacing)


def boundary_maximum_exponential(graph, xxx_todo_changeme3):
    """w = exp(-max(|Ip|,|Iq|)^2 / sigma^2); reference energy_voxel.py:194-238."""
    (gradient_image, sigma, spacing) = xxx_todo_changeme3
    _need_facade(graph)
    graph.record_boundary("maximum_exponential", gradient_image, sigma, spacing)


def boundary_difference_exponential(graph, xxx_todo_changeme4):
    """w = exp(-|Ip-Iq|^2 / sigma^2); reference energy_voxel.py:241-302."""
    (original_image, sigma, spacing) = xxx_todo_changeme4
    _need_facade(graph)
    graph.record_boundary("difference_exponential", original_image, sigma, spacing)


def boundary_maximum_division(graph, xxx_todo_changeme5):
    """w = 1 / (1 + |Ip-Iq| / sigma): the reference routes this through the *difference*
    skeleton (energy_voxel.py:347); kept for parity.  Reference energy_voxel.py:305-347."""
    (gradient_image, sigma, spacing) = xxx_todo_changeme5
    _need_facade(graph)
    graph.record_boundary("maximum_division", gradient_image, sigma, spacing)


def boundary_difference_division(graph, xxx_todo_changeme6):
    """w = 1 / (1 + |Ip-Iq| / sigma); reference energy_voxel.py:350-409."""
    (original_image, sigma, spacing) = xxx_todo_changeme6
    _need_facade(graph)
    graph.record_boundary("difference_division", original_image, sigma, spacing)


def boundary_maximum_power(graph, xxx_todo_changeme7):
    """w = (1 / (1 + max(|Ip|,|Iq|)))^sigma; reference energy_voxel.py:412-452."""
    (gradient_image, sigma, spacing) = xxx_todo_changeme7
    _need_facade(graph)
    graph.record_boundary("maximum_power", gradient_image, sigma, spacing)


def boundary_difference_power(graph, xxx_todo_changeme8):
    """w = (1 / (1 + |Ip-Iq|))^sigma; reference energy_voxel.py:455-516."""
    (original_image, sigma, spacing) = xxx_todo_changeme8
    _need_facade(graph)
    graph.record_boundary("difference_power", original_image, sigma, spacing)


def boundary_precomputed(graph, xxx_todo_changeme9):
    """Boundary term from weights the caller has evaluated already (extension; no reference counterpart): a gradient-magnitude
    map, a learned edge probability, a directed penalty.  ``weights`` is a sequence of one entry per array axis, in axis order;
    entry k holds the weights of the pairs (p, p + e_k), either one array (symmetric) or a pair ``(there, back)`` for the arcs
    p -> p + e_k and p + e_k -> p.  Arrays have the shape of the volume (the last slice along axis k is ignored) or the layout
    of the reference's ``__skeleton_base`` (extent - 1 along axis k).  They reach the tile solver as whole arrays
    (``GCGraph.set_nweights_dense``), not edge by edge."""
    (weights,) = xxx_todo_changeme9
    _need_facade(graph)
    weights = list(weights)
    ndim = len(graph.get_shape())
    if len(weights) != ndim:
        raise ValueError("{} weight entries for a volume of {} axes".format(len(weights), ndim))
    for axis, w in enumerate(weights):
        if isinstance(w, (tuple, list)) and len(w) == 2 and numpy.ndim(w[0]) == ndim:
            graph.set_nweights_dense(axis, w[0], w[1])
        else:
            graph.set_nweights_dense(axis, w)


def regional_precomputed(graph, xxx_todo_changeme10):
    """Regional term from t-link weights the caller has evaluated already (extension; no reference counterpart): negative
    log-likelihoods of a mixture model or a histogram, the output of a network.  ``weights_source[p]`` / ``weights_sink[p]``
    are the capacities of the links source -> p and p -> sink, arrays of the volume's shape.  They reach the tile solver as whole
    arrays (``GCGraph.set_tweights_dense``), not voxel by voxel."""
    (weights_source, weights_sink) = xxx_todo_changeme10
    _need_facade(graph)
    graph.set_tweights_dense(weights_source, weights_sink)


def regional_histogram(graph, xxx_todo_changeme11):
    """Regional term of interactive graph cut (Boykov & Jolly; extension, no reference counterpart): the intensity histograms of
    the voxels under the foreground and under the background markers give every voxel the t-links ``-lam * ln Pr(I_p | bkg)``
    (source) and ``-lam * ln Pr(I_p | obj)`` (sink).  ``image``: an array of the volume's shape; ``bins``: None for one bin per
    value of an integer image, else the number of equal bins between its minimum and maximum; ``lam`` weighs the term against
    the boundary term, ``eps`` (> 0) is added to every count.  ``medpy_amd.graphcut.histogram`` is the definition of the term.
    On the tile solver histograms and t-links are computed on the device from the resident image and markers, and
    ``VoxelGraph.refit_regional_histogram()`` fits the term again after ``edit_markers``."""
    (image, bins, lam, eps) = xxx_todo_changeme11
    _need_facade(graph)
    graph.record_regional_histogram(image, bins, lam, eps)


def regional_geodesic(graph, xxx_todo_changeme12):
    """Geodesic regional term (GeoS; Price et al., "Geodesic graph cut"; extension, no reference counterpart): with D_F and D_B
    the geodesic distances of a voxel to the foreground and to the background markers -- shortest lattice paths whose arcs
    cost ``step`` times their length plus ``gamma`` times the intensity step they cross -- every voxel gets the t-links
    ``lam * D_B / (D_F + D_B)`` (source) and ``lam * D_F / (D_F + D_B)`` (sink).  Arguments ``(gamma, lam[, step[, spacing[,
    connectivity[, image]]]])``: ``step`` defaults to 1, ``spacing`` to unity, ``connectivity`` (1 or the number of axes) to the
    graph's own, ``image`` to the boundary term's image.  Distances and t-links are computed on the device from the resident
    image and markers (``GCGraph.record_regional_geodesic``), and ``VoxelGraph.refit_regional_geodesic()`` fits the term again
    after ``edit_markers``."""
    args = tuple(xxx_todo_changeme12)
    if not 2 <= len(args) <= 6:
        raise ValueError("regional_geodesic takes (gamma, lam[, step[, spacing[, connectivity[, image]]]]), got {} values".format(len(args)))
    _need_facade(graph)
    graph.record_regional_geodesic(*args)
