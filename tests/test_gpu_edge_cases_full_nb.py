"""-m gpu: the degenerate inputs of tests/test_gpu_edge_cases.py again at the full neighbourhood (8 in 2-D, 26 in 3-D) -- the same
helpers, told the connectivity: shapes below one tile and with singleton axes, no markers, one-sided markers, everything marked, the
constant image, the DBL_MIN clamp, solving again and rebuilding -- and explicit edges on the 26-slot layout (k_add_edges, k_refresh_mask):
ordered sums of repeated edges over all 13 forward offsets, inside a tile and through tile faces, edges and corners, and batches added
after a build."""
import numpy as np
import pytest

import full_nb_cases as fc
import test_gpu_edge_cases as ec
from oracle import energy_numpy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 1, 5), (1, 1, 1), (1, 1, 17), (2, 2, 2), (8, 8, 8), (9, 8, 7)], ids=fc.shape_id)
def test_small_and_singleton_shapes(shape):
    ec._small_shape(shape, fc.full_connectivity(len(shape)))


def test_no_markers_at_all():
    ec._no_markers(26)


def test_only_foreground_or_only_background():
    ec._one_sided_markers(26)


def test_everything_marked():
    ec._everything_marked(26)


def test_constant_image_and_huge_dynamic_range():
    ec._constant_and_huge_range(26)


def test_repeated_solve_and_rebuild_are_idempotent():
    ec._solve_again_and_rebuild(26)


def _pairs(shape, seed, count=40):
    """``count`` distinct neighbour pairs over all 13 forward offsets as flat ids, and how many tile borders each crosses"""
    offs = energy_numpy.forward_offsets(3, 26)
    pairs, _ = fc.sample_pairs(shape, offs, seed, count=count)
    pairs = list(dict.fromkeys(pairs))[:count]
    assert {o for _, o in pairs} == set(offs)
    i = np.array([np.ravel_multi_index(p, shape) for p, _ in pairs], dtype=np.int64)
    j = np.array([np.ravel_multi_index(tuple(c + k for c, k in zip(p, o)), shape) for p, o in pairs], dtype=np.int64)
    return i, j, [fc._crossing(p, o) for p, o in pairs]


@pytest.mark.parametrize("shape", [(3, 4, 5), (9, 9, 9)], ids=fc.shape_id)
def test_repeated_explicit_edges_on_diagonal_offsets_sum_in_call_order(shape):
    i, j, crossed = _pairs(shape, seed=11)
    assert 0 in crossed   # some cross nothing
    if shape == (9, 9, 9):
        assert {1, 2, 3} <= set(crossed)   # ... a tile face, a tile edge, a tile corner
    ec._repeated_edges(shape, i, j, np.random.default_rng(6), connectivity=26)


def test_explicit_edge_batches_of_growing_size_and_rebuild():
    ec._edge_batches(26, (1, 1, 1), far=2)       # (0, 2): Chebyshev distance 2 along x
    ec._edge_batches(26, (0, 1, 1), far=2 * 16)  # ... along z
