"""CPU tier of the dense n-link weight arrays: the padding helper, the facade's argument checks -- all of them raised
before anything is recorded or any device is touched -- and the two new names of the C ABI."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1,), (2,), (7,), (1, 5), (4, 1), (3, 5), (1, 1, 4), (3, 1, 5), (2, 3, 4), (9, 8, 7)]


def _pad_restated(shape, axis, w):
    """the skeleton array with a slice of zeros appended along `axis`"""
    tail = list(shape)
    tail[axis] = 1
    return np.concatenate([w, np.zeros(tail, dtype=w.dtype)], axis=axis)


@pytest.mark.parametrize("shape", SHAPES)
def test_pad_skeleton_weights_every_axis(shape):
    from medpy_amd.graphcut.graph import pad_skeleton_weights
    rng = np.random.default_rng(len(shape) * 100 + sum(shape))
    for axis in range(len(shape)):
        sk = tuple(n - 1 if k == axis else n for k, n in enumerate(shape))
        for dtype in (np.float64, np.float32):
            w = rng.uniform(0.1, 10.0, sk).astype(dtype)
            out = pad_skeleton_weights(shape, axis, w)
            want = _pad_restated(shape, axis, w)
            assert out.shape == tuple(shape) and out.dtype == dtype and out.flags.c_contiguous
            assert np.array_equal(out, want)
        with pytest.raises(ValueError):
            pad_skeleton_weights(shape, axis, np.zeros(shape))   # the full shape is not the skeleton layout


def _facade(shape, connectivity=None):
    from medpy_amd.graphcut import GCGraph
    return GCGraph(int(np.prod(shape)), 0, shape=shape, connectivity=connectivity)


def test_wrong_shape_is_a_value_error():
    g = _facade((4, 5, 6))
    for bad in ((4, 5), (5, 5, 6), (4, 5, 6, 1), (3, 4, 5)):
        with pytest.raises(ValueError):
            g.set_nweights_dense(0, np.ones(bad))
    with pytest.raises(ValueError):
        g.set_nweights_dense(1, np.ones((3, 5, 6)))          # the skeleton layout of axis 0, given for axis 1
    with pytest.raises(ValueError):
        g.set_nweights_dense((-1, 0, 0), np.ones((3, 5, 6)))  # the skeleton layout belongs to the forward offset
    with pytest.raises(ValueError):
        g.set_nweights_dense(0, np.ones((4, 5, 6)), np.ones((4, 5)))
    with pytest.raises(ValueError):
        g.set_nweights_dense(0, np.array([["a"]]))
    # the accepted forms, for contrast: full shape, skeleton layout, integer dtype, a pair
    g.set_nweights_dense(0, np.ones((4, 5, 6)))
    g.set_nweights_dense(0, np.ones((3, 5, 6), np.float32))
    g.set_nweights_dense((0, 0, -1), np.ones((4, 5, 6), np.int16), np.ones((4, 5, 6)))


@pytest.mark.parametrize("shape,connectivity,bad", [
    ((4, 5, 6), None, [(1, 1, 0), (0, 0, 0), (2, 0, 0), (1, 0), (0, -1, 1), 3, -1, (0.5, 0, 0)]),
    ((4, 5, 6), 26, [(0, 0, 0), (2, 0, 0), (1, 0), (1, 1, 1, 1), 3]),
    ((4, 5), 4, [(1, 1), (1, -1), (0, 0), 2]),
    ((4, 5), 8, [(0, 0), (0, 2), (1, 1, 0)]),
])
def test_offset_that_is_no_neighbour_is_a_value_error(shape, connectivity, bad):
    g = _facade(shape, connectivity)
    for off in bad:
        with pytest.raises(ValueError):
            g.set_nweights_dense(off, np.ones(shape))
    if connectivity in (8, 26):
        g.set_nweights_dense((1,) * len(shape), np.ones(shape))       # a diagonal is a neighbour here
        g.set_nweights_dense((-1,) + (1,) * (len(shape) - 1), np.ones(shape))


def test_pair_whose_halves_differ_in_shape_is_a_value_error():
    from medpy_amd.graphcut import energy_voxel
    g = _facade((4, 5, 6))
    with pytest.raises(ValueError):
        g.set_nweights_dense(2, np.ones((4, 5, 6)), np.ones((4, 5, 5)))   # full shape / skeleton layout: each valid alone
    with pytest.raises(ValueError):
        g.set_nweights_dense(2, np.ones((4, 5, 5)), np.ones((4, 5, 6)))
    full = np.ones((4, 5, 6))
    with pytest.raises(ValueError):
        energy_voxel.boundary_precomputed(g, ([full, full, (full, np.ones((4, 5, 5)))],))
    with pytest.raises(ValueError):
        energy_voxel.boundary_precomputed(g, ([full, full],))               # one entry per axis


def test_graphs_of_the_sparse_solver_raise_not_implemented():
    from medpy_amd.graphcut import GCGraph
    g = GCGraph(24, 0)                                   # no lattice shape
    with pytest.raises(NotImplementedError):
        g.set_nweights_dense(0, np.ones(24))
    g = GCGraph(16, 0, shape=(2, 2, 2, 2))               # 4-D
    with pytest.raises(NotImplementedError):
        g.set_nweights_dense(0, np.ones((2, 2, 2, 2)))
    g = GCGraph(16, 0, shape=(4, 4))                     # an embedded boundary image
    g.record_boundary("difference_linear", np.zeros((3, 3)), None, False)
    with pytest.raises(NotImplementedError):
        g.set_nweights_dense(0, np.ones((4, 4)))


def test_header_and_signatures_hold_the_two_calls():
    import ctypes as C
    from medpy_amd import _lib
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    for name, nargs in (("mgc_add_nweights", 5), ("mgc_clear_nweights", 1)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    declared = set(re.findall(r"\b(m[gs][cg]_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
