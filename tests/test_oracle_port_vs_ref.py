"""oracle/bk_maxflow.c (C restatement) must be indistinguishable from the unmodified reference
solver: same flow bits, labels, residual t-links as the reference (compiled in place as oracle/_ref/libbkref.so) gave for
the same calls, stored in tests/golden/reference_oracle.npz (oracle/gen_golden.py oracle).  Where the compiled reference
is here too, it is held to the stored outputs as well."""
import os

import numpy as np
import pytest

from oracle import bk, pipeline
from oracle.gen_golden import ORACLE_LATTICES, lattice_key, oracle_graphs

KINDS = ["port"] + (["ref"] if bk.available("ref") else [])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_oracle.npz"))


def _solve(kind, n, i, j, cap, rev, src, snk):
    g = bk.BKGraph(n, max(len(i), 1), kind)
    if len(i):
        g.sum_edges(i, j, cap, rev)
    g.add_tweights(None, src, snk)
    f = g.maxflow()
    return f, g.labels(), np.array([g.get_trcap(k) for k in range(n)]), g.get_arc_num()


def test_random_graphs_bitwise(golden):
    for kind in KINDS:
        for t, case in enumerate(oracle_graphs()):
            key = "graph%03d/" % t
            f, labels, trcap, arcs = _solve(kind, *case)
            assert f == golden[key + "flow"], (kind, t)
            np.testing.assert_array_equal(labels, golden[key + "labels"]); np.testing.assert_array_equal(trcap, golden[key + "trcap"])
            assert arcs == golden[key + "arc_num"]


def test_sum_edge_and_realloc():
    """reference lib/maxflow/src/sum_edge_test.py:20-79: repeated pairs accumulate; exceeding the edge hint reallocs."""
    for kind in KINDS:
        g = bk.BKGraph(4, 1, kind)
        g.sum_edges([0, 0, 1, 2, 0], [1, 1, 2, 3, 2], [1., 2., 1., 1., 4.], [0.5, 0.5, 1., 1., 4.])
        assert g.get_edge(0, 1) == 3.0 and g.get_edge(1, 0) == 1.0 and g.get_edge(3, 0) == 0.0
        assert g.get_arc_num() == 8
        g2 = bk.BKGraph(40, 1, kind)
        i = np.arange(39); g2.sum_edges(i, i + 1, np.ones(39))
        g2.add_tweights([0], [5.0], [0.0]); g2.add_tweights([39], [0.0], [5.0])
        assert g2.maxflow() == 1.0


@pytest.mark.parametrize("gen,shape", ORACLE_LATTICES)
def test_lattices_bitwise(gen, shape, golden):
    from medpy_amd import synthetic
    s = getattr(synthetic, gen)(shape)
    key = lattice_key(gen, shape) + "/"
    for kind in KINDS:
        cut = pipeline.graphcut_voxel(s["fg"], s["bg"], kind=kind, term=s["term"], image=s["image"], sigma=s["sigma"])
        assert cut.flow == golden[key + "flow"], kind
        np.testing.assert_array_equal(cut.labels, golden[key + "labels"])
