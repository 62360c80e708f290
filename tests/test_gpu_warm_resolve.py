"""-m gpu: warm re-solves after marker / regional-term edits (VoxelGraph.update_markers / update_regional_term, C ABI
mgc_update_markers / mgc_update_regional_probability).  Every warm cut is held against (i) a COLD graph_from_voxels of
the same inputs in the same library -- labels identical, flow == (both are functions of the labels and the inputs, so bit
equality is owed) -- and (ii) the BK oracle, and the preflow it leaves must pass mgc_validate."""
import numpy as np
import pytest

from oracle import pipeline

pytestmark = pytest.mark.gpu


def _kwargs(s, reg=None, conn=None, boundary=None):
    from medpy_amd import graphcut
    kw = dict(boundary_term=boundary or graphcut.energy_voxel.boundary_difference_exponential,
              boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return kw


def _graph(fg, bg, s, reg=None, conn=None, boundary=None):
    from medpy_amd import graphcut
    return graphcut.graph_from_voxels(fg, bg, **_kwargs(s, reg, conn, boundary))


def _check(g, fg, bg, s, reg=None, conn=None, boundary=None, oracle=True):
    """the warm cut of g (inputs fg / bg / reg now) against a cold build and the BK oracle; returns (flow, labels)"""
    from medpy_amd import _lib
    flow = g.maxflow()
    labels = g.labels().copy()
    cold = _graph(fg, bg, s, reg, conn, boundary)
    cflow = cold.maxflow()
    assert np.array_equal(labels, cold.labels()), "warm and cold labels differ in %d voxels" % int((labels != cold.labels()).sum())
    assert flow == cflow, (flow, cflow)
    cold.close()
    if oracle:
        ref = pipeline.graphcut_voxel(fg, bg, term=s["term"], image=s["image"], sigma=s["sigma"],
                                      prob=None if reg is None else reg["prob"], alpha=None if reg is None else reg["alpha"],
                                      connectivity=conn)
        assert np.array_equal(labels, ref.labels), "labels differ from the BK oracle in %d voxels" % int((labels != ref.labels).sum())
        assert flow == pytest.approx(ref.flow, rel=1e-9)
    v = g.validate()
    _lib.assert_valid(v)
    assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9
    assert flow == pytest.approx(v["cut_capacity"] + v["flow_constant"], rel=1e-12)
    flat = labels.ravel()
    for i in (int(np.argmin(flat)), int(np.argmax(flat))):
        assert g.what_segment(i) == (g.termtype.SOURCE if flat[i] else g.termtype.SINK)
    return flow, labels


def _stroke(shape, lo, hi):
    """voxels on the ray from the centre along the last axis at distances [lo * n, hi * n), two or three voxels wide across it"""
    n = min(shape)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    m = np.ones(shape, dtype=bool)
    for k, (g, s) in enumerate(zip(grids, shape)):
        c = (s - 1) / 2.0
        m = m & (((g - c) >= lo * n) & ((g - c) < hi * n) if k == len(shape) - 1 else np.abs(g - c) <= 1)
    return m


def _edits(s):
    """the edits of an interactive session on synthetic.sphere: (name, fg, bg)"""
    fg, bg = s["fg"], s["bg"]
    shape = fg.shape
    no_face = bg.copy()
    no_face[0] = False
    return [("leak_fix", fg, bg | _stroke(shape, 0.15, 0.25)),      # background stroke inside the bright ball
            ("fg_outside", fg | _stroke(shape, 0.35, 0.45), bg),    # foreground stroke outside it
            ("face_removed", fg, no_face),                          # part of the face markers taken away
            ("identical", fg, bg)]


@pytest.mark.parametrize("n", [32, 64, 96])
@pytest.mark.parametrize("edit", ["leak_fix", "fg_outside", "face_removed", "identical"])
def test_marker_edit_6(n, edit):
    from medpy_amd import synthetic
    s = synthetic.sphere((n, n, n))
    g = _graph(s["fg"], s["bg"], s)
    flow_a = g.maxflow()
    labels_a = g.labels().copy()
    _, fg, bg = [e for e in _edits(s) if e[0] == edit][0]
    g.update_markers(fg, bg)
    flow, labels = _check(g, fg, bg, s)
    if edit == "identical":
        assert flow == flow_a and np.array_equal(labels, labels_a)


def test_chain_of_five_edits():
    from medpy_amd import synthetic
    s = synthetic.sphere((48, 48, 48))
    shape = s["fg"].shape
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    fg, bg = s["fg"], s["bg"]
    no_face = bg.copy()
    no_face[-1] = False
    chain = [(fg, bg | _stroke(shape, 0.15, 0.25)),
             (fg | _stroke(shape, 0.35, 0.45), bg | _stroke(shape, 0.15, 0.25)),
             (fg | _stroke(shape, 0.35, 0.45), no_face),
             (fg, no_face | _stroke(shape, -0.25, -0.15)),
             (fg, bg)]
    for fg_k, bg_k in chain:
        g.update_markers(fg_k, bg_k)
        _check(g, fg_k, bg_k, s)


def test_tiles_gain_and_lose_every_tlink():
    """64^3: the fg ball (r < 6.4 around 31.5) spans tiles 3 and 4 of every axis.  Clearing the fg markers of tile (3, 3, 3) takes
    every t-link from that tile -- its former source voxels whose flow left through their n-links keep a residual sink link under
    tr0 = 0 -- and strokes far from everything give t-links to tiles that had none; then both at once, and back."""
    from medpy_amd import synthetic
    s = synthetic.sphere((64, 64, 64))
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    fg_cut = s["fg"].copy()
    fg_cut[24:32, 24:32, 24:32] = False
    assert fg_cut.any() and not fg_cut[24:32, 24:32, 24:32].any()
    g.update_markers(fg_cut, s["bg"])
    _check(g, fg_cut, s["bg"], s)
    far_fg = np.zeros_like(s["fg"])
    far_fg[10:13, 10:12, 50:54] = True  # inside tiles that held no t-link: (1, 1, 6)
    far_bg = s["bg"].copy()
    far_bg[40:42, 12:15, 12:15] = True  # ... (5, 1, 1)
    g.update_markers(s["fg"] | far_fg, far_bg)
    _check(g, s["fg"] | far_fg, far_bg, s)
    g.update_markers(fg_cut | far_fg, s["bg"])
    _check(g, fg_cut | far_fg, s["bg"], s)
    g.update_markers(s["fg"], s["bg"])
    _check(g, s["fg"], s["bg"], s)


def test_update_before_the_first_maxflow():
    from medpy_amd import synthetic
    s = synthetic.sphere((40, 40, 40))
    fg, bg = s["fg"] | _stroke(s["fg"].shape, 0.35, 0.45), s["bg"] | _stroke(s["fg"].shape, 0.15, 0.25)
    g = _graph(s["fg"], s["bg"], s)
    g.update_markers(fg, bg)
    _check(g, fg, bg, s)


@pytest.mark.parametrize("conn", [None, 26])
def test_regional_term(conn):
    """config-3-shaped (sphere + regional map), 48^3: a new probability map, then a new alpha, then a marker edit on top"""
    from medpy_amd import synthetic
    shape = (48, 48, 48)
    s = synthetic.sphere(shape)
    r1 = synthetic.regional(shape, seed=1)
    g = _graph(s["fg"], s["bg"], s, r1, conn)
    g.maxflow()
    r2 = synthetic.regional(shape, seed=2)
    g.update_regional_term(r2["prob"], r2["alpha"])
    _check(g, s["fg"], s["bg"], s, r2, conn)
    r3 = dict(prob=r2["prob"], alpha=0.7)
    g.update_regional_term(r3["prob"], r3["alpha"])
    _check(g, s["fg"], s["bg"], s, r3, conn)
    bg = s["bg"] | _stroke(shape, 0.15, 0.25)
    g.update_markers(s["fg"], bg)
    _check(g, s["fg"], bg, s, r3, conn)


def test_regional_term_added_to_a_graph_built_without_one():
    from medpy_amd import synthetic
    shape = (40, 40, 40)
    s = synthetic.sphere(shape)
    g = _graph(s["fg"], s["bg"], s)
    g.maxflow()
    r = synthetic.regional(shape)
    prob64 = r["prob"].astype(np.float64)
    g.update_regional_term(prob64, 0.3)
    _check(g, s["fg"], s["bg"], s, dict(prob=prob64, alpha=0.3))


def test_full_neighbourhood_markers_only():
    from medpy_amd import synthetic
    s = synthetic.sphere((48, 48, 48))
    g = _graph(s["fg"], s["bg"], s, conn=26)
    g.maxflow()
    for _, fg, bg in _edits(s)[:3]:
        g.update_markers(fg, bg)
        _check(g, fg, bg, s, conn=26)


@pytest.mark.parametrize("shape,conn", [((96, 80), None), ((96, 80), 8), ((600,), None)])
def test_two_and_one_dimensional(shape, conn):
    from medpy_amd import synthetic
    s = synthetic.sphere(shape)
    g = _graph(s["fg"], s["bg"], s, conn=conn)
    g.maxflow()
    for _, fg, bg in _edits(s):
        g.update_markers(fg, bg)
        _check(g, fg, bg, s, conn=conn)


def test_plugin_edges_survive_an_update():
    """explicit lattice edges that a plug-in boundary term adds on top of the built-in one stay part of the graph"""
    from medpy_amd import graphcut, synthetic
    s = synthetic.sphere((40, 40, 40))
    shape = s["fg"].shape
    ids = np.arange(s["fg"].size).reshape(shape)
    line = ids[19, 19, 20:34]  # a strong chain of x-neighbours from inside the ball out through its surface

    def boundary(graph, args):
        graphcut.energy_voxel.boundary_difference_exponential(graph, args)
        for a, b in zip(line[:-1], line[1:]):
            graph.set_nweight(int(a), int(b), 2.0, 2.0)

    g = _graph(s["fg"], s["bg"], s, boundary=boundary)
    flow_a = g.maxflow()
    plain = _graph(s["fg"], s["bg"], s)
    assert flow_a != plain.maxflow()  # the edges are part of the cut
    plain.close()
    for _, fg, bg in _edits(s)[:3]:
        g.update_markers(fg, bg)
        _check(g, fg, bg, s, boundary=boundary, oracle=False)


def test_error_paths():
    from medpy_amd import _lib, graphcut, synthetic
    from medpy_amd.graphcut.graph import EmbeddedLatticeGraph, VoxelGraph
    s = synthetic.sphere((24, 24, 24))
    # before mgc_build
    g = VoxelGraph(s["fg"].shape)
    g._set_boundary("difference_exponential", s["image"], s["sigma"], False)
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_markers(s["fg"], s["bg"])
    assert ei.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_regional_term(np.full(s["fg"].shape, 0.5, np.float32), 0.5)
    assert ei.value.code == _lib.ERR_STATE
    g.close()
    # a shape other than the volume's
    g = _graph(s["fg"], s["bg"], s)
    with pytest.raises(ValueError):
        g.update_markers(s["fg"][1:], s["bg"])
    with pytest.raises(ValueError):
        g.update_markers(s["fg"], s["bg"].reshape(24, 576))
    with pytest.raises(ValueError):
        g.update_regional_term(np.full((24, 24, 23), 0.5, np.float32), 0.5)
    # after an update, a rebuild (mgc_build of the inputs resident now) gives the cold result again
    bg = s["bg"] | _stroke(s["fg"].shape, 0.15, 0.25)
    g.maxflow()
    g.update_markers(s["fg"], bg)
    g._build()
    _check(g, s["fg"], bg, s)
    # graphs that went to the sparse-graph solver
    s4 = synthetic.sphere((6, 6, 6, 6))
    g4 = _graph(s4["fg"], s4["bg"], s4)
    assert not isinstance(g4, VoxelGraph)
    with pytest.raises(NotImplementedError):
        g4.update_markers(s4["fg"], s4["bg"])
    with pytest.raises(NotImplementedError):
        g4.update_regional_term(np.full(s4["fg"].shape, 0.5), 0.5)
    fg2, bg2 = np.zeros((4, 4), bool), np.zeros((4, 4), bool)
    fg2[0, 0], bg2[3, 3] = True, True
    ge = graphcut.graph_from_voxels(fg2, bg2, boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                    boundary_term_args=(np.arange(9, dtype=np.float64).reshape(3, 3), 1.0, False))
    assert isinstance(ge, EmbeddedLatticeGraph)
    with pytest.raises(NotImplementedError):
        ge.update_markers(fg2, bg2)


def test_no_update_after_a_solve_that_did_not_converge():
    from medpy_amd import _lib, synthetic
    s = synthetic.sphere((96, 96, 96))
    g = _graph(s["fg"], s["bg"], s)
    g.set_param("max_outer", 1)
    with pytest.raises(_lib.MedpyHipError):
        g.maxflow()
    with pytest.raises(_lib.MedpyHipError) as ei:
        g.update_markers(s["fg"], s["bg"])
    assert ei.value.code == _lib.ERR_STATE
    g.set_param("max_outer", 100000)
    g._build()
    g.maxflow()
    bg = s["bg"] | _stroke(s["fg"].shape, 0.15, 0.25)
    g.update_markers(s["fg"], bg)
    _check(g, s["fg"], bg, s)
