"""-m gpu: k_dt_axis -- both scans of one axis of a distance transform in one launch, a tile line split over the waves of a workgroup.

The first global relabel alone (MGC_OP_FIRST_RELABEL, read back with mgc_get_heights) must leave the same integers, voxel for voxel,
in three forms: the one-launch-per-axis kernels (first_relabel_dt = 1; the launch counts must say that k_dt_axis ran), the forward +
backward launches of k_dt_scan (first_relabel_dt = 2), and two references on the CPU -- the host simulator's first relabel, which runs
mgc_dt_scan_line itself, and a NumPy min-plus scan.  Shapes: the smallest at which a line split over waves can go wrong (1, 2, 3 and 16
waves a line, ragged last runs, partial tiles, a line one tile too long for a workgroup); every layout also with grids of 1 and 3
workgroups, so that the loop over the lines with its barrier goes round many times.  Then whole solves in both forms against BK."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))

from oracle import energy_numpy, pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

HINF = 0x3f3f3f3f
SHAPES = [(8, 8, 8), (5, 9, 17), (20, 33, 47), (24, 72, 136), (8, 16, 1024), (8, 16, 1032)]
LAYOUTS = ["faces_ball", "corners", "bg_before_tail", "random", "no_bg"]
C_MIN = 8  # (radial_min_c as shipped; the host simulator's first_relabel(.., 3) uses the same)
_VOL = {}


def _volume(shape):
    if shape not in _VOL:
        from medpy_amd import synthetic
        s = synthetic.sphere(shape)
        _VOL[shape] = (s, energy_numpy.boundary_weights(s["term"], s["image"], s["sigma"]))
    return _VOL[shape]


def _markers(shape, layout):
    s = _volume(shape)[0]
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    if layout == "faces_ball":
        fg, bg = s["fg"].copy(), s["bg"].copy()
    elif layout == "corners":  # distances run to D0 + D1 + D2: what enters a wave's run comes from far away
        bg[0, 0, 0] = True
        fg[-1, -1, -1] = True
    elif layout == "bg_before_tail":  # the only sink link on the last real voxel in front of the padding of a partial tile
        bg[-1, -1, -1] = True
        fg[0, 0, 0] = True
    elif layout == "random":
        u = np.random.default_rng(7).random(shape)
        bg, fg = u < 0.01, (u >= 0.01) & (u < 0.02)
    elif layout == "no_bg":
        fg = s["fg"].copy()
        if not fg.any():
            fg[tuple(d // 2 for d in shape)] = True
    return fg, bg & ~fg


def _l1_transform(seed):
    """1 + L1 distance to the nearest True voxel (int64, HINF where there is none): a min-plus scan forward and backward along each axis"""
    big = np.int64(1) << 40
    d = np.where(seed, np.int64(1), big)
    for ax in range(d.ndim):
        d = np.moveaxis(d, ax, 0)
        for i in range(1, d.shape[0]):
            np.minimum(d[i], d[i - 1] + 1, out=d[i])
        for i in range(d.shape[0] - 2, -1, -1):
            np.minimum(d[i], d[i + 1] + 1, out=d[i])
        d = np.moveaxis(d, 0, ax)
    return np.where(d >= big, np.int64(HINF), d)


def _numpy_labels(fg, bg, c_min):
    exact = _l1_transform(bg)
    ds = _l1_transform(fg)
    src = fg & (exact < HINF)
    C = int(exact[src].min()) if src.any() else HINF
    low = exact.copy()
    if C < HINF and C >= c_min:
        ok = (exact < HINF) & (ds < HINF)
        low[ok] = np.minimum(exact[ok], np.maximum(1, C - (ds[ok] - 1)))
    return exact, low


def _untile(h, shape):
    g = [(d + 7) // 8 for d in shape]
    v = h.reshape(g[0], g[1], g[2], 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(g[0] * 8, g[1] * 8, g[2] * 8)
    return v[:shape[0], :shape[1], :shape[2]].astype(np.int64)


def _graph(shape, fg, bg, **params):
    from medpy_amd import graphcut
    s = _volume(shape)[0]
    g = graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                   boundary_term_args=(s["image"], s["sigma"], False))
    for k, v in params.items():
        g.set_param(k, v)
    return g


def _expected_launches(shape, form, transforms):
    """(k_dt_axis, k_dt_scan) launches of `transforms` transforms: one per axis, or two where a line has more than 128 tiles / in form 2"""
    fused = [0 if form == 2 or (d + 7) // 8 > 128 else 1 for d in shape]
    return transforms * sum(fused), transforms * 2 * (3 - sum(fused))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_relabel_in_every_form(shape, layout):
    import sim
    fg, bg = _markers(shape, layout)
    w = _volume(shape)[1]
    tr = (np.where(fg, 65535.0, 0.0) - np.where(bg, 65535.0, 0.0)).ravel()
    ex_np, low_np = _numpy_labels(fg, bg, C_MIN)
    ran, h_sim, _ = sim.first_relabel(shape, w, tr, 1)
    assert ran
    np.testing.assert_array_equal(_untile(h_sim, shape), ex_np)
    ran, h_sim, _ = sim.first_relabel(shape, w, tr, 3)
    assert ran
    np.testing.assert_array_equal(_untile(h_sim, shape), low_np)
    if layout == "no_bg":
        assert (ex_np == HINF).all()
    # the transform towards the sink alone
    for form in (1, 2):
        g = _graph(shape, fg, bg, first_relabel_dt=form)
        g.first_relabel()
        counts = g.launch_counts()
        h = g.heights()
        g.close()
        assert (counts["k_dt_axis"], counts["k_dt_scan"]) == _expected_launches(shape, form, 1), (form, counts)
        np.testing.assert_array_equal(h, ex_np, err_msg="form %d" % form)
    # ... and with the radial labels on top: the labels in use are the lowered ones, the exact ones are kept aside
    for form in (1, 2):
        for cap in (None, 1, 3):
            params = dict(first_relabel_dt=form)
            if cap:
                params["grid_cap"] = cap
            g = _graph(shape, fg, bg, **params)
            g.first_relabel(radial=True, c_min=C_MIN)
            counts = g.launch_counts()
            low, aside = g.heights(), g.heights(aside=True)
            g.close()
            assert (counts["k_dt_axis"], counts["k_dt_scan"]) == _expected_launches(shape, form, 2), (form, cap, counts)
            np.testing.assert_array_equal(aside, ex_np, err_msg="form %d grid_cap %s" % (form, cap))
            np.testing.assert_array_equal(low, low_np, err_msg="form %d grid_cap %s" % (form, cap))


def test_radial_labels_from_one_hop_on():
    """c_min = 1 (the host simulator's first_relabel(.., 7)): the labels are lowered however short the shortest source -> sink path"""
    import sim
    shape = (20, 33, 47)
    fg, bg = _markers(shape, "random")
    tr = (np.where(fg, 65535.0, 0.0) - np.where(bg, 65535.0, 0.0)).ravel()
    ex_np, low_np = _numpy_labels(fg, bg, 1)
    assert (low_np < ex_np).any()
    _, h_sim, _ = sim.first_relabel(shape, _volume(shape)[1], tr, 7)
    np.testing.assert_array_equal(_untile(h_sim, shape), low_np)
    for form in (1, 2):
        g = _graph(shape, fg, bg, first_relabel_dt=form)
        g.first_relabel(radial=True, c_min=1)
        low, aside = g.heights(), g.heights(aside=True)
        g.close()
        np.testing.assert_array_equal(aside, ex_np)
        np.testing.assert_array_equal(low, low_np)


def test_first_relabel_op_is_refused_where_the_transform_does_not_apply():
    from medpy_amd import _lib
    shape = (8, 8, 8)
    fg, bg = _markers(shape, "faces_ball")
    g = _graph(shape, fg, bg, first_relabel_dt=0)
    with pytest.raises(_lib.MedpyHipError):
        g.first_relabel()
    g.set_param("first_relabel_dt", 1)
    g.first_relabel()
    with pytest.raises(_lib.MedpyHipError):  # (the labels of this build are there already)
        g.first_relabel()
    with pytest.raises(_lib.MedpyHipError):
        g.set_param("first_relabel_dt", 3)
    g.close()


WORK = ("global_relabels", "phases", "discharge_tiles", "relabel_tiles")


@pytest.mark.parametrize("shape", [(40, 40, 40), (20, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_whole_solves_in_both_forms(shape):
    from medpy_amd import _lib
    s = _volume(shape)[0]
    ref = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"])
    for radial in (0, 1, 2):
        got = {}
        for form in (1, 2):
            g = _graph(shape, s["fg"], s["bg"], first_relabel_dt=form, radial=radial)
            flow = g.maxflow()
            labels = g.labels().copy()
            _lib.assert_valid(g.validate())
            got[form] = (flow, labels, g.stats(), g.launch_counts())
            g.close()
            assert int((labels != ref.labels).sum()) == 0, (radial, form)
            assert flow == pytest.approx(ref.flow, rel=1e-9), (radial, form)
        assert got[1][3]["k_dt_axis"] > 0 and got[1][3]["k_dt_scan"] == 0, got[1][3]
        assert got[2][3]["k_dt_axis"] == 0 and got[2][3]["k_dt_scan"] > 0, got[2][3]
        assert got[1][0] == got[2][0], (radial, got[1][0], got[2][0])  # bit for bit
        np.testing.assert_array_equal(got[1][1], got[2][1])
        assert [got[1][2][k] for k in WORK] == [got[2][2][k] for k in WORK], (radial, got[1][2], got[2][2])


def test_two_slabs_run_the_axis_kernels_and_give_the_single_handle_labels():
    from medpy_amd.slab import HipSlab, LoopbackExchange, solve_slabs
    shape = (32, 24, 40)
    s = _volume(shape)[0]
    g = _graph(shape, s["fg"], s["bg"])
    g.maxflow()
    single = g.labels().copy()
    g.close()
    slabs = [HipSlab(shape, r, 2) for r in range(2)]
    for sl in slabs:
        z = slice(sl.plane0, sl.plane1)
        sl.set_boundary(s["term"], s["image"][z], s["sigma"])
        sl.set_markers(s["fg"][z], s["bg"][z])
        sl.build()
    st = solve_slabs(slabs, LoopbackExchange(slabs), max_outer=5000)
    assert st["converged"] == 1, st
    counts = [sl.launch_counts() for sl in slabs]
    labels = np.concatenate([sl.finish()[0] for sl in slabs], axis=0)
    for sl in slabs:
        sl.close()
    for c in counts:
        assert c["k_dt_axis"] > 0 and c["k_dt_scan"] > 0, c  # x and y in one launch each, the z scans with their carry planes in two
    np.testing.assert_array_equal(labels, single)
