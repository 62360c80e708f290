"""-m gpu: thin cross-tile flow held back during the early cycles of a solve that floods against walls (MGCW_HOLD_THIN,
mgc_wave_ops.inl).  Every case is solved twice on fresh handles -- hold on (the flood cycle, as shipped)
and hold off (MEDPY_HIP_HOLD_THIN_CYCLES, read when a handle is created) -- and both cuts are held against the BK oracle: labels
voxel for voxel, flow to 1e-9, mgc_validate all zero (pending_outbox and active_excess among the counts), and on == off.
stats()["held_wakeups"] says whether the rule engaged.  A reference cut is computed once per case and shared.

The rule lives in the one-wave-per-tile discharge, which as shipped takes over from 512 active tiles per phase on: volumes of 64^3
(512 tiles) never get there.  So the cases run with wave_min_tiles = 0 (MEDPY_HIP_PARAMS, as the suite sends its small vectors through
the kernel forms of a large volume elsewhere); two more run a mix of both discharge forms."""
import os

import numpy as np
import pytest

from oracle import energy_numpy, pipeline

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = "MEDPY_HIP_HOLD_THIN_CYCLES"
WAVE_FORM = "wave_min_tiles=0"  # every discharge launch goes to k_discharge_w, as on the volumes the rule is meant for
_REF = {}
_RUN = {}


def _two_objects():
    """two bright balls side by side in one 96 x 64 x 64 volume, a seed in each: what leaks out of one while its wall closes runs into the other"""
    from medpy_amd import synthetic
    a, b = synthetic.sphere((48, 64, 64), seed=0), synthetic.sphere((48, 64, 64), seed=1)
    s = {k: np.concatenate([a[k], b[k]], axis=0) for k in ("image", "fg")}
    s["bg"] = synthetic._faces((96, 64, 64))
    s.update(sigma=a["sigma"], term=a["term"])
    return s


def _inputs(case):
    from medpy_amd import synthetic
    if case == "two_objects":
        return _two_objects(), None
    gen, shape, spacing = {"sphere64": ("sphere", (64, 64, 64), None), "sphere96": ("sphere", (96, 96, 96), None),
                           "sphere_partial": ("sphere", (50, 37, 41), None), "sphere64_spacing": ("sphere", (64, 64, 64), (0.5, 1.0, 2.0)),
                           "hard64": ("hard", (64, 64, 64), None), "ct64": ("ct", (64, 64, 64), None)}[case]
    return getattr(synthetic, gen)(shape), spacing


def _reference(case):
    if case not in _REF:
        s, spacing = _inputs(case)
        ref = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"], spacing=spacing or False)
        _REF[case] = (ref.labels.copy(), float(ref.flow))
    return _REF[case]


def _solve(monkeypatch, case, cycles, forms=WAVE_FORM):
    """(labels, flow, stats, validation) of `case` on a fresh handle created under MEDPY_HIP_HOLD_THIN_CYCLES = cycles; solved once per module"""
    if (case, cycles, forms) not in _RUN:
        from medpy_amd import graphcut
        s, spacing = _inputs(case)
        monkeypatch.setenv(ENV, str(cycles))
        monkeypatch.setenv("MEDPY_HIP_PARAMS", forms)
        g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                       boundary_term_args=(s["image"], s["sigma"], spacing or False))
        flow = g.maxflow()
        _RUN[(case, cycles, forms)] = (g.labels().copy(), flow, g.stats(), g.validate())
        g.close()
    return _RUN[(case, cycles, forms)]


def _assert_cut(got, labels_ref, flow_ref):
    from medpy_amd import _lib
    labels, flow, st, v = got
    print("flow %r (reference %r), %d voxels differ, held_wakeups %d, %d tile visits, %d phases, %d global relabels, %d radial cycles" % (
        flow, flow_ref, int((labels != labels_ref).sum()), st["held_wakeups"], st["discharge_tiles"], st["phases"], st["global_relabels"], st["radial_cycles"]))
    np.testing.assert_array_equal(labels, labels_ref)
    assert flow == pytest.approx(flow_ref, rel=1e-9)
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v


def _on_off(monkeypatch, case, forms=WAVE_FORM, cycles=1):
    labels_ref, flow_ref = _reference(case)
    on, off = _solve(monkeypatch, case, cycles, forms), _solve(monkeypatch, case, 0, forms)
    _assert_cut(on, labels_ref, flow_ref)
    _assert_cut(off, labels_ref, flow_ref)
    np.testing.assert_array_equal(on[0], off[0])
    return on, off


@pytest.mark.parametrize("cycles", [1, 2], ids=["flood_cycle", "and_the_cycle_behind_it"])
@pytest.mark.parametrize("case", ["sphere64", "sphere96"])
def test_walls_hold_engages_and_the_cut_is_the_oracles(monkeypatch, case, cycles):
    on, off = _on_off(monkeypatch, case, cycles=cycles)
    assert on[2]["radial_cycles"] > 0 and off[2]["radial_cycles"] > 0  # (the flood ran: the rule's precondition)
    assert on[2]["held_wakeups"] > 0
    assert off[2]["held_wakeups"] == 0


@pytest.mark.parametrize("forms", ["", "wave_min_tiles=64"], ids=["as_shipped", "switch_at_64_tiles"])
def test_both_discharge_forms_mixed(monkeypatch, forms):
    """96^3 with the switch between the two discharge forms as shipped (512 tiles per phase) and at 64 tiles: the long lists go to the wave form,
    the short ones to the workgroup form, which must add to what the wave form left waiting in an outbox, never overwrite it"""
    on, off = _on_off(monkeypatch, "sphere96", forms=forms)
    assert off[2]["held_wakeups"] == 0


@pytest.mark.parametrize("case", ["sphere_partial", "sphere64_spacing", "two_objects"])
def test_partial_tiles_spacing_and_two_objects(monkeypatch, case):
    on, off = _on_off(monkeypatch, case)
    assert off[2]["held_wakeups"] == 0


@pytest.mark.parametrize("case", ["hard64", "ct64"])
def test_no_walls_never_hold(monkeypatch, case):
    """graphs without walls live on thin flows: the flag must stay clear and the schedule be the one of hold off, visit for visit"""
    on, off = _on_off(monkeypatch, case)
    assert on[2]["held_wakeups"] == 0 and off[2]["held_wakeups"] == 0
    for k in ("discharge_tiles", "relabel_tiles", "phases", "global_relabels"):
        assert on[2][k] == off[2][k], k


def test_golden_image_whose_cut_is_not_the_marker_ball(monkeypatch):
    """the reference's own notebook image (1024 x 1024, uint16) and markers, against the labels and the flow the reference gave for them"""
    from medpy_amd import graphcut
    z = np.load(os.path.join(HERE, "golden", "reference_b0.npz"))
    img = z["image"].astype(np.dtype(str(z["image_dtype"])))
    fg, bg = z["markers"] == 1, z["markers"] == 2
    term = "difference_exponential"
    labels_ref = np.unpackbits(z[term + "/labels"])[: img.size].reshape(img.shape).astype(bool)
    got = {}
    monkeypatch.setenv("MEDPY_HIP_PARAMS", WAVE_FORM)
    for cycles in (1, 0):
        monkeypatch.setenv(ENV, str(cycles))
        g = graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                       boundary_term_args=(img, float(z[term + "/sigma"]), False))
        flow = g.maxflow()
        got[cycles] = (g.labels().copy(), flow, g.stats(), g.validate())
        g.close()
        _assert_cut(got[cycles], labels_ref, float(z[term + "/flow"]))
    np.testing.assert_array_equal(got[1][0], got[0][0])
    assert got[0][2]["held_wakeups"] == 0


def test_dense_nlink_weights_never_hold(monkeypatch):
    """the sphere's own weights given as dense arrays: the scale of explicit capacities is unknown, so the rule stays off"""
    from medpy_amd.graphcut import VoxelGraph
    s, _ = _inputs("sphere64")
    labels_ref, flow_ref = _reference("sphere64")
    shape = s["fg"].shape
    got = {}
    monkeypatch.setenv("MEDPY_HIP_PARAMS", WAVE_FORM)
    for cycles in (1, 0):
        monkeypatch.setenv(ENV, str(cycles))
        g = VoxelGraph(shape)
        g._set_markers(s["fg"], s["bg"])
        for axis, w in enumerate(energy_numpy.boundary_weights(s["term"], s["image"], s["sigma"])):
            full = np.zeros(shape)
            full[tuple(slice(0, n - 1) if k == axis else slice(None) for k, n in enumerate(shape))] = w
            g._add_nweights(tuple(1 if k == axis else 0 for k in range(3)), full)
        g._build()
        flow = g.maxflow()
        got[cycles] = (g.labels().copy(), flow, g.stats(), g.validate())
        g.close()
        _assert_cut(got[cycles], labels_ref, flow_ref)
        assert got[cycles][2]["held_wakeups"] == 0
    np.testing.assert_array_equal(got[1][0], got[0][0])
    assert got[1][2]["discharge_tiles"] == got[0][2]["discharge_tiles"]


def test_hold_in_every_cycle_still_converges_to_the_oracle(monkeypatch):
    """MEDPY_HIP_HOLD_THIN_CYCLES = 50: held flow then only moves with the absorb + activation of a global relabel, a tile per relabel --
    the path that delivers it.  On 64^3 that is a handful of relabels more."""
    labels_ref, flow_ref = _reference("sphere64")
    forced, off = _solve(monkeypatch, "sphere64", 50), _solve(monkeypatch, "sphere64", 0)
    _assert_cut(forced, labels_ref, flow_ref)
    np.testing.assert_array_equal(forced[0], off[0])
    assert forced[2]["held_wakeups"] > 0
    assert forced[2]["global_relabels"] >= off[2]["global_relabels"]
