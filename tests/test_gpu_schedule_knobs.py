"""-m gpu: every knob mgc_set_param accepts, at the edges of its range, against the BK oracle.

The contract under test: a value is either refused (MedpyHipError) or gives the oracle's cut -- labels voxel for voxel (the
equivalence checker on the tie-heavy volume), flow within 1e-9, a maximum preflow that mgc_validate finds sound, and no
ERR_NOT_CONVERGED within a finite max_outer.  Each value runs on a fresh handle, once on top of the shipped defaults and once on top
of the thresholds at zero (conftest.LARGE_VOLUME_FORMS, set here through set_param: the kernel forms a large volume uses).  The grid
knobs get cases of their own, on the thresholds at zero with the kernel form that reads the grid (the solve must have launched that
kernel: mgc_get_launch_counts), that force every grid-stride and ticket loop round many times; the Z-slab schedule knobs run on slab
handles time-multiplexed on the device.  tests/test_schedule_knobs_hostsim.py::test_every_set_param_knob_is_in_the_gpu_table (CPU) keeps
the table in step with mgc_set_param."""
import numpy as np
import pytest

from oracle import cutcheck, energy_numpy, pipeline

pytestmark = pytest.mark.gpu

MAX_OUTER = 5000  # a schedule that does not converge fails with ERR_NOT_CONVERGED instead of spinning for minutes

# name -> (test values, neighbourhoods the knob acts in, knobs set along with it: the kernel form it belongs to, {neighbourhood: the
# kernel that form runs}: the solve must have launched it, mgc_get_launch_counts -- a form switched off by another bit fails)
N6, N26, BOTH = (6,), (26,), (6, 26)
KNOBS = {
    "rounds_per_relabel": ((1, 3, 7, 64), BOTH, {}, {}),
    "max_cycles": ((-1, 1, 3), BOTH, {}, {}),
    "max_sweeps": ((1, 3, 5), BOTH, {}, {}),
    "max_outer": ((200, MAX_OUTER), BOTH, {}, {}),
    "relabel_batch": ((1, 3), BOTH, {}, {}),
    "check_rounds": ((1, 3, 5), BOTH, {}, {}),
    "stop_below": ((1, 10 ** 6), BOTH, {}, {}),
    "incremental_relabel": ((0,), BOTH, {}, {}),
    "trace": ((1,), N6, {}, {}),
    "adaptive_rounds": ((0, 1, 100), BOTH, {}, {}),
    "radial": ((0, 1, 2), BOTH, {}, {}),
    "radial_min_walls": ((0, 10 ** 6), N6, {}, {}),
    "radial_budget_x16": ((1, 64), BOTH, {"radial": 1}, {}),
    "radial_min_c": ((1,), BOTH, {"radial": 1}, {}),
    "radial_rounds0": ((1, 2), BOTH, {"radial": 1}, {}),
    "use_filters": (tuple(range(8)), BOTH, {}, {}),
    "wave_kernels": ((0, 1, 2, 4, 8, 16, 32), BOTH, {}, {}),
    "wave_min_tiles": ((0,), N6, {}, {}),
    "sweeps_sparse26": ((0, 1), N26, {}, {}),
    "prepush": ((0, 1), BOTH, {}, {}),
    "exchange_passes": ((1, 3), N6, {}, {}),  # (single handle: no effect; the slab cases below)
    "relabel_exchange_every": ((3,), N6, {}, {}),
    "exchange_rounds": ((3, 5), N6, {}, {}),
    "w26_passes": ((1, 3), N26, {"wave_kernels": 41, "max_cycles": -1}, {26: "k26_discharge_w"}),
    "w26_raises": ((1, 3), N26, {"wave_kernels": 41, "max_cycles": -1}, {26: "k26_discharge_w"}),
    "w26_flags": ((1, 2, 3), N26, {"wave_kernels": 41, "max_cycles": -1}, {26: "k26_discharge_w"}),
    "first_relabel_dt": ((0,), N6, {}, {}),
    "relabel_bricks": ((1,), N6, {}, {}),
    "exact_sink_tiles": ((0, 1, 2), N6, {}, {}),
    "sink_sweeps": ((1, 3), N6, {"exact_sink_tiles": 1}, {}),
    "halo_max_records": ((1, 3), N6, {}, {}),  # (single handle: no effect; the slab cases below)
    "wave_stagger": ((1,), N6, {}, {}),
    "repeat_steps": (tuple(range(8)), N6, {}, {}),
    "repeat_min_tiles": ((0,), N6, {"repeat_steps": 3}, {}),
    "repeat_flood_min_tiles": ((0,), N6, {"repeat_steps": 7}, {}),
    "list_shards": ((1,), BOTH, {}, {}),
    "activate_exact_max": ((0,), N6, {}, {}),
    "kernel_timing": ((1,), BOTH, {}, {}),
    "timing_stride": ((1,), BOTH, {"kernel_timing": 1}, {}),
    "profile_sections": ((1,), BOTH, {}, {}),
}
# the grids, at or below the shipped ones (a grid above them is not co-resident): every grid-stride / ticket loop goes round many times
# with a ragged remainder.  On the thresholds-at-zero base, with the form that reads the grid switched on (wave_kernels: bit 0 the wave
# discharge, 1 the wave relabel unless bit 3 takes the relabels, 4 / 5 the 26-neighbourhood forms that take the discharge from k26_discharge)
GRID_KNOBS = {
    "grid_cap": ((1, 3, 64), BOTH, {}, {6: "k_relabel_v", 26: "k26_discharge_v"}),
    "grid26_dis": ((0, 1, 7), N26, {"wave_kernels": 9}, {26: "k26_discharge"}),
    "wave_grid_dis": ((1, 3), N6, {}, {6: "k_discharge_w"}),
    "wave_grid_rel": ((1, 3), N6, {"wave_kernels": 3}, {6: "k_relabel_w"}),
    "wave_grid26": ((1, 3), N26, {"wave_kernels": 41, "max_cycles": -1}, {26: "k26_discharge_w"}),
}
EXCLUDED = {}  # name -> why it has no row above (nothing so far)
# values out of range: mgc_set_param must refuse them
REFUSED = {
    "rounds_per_relabel": (0, -1), "max_cycles": (0,), "max_sweeps": (0, -1), "max_outer": (0, -1), "grid_cap": (0, -1), "grid26_dis": (-1,),
    "relabel_batch": (0, -1), "check_rounds": (0, -1), "stop_below": (-1,), "adaptive_rounds": (-1,), "radial": (3, -1),
    "radial_min_walls": (-1,), "radial_budget_x16": (0,), "radial_min_c": (0,), "radial_rounds0": (-1,), "use_filters": (8, -1),
    "wave_kernels": (64, -1), "wave_min_tiles": (-1,), "sweeps_sparse26": (-1,), "wave_grid_dis": (0, -1), "wave_grid26": (0,),
    "exchange_passes": (0,), "relabel_exchange_every": (0,), "exchange_rounds": (0, -1), "w26_passes": (0,), "w26_raises": (0,),
    "w26_flags": (-1,), "wave_grid_rel": (0,), "exact_sink_tiles": (3, -1), "sink_sweeps": (0,), "halo_max_records": (0,),
    "wave_stagger": (-1,), "repeat_steps": (8, -1), "repeat_min_tiles": (-1,), "repeat_flood_min_tiles": (-1,), "list_shards": (2, 0),
    "activate_exact_max": (-1,), "timing_stride": (0,), "no_such_knob": (1,),
}


def _thresholds_at_zero():
    from conftest import LARGE_VOLUME_FORMS
    return [(k, int(v)) for k, v in (kv.split("=") for kv in LARGE_VOLUME_FORMS.split(","))]


BASES = {"shipped": lambda: [], "thresholds_at_zero": _thresholds_at_zero}

VOLUMES = {  # name -> (generator, shape, connectivity, regional term)
    "sphere40": ("sphere", (40, 40, 40), 6, False),
    "sphere20x33x47": ("sphere", (20, 33, 47), 6, False),
    "hard48": ("hard", (48, 48, 48), 6, False),
    "ties32": ("ties", (32, 32, 32), 6, False),
    "sphere32_n26": ("sphere", (32, 32, 32), 26, False),
    "sphere32_n26_regional": ("sphere", (32, 32, 32), 26, True),
    "sphere40_n26": ("sphere", (40, 40, 40), 26, False),
    "hard48_n26": ("hard", (48, 48, 48), 26, False),
}
KNOB_VOLUMES = {6: ("sphere40", "sphere20x33x47", "hard48", "ties32"), 26: ("sphere32_n26", "sphere32_n26_regional")}
GRID_VOLUMES = {6: ("sphere40", "hard48"), 26: ("sphere40_n26", "hard48_n26")}
_REF = {}


def _volume(name):
    """(synthetic volume, regional (prob, alpha) or None, BK cut): the oracle once per volume and module"""
    if name not in _REF:
        from medpy_amd import synthetic
        gen, shape, conn, regional = VOLUMES[name]
        s = getattr(synthetic, gen)(shape)
        r = synthetic.regional(shape) if regional else None
        kw = dict(prob=r["prob"], alpha=r["alpha"]) if r else {}
        ref = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"],
                                      connectivity=conn if conn != 6 else None, **kw)
        _REF[name] = (s, (r["prob"], r["alpha"]) if r else None, ref)
    return _REF[name]


def _exact(name):
    """the lattice edges and t-links of a tie-heavy volume for the equivalence checker (as test_gpu_parity.py does)"""
    key = name + "/exact"
    if key not in _REF:
        s = _volume(name)[0]
        i, j, ww = cutcheck.lattice_edges(s["image"].shape, energy_numpy.boundary_weights(s["term"], s["image"], s["sigma"]))
        tr = np.where(s["fg"], 65535.0, 0.0) - np.where(s["bg"], 65535.0, 0.0)
        _REF[key] = (i, j, ww, ww, tr)
    return _REF[key]


def _check_cut(name, base, knob, monkeypatch):
    """a fresh handle on volume ``name``: ``knob`` [(name, value), ...] (the knob under test, last, and what goes with it) set at handle
    creation, so that what acts at build time sees it; then max_outer, ``base`` and ``knob`` again through set_param, in that order.
    Solved and compared with the oracle."""
    from medpy_amd import _lib, graphcut
    s, regional, ref = _volume(name)
    conn = VOLUMES[name][2]
    monkeypatch.setenv("MEDPY_HIP_PARAMS", ",".join("%s=%d" % kv for kv in knob))
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    if regional is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=regional)
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], connectivity=conn, **kw)
    monkeypatch.delenv("MEDPY_HIP_PARAMS")
    g.set_param("max_outer", MAX_OUTER)
    for k, v in list(base) + list(knob):
        g.set_param(k, v)
    flow = g.maxflow()  # (raises on ERR_NOT_CONVERGED)
    labels = g.labels()
    what = "%s %s + %s" % (name, base, knob)
    if VOLUMES[name][0] == "ties":  # exact ties between minimum cuts: equivalent, not identical (oracle/cutcheck.py)
        cutcheck.assert_labels_equivalent(labels, ref, exact=_exact(name))
    else:
        bad = int((labels != ref.labels).sum())
        assert bad == 0, "%s: %d voxels differ from BK" % (what, bad)
    assert flow == pytest.approx(ref.flow, rel=1e-9), what
    _lib.assert_valid(g.validate())
    launches = g.launch_counts()
    g.close()
    return launches


def _cases(table):
    out = []
    for knob, (values, scope, along, expect) in table.items():
        for v in values:
            out.append(pytest.param(knob, v, scope, along, expect, id="%s=%d" % (knob, v)))
    return out


def _assert_launched(expect, conn, launches, what):
    if conn in expect:
        assert launches[expect[conn]] > 0, "%s: %s never ran (launches %s)" % (what, expect[conn], launches)


@pytest.mark.parametrize("knob,value,scope,along,expect", _cases(KNOBS))
def test_knob_value_gives_the_oracle_cut(knob, value, scope, along, expect, monkeypatch):
    for base in BASES.values():
        for conn in scope:
            for name in KNOB_VOLUMES[conn]:
                launches = _check_cut(name, base(), sorted(along.items()) + [(knob, value)], monkeypatch)
                _assert_launched(expect, conn, launches, name)


@pytest.mark.parametrize("knob,value,scope,along,expect", _cases(GRID_KNOBS))
def test_small_grids_give_the_oracle_cut(knob, value, scope, along, expect, monkeypatch):
    for conn in scope:
        for name in GRID_VOLUMES[conn]:
            launches = _check_cut(name, _thresholds_at_zero(), sorted(along.items()) + [(knob, value)], monkeypatch)
            _assert_launched(expect, conn, launches, name)


def test_out_of_range_values_are_refused():
    from medpy_amd import _lib, graphcut, synthetic
    s = synthetic.sphere((16, 16, 16))
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                   boundary_term_args=(s["image"], s["sigma"], False))
    for knob, values in REFUSED.items():
        for v in values:
            with pytest.raises(_lib.MedpyHipError):
                g.set_param(knob, v)
    g.close()


@pytest.mark.parametrize("shape,seed,nslabs", [((64, 48, 40), 0, 2), ((64, 48, 40), 0, 3), ((32, 16, 24), 1, 4)],
                         ids=["sphere64x48x40-2slabs", "sphere64x48x40-3slabs", "sphere32x16x24s1-4slabs"])
@pytest.mark.parametrize("schedule", [dict(exchange_rounds=xr, check_rounds=cr) for xr in (3, 5) for cr in (3, 8)] + [dict(stop_below=10 ** 6)],
                         ids=lambda d: "-".join("%s%d" % kv for kv in d.items()))
def test_slab_schedule_knobs_give_the_single_handle_cut(shape, seed, nslabs, schedule):
    """the Z-slab schedule with exchange_rounds that do not divide check_rounds, and with the colour rounds ending at the first look:
    HipSlab handles time-multiplexed on the device, labels = the single handle's = BK's, and no border flow left in an outbox.  64 rounds
    per relabel, so that the look after every check_rounds-th round (only before the cycle's last round) can end a cycle early; the
    (32,16,24) volume is the one where the simulator lost the border flow."""
    from medpy_amd import _lib, graphcut, synthetic
    from medpy_amd.slab import HipSlab, LoopbackExchange, solve_slabs, validate_slabs
    key = "slab_sphere%s_%d" % (shape, seed)
    if key not in _REF:
        s = synthetic.sphere(shape, seed=seed)
        ref = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"])
        g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                       boundary_term_args=(s["image"], s["sigma"], False))
        g.maxflow()
        _REF[key] = (s, ref, g.labels())
        g.close()
    s, ref, single = _REF[key]
    slabs = [HipSlab(shape, r, nslabs) for r in range(nslabs)]
    for sl in slabs:
        z = slice(sl.plane0, sl.plane1)
        sl.set_boundary(s["term"], s["image"][z], s["sigma"])
        sl.set_markers(s["fg"][z], s["bg"][z])
        sl.build()
    ex = LoopbackExchange(slabs)
    st = solve_slabs(slabs, ex, max_outer=MAX_OUTER, rounds_per_relabel=64, **schedule)
    assert st["converged"] == 1, st
    parts = [sl.finish() for sl in slabs]
    labels = np.concatenate([p[0] for p in parts], axis=0)
    flow = sum(p[1] for p in parts)
    v = validate_slabs(slabs, ex)
    for sl in slabs:
        sl.close()
    assert v["voxels"] == int(np.prod(shape)) and v["pending_outbox"] == 0, v
    _lib.assert_valid(v)
    np.testing.assert_array_equal(labels, single)
    np.testing.assert_array_equal(labels, ref.labels)
    assert flow == pytest.approx(ref.flow, rel=1e-9)
