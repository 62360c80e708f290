"""CPU tier: what tests/test_gpu_slab_build.py (-m gpu) stands on, and the Z-slab schedule on border tiles that are partial in y or x.

(1) slab_cases.slab_spec, the plain restatement of the split, against the host simulator's slabs (compiled from the same mgc_common.h
as the library) for every plane count 1 .. 41 and 1 .. 6 slabs, refusals included.
(2) The geometries of slab_cases.GEOMETRIES through the host simulator at both neighbourhoods, weights from oracle/energy_numpy.py: one
linear, one division, one exponential and one power term on the float32 and the int16 image; labels are BK's, the schedule converges,
again with one record slot per border message (every partial border tile is deferred and drained).
(3) Which of those cases have a unique minimum cut (cutcheck.ambiguity): the GPU tier compares those voxel for voxel and the others by
equivalence.  Condition: every geometry keeps a unique case at either neighbourhood.
(4) slab_cases.check_slab_build passes read-backs restated in NumPy (the whole volume as "single", the held planes as "slab"), and
rejects them doctored in each of the ways a slab build could be wrong, by the assertion named for the fault."""
import os
import re
import sys

import numpy as np
import pytest

import face_nb_cases as fn
import full_nb_cases as fc
import slab_cases as sc
from oracle import energy_numpy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))

GEOMETRY_IDS = [sc.geometry_id(g) for g in sc.GEOMETRIES]


# ---- (1) the split ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", sc.CONNS)
def test_slab_spec_is_the_simulators(conn):
    import sim
    cls = sim.SimSlab if conn == 6 else sim.SimSlab26
    refused = 0
    for d0 in range(1, 42):
        for nranks in range(1, 7):
            if nranks > -(-d0 // 8):
                for rank in range(nranks):
                    with pytest.raises(ValueError):
                        sc.slab_spec(d0, rank, nranks)
                    with pytest.raises(AssertionError, match="cannot cut"):
                        cls((d0, 3, 2), rank, nranks)
                refused += 1
                continue
            specs = [sc.slab_spec(d0, r, nranks) for r in range(nranks)]
            for r, want in enumerate(specs):
                s = cls((d0, 3, 2), r, nranks)
                assert sc.spec_of(s) == want, (d0, r, nranks)
                assert s.local_shape == (want["plane1"] - want["plane0"], 3, 2)
                s.close()
            # slab boundaries fall on tile layers, partition the planes, and nobody owns nothing
            assert specs[0]["own0"] == 0 and specs[-1]["own1"] == d0
            assert all(a["own1"] == b["own0"] and a["own1"] % 8 == 0 for a, b in zip(specs, specs[1:]))
            assert all(s["own0"] < s["own1"] and s["plane0"] <= s["own0"] and s["own1"] <= s["plane1"] <= d0 for s in specs)
            assert all(s["own0"] - s["plane0"] == (8 if s["has_lo"] else 0) for s in specs)
            assert all(s["plane1"] - s["own1"] == (min(8, d0 - s["own1"]) if s["has_hi"] else 0) for s in specs)
    assert refused == sum(1 for d0 in range(1, 42) for n in range(1, 7) if n > -(-d0 // 8)) > 0
    for bad in ((16, -1, 2), (16, 2, 2), (16, 0, 0)):
        with pytest.raises(ValueError):
            sc.slab_spec(*bad)


def test_the_geometries_are_what_the_issue_names():
    """a one-plane owned layer and a one-plane ghost layer; ghost layers on both sides; partial tiles in y and x; x inside one tile"""
    assert sc.slab_spec(9, 1, 2) == {"own0": 8, "own1": 9, "plane0": 0, "plane1": 9, "has_lo": True, "has_hi": False}
    assert sc.slab_spec(9, 0, 2) == {"own0": 0, "own1": 8, "plane0": 0, "plane1": 9, "has_lo": False, "has_hi": True}
    assert sc.slab_spec(17, 1, 3) == {"own0": 8, "own1": 16, "plane0": 0, "plane1": 17, "has_lo": True, "has_hi": True}
    assert sc.slab_spec(17, 2, 3)["own1"] - sc.slab_spec(17, 2, 3)["own0"] == 1
    assert [sc.slab_spec(20, r, 2)["own1"] - sc.slab_spec(20, r, 2)["own0"] for r in range(2)] == [8, 12]
    assert sc.slab_spec(20, 0, 2)["plane1"] == 16 and sc.slab_spec(24, 1, 3)["plane0"] == 0 and sc.slab_spec(24, 0, 3)["plane1"] == 16
    partial = [shape for shape, _ in sc.GEOMETRIES if shape[1] % 8 or shape[2] % 8]
    assert len(partial) == 5 and (16, 17, 7) in partial
    sizes = sorted(int(np.prod(shape)) for shape in {g[0] for g in sc.GEOMETRIES})
    assert sorted(int(np.prod(s)) for s in sc.SWEEP_SHAPES) == sizes[:2]
    for shape, nslabs in sc.GEOMETRIES:   # the planted extremes lie in planes that only the first / only the last slab OWNS
        x = sc.inputs(shape)
        for dt in sc.DTYPES:
            img = x[dt]
            assert img[0].min() == img.min() == sc.LOW and img[-1].max() == img.max() == sc.HIGH
            assert img[1:].min() >= 0 and img[:-1].max() < sc.HIGH


def test_the_arc_sets():
    for shape, nslabs in sc.GEOMETRIES:
        for conn in sc.CONNS:
            every, read = sc.every_arc(shape, conn), sc.arcs_to_read(shape, conn)
            idx = np.indices(shape)
            for o, m in read.items():
                assert not (m & ~every[o]).any()
                if shape in sc.SWEEP_SHAPES:
                    assert np.array_equal(m, every[o])
                for a, k in enumerate(o):
                    if k:
                        assert m[every[o] & ((idx[a] + k) // 8 != idx[a] // 8)].all()   # every arc through a tile face (slab borders among them)
                assert m[every[o] & ((idx[0] == 0) | (idx[0] + o[0] == shape[0] - 1))].all()
            for r in range(nslabs):
                spec = sc.slab_spec(shape[0], r, nslabs)
                loc = sc.local_arcs(read, spec)
                n = spec["plane1"] - spec["plane0"]
                for o, m in loc.items():
                    assert m.shape == (n,) + shape[1:] and not (m & ~sc.every_arc(m.shape, conn)[o]).any()


# ---- (2), (3) the schedule on these geometries, and which cuts are unique ----------------------------------------------------------------

def _sim_problem(shape, conn, term, dtype):
    import sim
    case, ref, unique = sc.reference_cut(shape, conn, term, dtype)
    tr = fc.merged_tlinks(case["fg"], case["bg"])
    if conn == 6:
        w = energy_numpy.boundary_weights(term, case["image"], case["sigma"])
        return sim.SimSlab, w, tr, ref, unique
    return sim.SimSlab26, sim.weights26(shape, sc.cut_weights(case)), tr, ref, unique


@pytest.fixture
def wave_mode(request):
    import sim
    sim.set_wave_mode(request.param)
    yield request.param
    sim.set_wave_mode(0)


@pytest.mark.parametrize("conn,wave_mode", [(6, 0), (6, 7), (26, 0), (26, 16)], indirect=["wave_mode"], ids=["6-workgroup", "6-wave", "26-workgroup", "26-wave"])
@pytest.mark.parametrize("geometry", sc.GEOMETRIES, ids=GEOMETRY_IDS)
def test_geometries_through_the_host_simulator(geometry, conn, wave_mode):
    """the schedule, the halo pack / unpack and the label read-out on border tiles that are partial in y or x, on one-plane owned and
    ghost layers and on a slab with two ghost layers: BK's labels, also when every border message holds one record.  In the 512-lane
    workgroup forms of the tile operations and in the one-wave-per-tile forms the library runs by default (sim.set_wave_mode).

    Found here, on 24 x 8 x 8 / 3 and 20 x 11 x 10 / 2 under difference_linear: with border flow exchanged every SECOND colour round
    (exchange_rounds 2, the default) a border tile can be discharged twice before a border message takes what it pushed over the slab
    border, and both forms of the 6-neighbourhood discharge stored the second visit's outbox over the first's: flow vanished, the
    schedule ended "converged" on a cut at the foreground markers."""
    from medpy_amd.slab import LoopbackExchange, solve_slabs
    shape, nslabs = geometry
    for term in sc.CUT_TERMS:
        for dtype in sc.DTYPES:
            cls, w, tr, ref, unique = _sim_problem(shape, conn, term, dtype)
            for halo_max in (None, 1):
                slabs = [cls(shape, r, nslabs) for r in range(nslabs)]
                for r, s in enumerate(slabs):
                    assert sc.spec_of(s) == sc.slab_spec(shape[0], r, nslabs)
                    s.load(w, tr)
                    if halo_max:
                        s.set_halo_max(halo_max)
                st = solve_slabs(slabs, LoopbackExchange(slabs))
                what = "%s %s %s, %d-neighbourhood, halo_max %s" % (sc.geometry_id(geometry), term, dtype, conn, halo_max)
                assert st["converged"] == 1, what
                labels = np.concatenate([s.finish()[0] for s in slabs], axis=0)
                for s in slabs:
                    s.close()
                differing = int((labels != ref.labels).sum())
                assert not differing, "%s: %d labels differ from BK's (unique minimum cut: %s)" % (what, differing, unique)


@pytest.mark.parametrize("conn", sc.CONNS)
def test_every_geometry_keeps_a_unique_minimum_cut(conn):
    for shape in sorted({g[0] for g in sc.GEOMETRIES}):
        facts = {}
        for term in sc.CUT_TERMS:
            for dtype in sc.DTYPES:
                case, ref, unique = sc.reference_cut(shape, conn, term, dtype)
                n, share, amb = fc.cut_facts(case, ref)
                assert unique == (amb == 0.0) or n == 0
                facts[(term, dtype)] = (unique, share)
        print("%s, %d-neighbourhood: unique minimum cut for %s" % (fc.shape_id(shape), conn, sorted(k for k, v in facts.items() if v[0])))
        assert any(u for u, _ in facts.values()), "%s at %d: no case with a unique minimum cut" % (fc.shape_id(shape), conn)
        # ... and one that is cut away from the markers (a cut at a marker plane comes out right if no flow crosses a slab border)
        assert any(u and 0.10 <= share <= 0.90 for u, share in facts.values()), "%s at %d: %r" % (fc.shape_id(shape), conn, facts)


# ---- (4) the comparison ------------------------------------------------------------------------------------------------------------------

def _tr(shape, term=None):
    x = sc.inputs(shape)
    if term is None:
        return fc.merged_tlinks(x["fg"], x["bg"])
    prob, alpha = sc.regional(shape, term)
    return fc.merged_tlinks(x["fg"], x["bg"], prob, alpha)


def _whole(shape, conn, term="difference_division", dtype="float32", spacing_on=False, regional=False):
    image = sc.inputs(shape)[dtype]
    return sc.HostHandle(term, image, fc.spacing_of(shape, spacing_on), conn, _tr(shape, term if regional else None))


def _check(whole, slab, spec, conn, arcs, prepush=False):
    return sc.check_slab_build(slab.reads(sc.local_arcs(arcs, spec)), whole.reads(arcs), spec, conn, prepush)


@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("geometry", sc.GEOMETRIES, ids=GEOMETRY_IDS)
def test_the_restated_slab_passes(geometry, conn):
    shape, nslabs = geometry
    arcs = sc.arcs_to_read(shape, conn)
    for term, dtype, spacing_on in (("difference_linear", "float32", True), ("maximum_power", "int16", False)):
        whole = _whole(shape, conn, term, dtype, spacing_on)
        single = whole.reads(arcs)
        for r in range(nslabs):
            spec = sc.slab_spec(shape[0], r, nslabs)
            n = sc.check_slab_build(whole.slab(spec).reads(sc.local_arcs(arcs, spec)), single, spec, conn)
            assert n > 0
    if conn == 6:   # with the model of a pre-push: the stored arcs are no longer the weights, and still the single handle's
        whole = _whole(shape, 6, "difference_division", "float32", regional=True).prepush()
        single = whole.reads(arcs)
        changed = sum(int((sc.bits(whole.rcap[o]) != sc.bits(whole.w[o])).sum()) for o in sc.offsets(6))
        assert changed > 0
        for r in range(nslabs):
            spec = sc.slab_spec(shape[0], r, nslabs)
            sc.check_slab_build(whole.slab(spec).reads(sc.local_arcs(arcs, spec)), single, spec, 6, prepush=True)


def _rejected(name, whole, slab, spec, conn, arcs, prepush=False):
    with pytest.raises(AssertionError, match=re.escape(name)):
        _check(whole, slab, spec, conn, arcs, prepush)


@pytest.mark.parametrize("conn", sc.CONNS)
def test_local_planes_shifted_by_one_plane(conn):
    """the slab built from planes [plane0 + 1, plane1 + 1), where the volume has them, or read back one plane off"""
    shape, nslabs = (24, 8, 8), 3
    arcs = sc.arcs_to_read(shape, conn)
    whole = _whole(shape, conn)
    built_off = 0
    for r in range(nslabs):
        spec = sc.slab_spec(shape[0], r, nslabs)
        shift = 1 if spec["plane1"] < shape[0] else (-1 if spec["plane0"] > 0 else 0)
        if shift:
            off = dict(spec, plane0=spec["plane0"] + shift, plane1=spec["plane1"] + shift, own0=spec["own0"] + shift, own1=spec["own1"] + shift)
            _rejected(sc.NW_NOT_SINGLE, whole, whole.slab(off), spec, conn, arcs)
            built_off += 1
        slab = whole.slab(spec)   # the image, hence the weights, one plane off
        for o in slab.w:
            slab.w[o] = np.roll(slab.w[o], 1, axis=0)
        _rejected(sc.NW_NOT_SINGLE, whole, slab, spec, conn, arcs)
        slab = whole.slab(spec)   # the weights right, what was stored one plane off
        for o in slab.rcap:
            slab.rcap[o] = np.roll(slab.rcap[o], 1, axis=0)
        _rejected(sc.EDGE_NOT_SINGLE, whole, slab, spec, conn, arcs)
    assert built_off == 2   # (the middle slab holds every plane of the volume)


@pytest.mark.parametrize("term", ["difference_linear", "maximum_linear"])
@pytest.mark.parametrize("conn", sc.CONNS)
def test_linear_term_normalised_by_the_slabs_own_range(conn, term):
    shape, nslabs = (24, 8, 8), 3
    arcs = sc.arcs_to_read(shape, conn)
    for dtype in sc.DTYPES:
        whole = _whole(shape, conn, term, dtype)
        full = sc.inputs(shape)[dtype].astype(np.float64)
        scale = (lambda a: np.abs(a).max()) if term.startswith("maximum") else (lambda a: a.max() - a.min())   # what the term divides by
        rejected = 0
        for r in range(nslabs):
            spec = sc.slab_spec(shape[0], r, nslabs)
            image = sc.inputs(shape)[dtype][spec["plane0"]:spec["plane1"]]
            if scale(image.astype(np.float64)) == scale(full):
                continue   # (the middle slab holds every plane; max |I| is HIGH, which the last slab holds)
            local = sc.HostHandle(term, image, False, conn, whole.tr[spec["plane0"]:spec["plane1"]])   # the range of the held planes
            if conn == 26:
                local.rcap = whole.slab(spec).rcap
            _rejected(sc.NW_NOT_SINGLE, whole, local, spec, conn, arcs)
            rejected += 1
        assert rejected == (1 if term.startswith("maximum") else 2)


@pytest.mark.parametrize("conn", sc.CONNS)
@pytest.mark.parametrize("geometry", [((9, 9, 17), 2), ((17, 13, 9), 3)], ids=sc.geometry_id)
def test_arcs_into_the_ghost_plane_zeroed(geometry, conn):
    shape, nslabs = geometry
    arcs = sc.arcs_to_read(shape, conn)
    whole = _whole(shape, conn, "difference_power", "int16")
    for r in range(nslabs):
        spec = sc.slab_spec(shape[0], r, nslabs)
        for up in (1, -1):
            if not spec["has_hi" if up > 0 else "has_lo"]:
                continue
            slab = whole.slab(spec)
            last = (spec["own1"] - 1 if up > 0 else spec["own0"]) - spec["plane0"]
            for o in slab.rcap:
                if o[0] == up:
                    slab.rcap[o][last] = 0.0
            _rejected(sc.EDGE_NOT_SINGLE, whole, slab, spec, conn, arcs)
    # ... and the other way round: a ghost layer whose stored arcs were NOT cleared (26), or not built (6)
    spec = sc.slab_spec(shape[0], 0, nslabs)
    slab = whole.slab(spec)
    g = spec["own1"] - spec["plane0"]
    for o in slab.rcap:
        slab.rcap[o][g:] = slab.w[o][g:] if conn == 26 else 0.0
    _rejected(sc.GHOST_EDGE, whole, slab, spec, conn, arcs)


def test_a_back_arc_swapped_with_its_forward_arc():
    """weights are symmetric, so this shows only on residuals that a pre-push moved: the model of fn.model_prepush"""
    shape, nslabs = (17, 13, 9), 2
    arcs = sc.every_arc(shape, 6)
    whole = _whole(shape, 6, "difference_division", "float32", regional=True).prepush()
    for r in range(nslabs):
        spec = sc.slab_spec(shape[0], r, nslabs)
        slab = whole.slab(spec)
        owned = np.zeros(slab.shape, bool)
        owned[spec["own0"] - spec["plane0"]:spec["own1"] - spec["plane0"]] = True
        swapped = 0
        for o in sc.offsets(6):
            src, dst = fc._slices(slab.shape, o)
            f, b = slab.rcap[o][src], slab.rcap[fc.negated(o)][dst]
            pick = np.flatnonzero(((sc.bits(f) != sc.bits(b)).reshape(f.shape) & owned[src] & owned[dst]).ravel())[:1]
            for k in pick:
                p = np.unravel_index(k, f.shape)
                f[p], b[p] = b[p], f[p]
                swapped += 1
        assert swapped
        _rejected(sc.EDGE_NOT_SINGLE, whole, slab, spec, 6, arcs, prepush=True)


@pytest.mark.parametrize("conn", sc.CONNS)
def test_tlinks_of_the_ghost_plane_leak_into_the_owned_planes(conn):
    shape, nslabs = (9, 9, 17), 2
    arcs = sc.arcs_to_read(shape, conn)
    whole = _whole(shape, conn, "difference_exponential", "float32", regional=True)
    spec = sc.slab_spec(shape[0], 0, nslabs)   # owns planes 0 .. 7, plane 8 is its ghost layer
    slab = whole.slab(spec)
    slab.tr[7] = slab.tr[8]
    _rejected(sc.TW_NOT_SINGLE, whole, slab, spec, conn, arcs)
    slab = whole.slab(spec)
    slab.tr[8] = slab.tr[7]   # ... and the reverse
    _rejected(sc.GHOST_TW, whole, slab, spec, conn, arcs)
    slab = whole.slab(spec)   # an arc out of the held planes that is not "outside"
    spec1 = sc.slab_spec(17, 0, 3)
    whole1 = _whole((17, 13, 9), conn)
    slab1 = whole1.slab(spec1)
    up = (1, 0, 0)
    slab1.w[up][-1] = whole1.w[up][spec1["plane1"] - 1]
    _rejected(sc.GHOST_NW, whole1, slab1, spec1, conn, sc.arcs_to_read((17, 13, 9), conn))
