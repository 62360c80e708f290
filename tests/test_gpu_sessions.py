"""-m gpu: one handle driven through a session that mixes every warm edit -- update_markers / edit_markers, update_regional_term,
update_boundary_term, edit_nweights / clear_nweight_edits, update_tweights_dense / edit_tweights, update_tweights_binned /
refit_regional_histogram / iterate_regional_histogram -- against the host model of tests/session_model.py and the BK oracle.

The sessions are those tests/test_session_model_host.py checks on the CPU (the same generators, the same committed seeds).  After
every step that changes the handle its read-backs equal the model's bit for bit: tweights(), nweights_offset() of every offset in
both directions, markers(), the counters of the three info calls the model can know; the residuals of edited arc pairs add up to
the pair's new capacities.  After every solve: families A and B (exact arithmetic) -- flow, labels, source_side(), ambiguous(),
cut_is_unique() equal BK's and cutcheck.ambiguity(tol=0.0), source_cut is the flow, both conservation errors of validate() are 0.0;
family C (floating point, unique cuts) -- labels voxel for voxel, the flow to rel 1e-9, the errors to 1e-9.  changed_labels() is
flatnonzero(labels != snapshot) where the model holds a snapshot and ERR_STATE where it holds none, labels(out=) brings a copy of
the snapshot up to date, and the cut-set calls change none of it.  A refused call leaves every read-back as it was.  At the end
the same handle is rebuilt cold, and a fresh handle is built from the model's final arrays: the same flow and labels.

update_boundary_term on a handle that holds its capacities is refused with ERR_UNSUPPORTED, as include/medpy_hip.h documents
and tests/test_gpu_nweight_edit.py asserts."""
import numpy as np
import pytest

import session_model as sm

pytestmark = pytest.mark.gpu

FORMS = ["as_shipped", "large_volume_forms"]
A_CASES = [(shape, conn, seed) for shape, conn in sm.FAMILY_A for seed in sm.seeds("A", shape)]
B_CASES = [(shape, conn, seed) for shape, conn in sm.FAMILY_B for seed in sm.seeds("B", shape)]
C_CASES = [(shape, conn, kind, seed) for shape, conn, kind in sm.FAMILY_C for seed in sm.seeds("C", shape)]


def _id(case):
    return "%s_seed%d" % (sm.case_id(case[0], case[1]), case[-1])


# ---- handles --------------------------------------------------------------------------------------------------------------------------
def _boundary_arrays(graph, nw):
    for o, (there, back) in nw.items():
        graph.set_nweights_dense(o, there, back)


def _regional(graph, args):
    from medpy_amd.graphcut import energy_voxel
    store, prob, hist = args
    if store is not None:
        energy_voxel.regional_precomputed(graph, store)
    if hist is not None:
        energy_voxel.regional_histogram(graph, hist)
    if prob is not None:
        energy_voxel.regional_probability_map(graph, prob)


def _open(model, from_arrays=False):
    """a handle of the model's inputs through graph_from_voxels: as the session starts (the built-in term, the histogram term fitted
    on the device), or ``from_arrays``: of what the model holds now -- capacities() as dense arrays, the store as the one dense
    call that leaves it"""
    from medpy_amd import graphcut
    from medpy_amd.graphcut import energy_voxel
    full = model.conn not in (None, 2 * len(model.shape))
    store = hist = None
    if model.tr is not None and (from_arrays or model.hist is None):
        tr, share = model.tr.reshape(model.shape), model.share.reshape(model.shape)
        store = (np.maximum(tr, 0.0) + share, np.maximum(-tr, 0.0) + share)
    elif model.hist is not None:
        hist = (model.feature, model.hist["bins"], model.hist["lam"], model.hist["eps"])
    if model.boundary is not None and not from_arrays:
        boundary, args = energy_voxel.boundary_difference_division, (model.boundary["image"], model.boundary["sigma"], False)
    elif full:
        boundary, args = _boundary_arrays, model.capacities()
    else:
        caps = model.capacities()
        boundary, args = energy_voxel.boundary_precomputed, ([caps[o] for o in model.offsets],)
    g = graphcut.graph_from_voxels(model.fg, model.bg, regional_term=_regional, regional_term_args=(store, model.prob, hist),
                                   boundary_term=boundary, boundary_term_args=args, connectivity=model.conn)
    if model.feature is not None and hist is None:
        g._set_feature_image(model.feature)   # (what update_tweights_binned takes its bins of: no public call hands it over alone)
    return g


# ---- what is asserted -------------------------------------------------------------------------------------------------------------------
def _changed(g):
    from medpy_amd import _lib
    try:
        return g.changed_labels().tolist()
    except _lib.MedpyHipError as e:
        return e.code


def _readbacks(g, model):
    out = {"tweights": g.tweights(), "markers": g.markers(), "tw": g.tweight_edit_info(), "nw": g.nweight_edit_info(), "bu": g.boundary_update_info()}
    for o in model.offsets:
        out[o], out[sm.neg(o)] = g.nweights_offset(o), g.nweights_offset(sm.neg(o))
    return out


def _same_readbacks(a, b):
    for key in a:
        if key == "markers":
            assert np.array_equal(a[key][0], b[key][0]) and np.array_equal(a[key][1], b[key][1])
        elif isinstance(a[key], dict):
            assert a[key] == b[key], key
        else:
            assert np.array_equal(sm.bits(a[key]), sm.bits(b[key])), key


def _assert_state(g, model, what):
    """every read-back of the handle against the model, bit for bit"""
    got = _readbacks(g, model)
    assert np.array_equal(sm.bits(got["tweights"]), sm.bits(model.merged()[0])), "%s: tweights()" % (what,)
    caps = model.capacities()
    for o in model.offsets:
        for off in (o, sm.neg(o)):
            want = model.nweights_offset(off, caps)
            assert np.array_equal(np.isnan(got[off]), np.isnan(want)), "%s: nweights_offset(%r): where the neighbour is outside" % (what, off)
            assert np.array_equal(sm.bits(np.nan_to_num(got[off])), sm.bits(np.nan_to_num(want))), "%s: nweights_offset(%r)" % (what, off)
    assert np.array_equal(got["markers"][0], model.fg) and np.array_equal(got["markers"][1], model.bg), "%s: markers()" % (what,)
    assert got["tw"] == model.tweight_info(), (what, got["tw"], model.tweight_info())
    assert (got["nw"]["pairs_kept"], got["nw"]["pairs_changed"]) == (len(model.overrides), model.pairs_changed), (what, got["nw"], len(model.overrides), model.pairs_changed)
    return got


def _assert_solve(g, model, what):
    from medpy_amd import _lib
    exact = model.exact_k is not None
    flow_ref, labels_ref, fs_ref, amb_ref = model.solve()
    flow = g.maxflow()
    labels = g.labels().copy()
    v = g.validate()
    print("%-26s flow %r (BK %r) %d differ, ambiguous %d, pair error %g node error %g, snapshot %s" % (
        what, flow, flow_ref, int((labels != labels_ref).sum()), int(amb_ref.sum()), v["max_pair_error"], v["max_node_error"], model.snapshot is not None))
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), (what, v)
    if exact:
        assert flow == flow_ref, what
        assert v["max_pair_error"] == 0.0 and v["max_node_error"] == 0.0, (what, v)
    else:
        assert flow == pytest.approx(flow_ref, rel=1e-9, abs=1e-300), what
        assert v["max_pair_error"] <= 1e-9 and v["max_node_error"] <= 1e-9, (what, v)
    assert np.array_equal(labels, labels_ref), what
    # the snapshot, before and after the cut-set calls
    if model.snapshot is not None:
        want = np.flatnonzero((labels_ref != model.snapshot).ravel()).tolist()
    else:
        want = _lib.ERR_STATE
    assert _changed(g) == want, what
    g.__dict__["_cut_sets_cache"] = {}   # (a fresh call, not a cached answer)
    fs, amb, info = g.source_side(), g.ambiguous(), g.cut_sets_info()
    if exact:
        assert np.array_equal(fs, fs_ref) and np.array_equal(amb, amb_ref), what
        assert g.cut_is_unique() == (not amb_ref.any()) and info["source_cut"] == flow, (what, info)
        assert (info["from_source"], info["to_sink"], info["ambiguous"]) == (int(fs_ref.sum()), int((~labels_ref).sum()), int(amb_ref.sum())), (what, info)
    else:
        assert not (fs & ~labels).any() and not (amb & fs).any() and not (amb & ~labels).any(), what
        assert info["source_cut"] == pytest.approx(flow, rel=1e-9), what
    assert _changed(g) == want, "%s: after the cut-set calls" % (what,)
    assert g.maxflow() == flow and np.array_equal(g.labels(), labels), "%s: after the cut-set calls" % (what,)
    v2 = g.validate()
    if exact:
        assert v2 == v, "%s: validate() after the cut-set calls" % (what,)
    else:   # (floating point: validate() adds its two totals up with atomics, the last bit moves from call to call)
        assert all(v2[k] == v[k] if k in _lib.VIOLATION_KEYS else v2[k] == pytest.approx(v[k], rel=1e-12, abs=1e-12) for k in v), (what, v, v2)
    if model.snapshot is not None:
        previous = model.snapshot.copy()
        assert g.labels(out=previous) is previous and np.array_equal(previous, labels_ref), "%s: labels(out=)" % (what,)
    else:
        full = np.zeros(model.shape, np.uint8)
        g.labels(out=full)      # no snapshot: the whole volume is read
        assert np.array_equal(full.astype(bool), labels_ref), "%s: labels(out=) without a snapshot" % (what,)
    return flow


def _call(g, model, op, kw):
    """one step of the script on the handle"""
    from medpy_amd.graphcut import energy_voxel
    if op == "edit_nweights":
        return g.edit_nweights(kw["i"], kw["j"], kw["cap"], kw["rev"])
    if op == "edit_tweights":
        return g.edit_tweights(kw["ids"], kw["source"], kw["sink"])
    if op == "update_tweights_dense":
        return g.update_tweights_dense(kw["source"], kw["sink"])
    if op == "update_regional_term":
        return g.update_regional_term(kw["prob"], kw["alpha"])
    if op == "update_boundary_term":
        sigma = model.boundary["sigma"] if kw["sigma"] is None else kw["sigma"]
        return g.update_boundary_term(energy_voxel.boundary_difference_division, (kw["image"], sigma, False))
    if op == "update_markers":
        return g.update_markers(kw["fg"], kw["bg"])
    if op == "build":
        return g._build()
    if op == "refit":
        return g.refit_regional_histogram()
    return getattr(g, op)(**kw)     # edit_markers, update_tweights_binned, clear_nweight_edits


def _play(model, steps, forms, monkeypatch):
    from conftest import LARGE_VOLUME_FORMS
    from medpy_amd import _lib
    if forms == "large_volume_forms":
        monkeypatch.setenv("MEDPY_HIP_PARAMS", LARGE_VOLUME_FORMS)
    exact = model.exact_k is not None
    g = _open(model)
    _assert_state(g, model, "as built")
    remembered = None
    for number, (op, kw) in enumerate(steps):
        what = "%d %s" % (number, op)
        if op == "maxflow":
            _assert_solve(g, model, what)
        elif op == "refused":
            what += " " + kw["op"] + ": " + kw["reason"]
            before, changed = _readbacks(g, model), _changed(g)
            kind, code = kw["error"]
            with pytest.raises(ValueError if kind == "ValueError" else _lib.MedpyHipError) as ei:
                _call(g, model, kw["op"], kw["kw"])
            assert code is None or ei.value.code == getattr(_lib, code), (what, str(ei.value))
            _same_readbacks(before, _readbacks(g, model))
            assert _changed(g) == changed, what
            _assert_state(g, model, what)
        elif op == "check_current":
            # the n == 0 edits kept the solve (the cut sets need one) and the snapshot
            assert model.solved
            g.__dict__["_cut_sets_cache"] = {}
            fs = g.source_side()
            assert not exact or np.array_equal(fs, model.cut[2]), what
            _assert_solve(g, model, what)
        elif op == "remember_nweights":
            remembered = {off: g.nweights_offset(off) for o in model.offsets for off in (o, sm.neg(o))}
        elif op == "compare_nweights":
            # the capacities written out by the first edit: bit for bit what the image gave, but for the edited arcs
            strides = [int(np.prod(model.shape[k + 1:])) for k in range(len(model.shape))]
            for off, was in remembered.items():
                step = sum(v * s for v, s in zip(off, strides))
                for a, b in list(zip(kw["i"].tolist(), kw["j"].tolist())) + list(zip(kw["j"].tolist(), kw["i"].tolist())):
                    if b - a == step and all(0 <= p + v < n for p, v, n in zip(np.unravel_index(a, model.shape), off, model.shape)):
                        was.ravel()[a] = model.arc_capacity(a, b)
                now = g.nweights_offset(off)
                assert np.array_equal(sm.bits(np.nan_to_num(now)), sm.bits(np.nan_to_num(was))) and np.array_equal(np.isnan(now), np.isnan(was)), (what, off)
        elif op == "iterate":
            flows, converged = model.iterate_regional_histogram(kw["max_refits"])
            res = g.iterate_regional_histogram(max_refits=kw["max_refits"])
            assert len(res["rounds"]) == len(flows) and res["converged"] == converged, (what, res, flows)
            for r, f in zip(res["rounds"], flows):
                assert r["flow"] == pytest.approx(f, rel=1e-9), what
            _assert_state(g, model, what)
            _assert_solve(g, model, what)
        else:
            want = sm.apply_step(model, op, kw)
            got = _call(g, model, op, kw)
            if op == "refit":
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            if op == "clear_nweight_edits":
                assert g.nweight_edit_info()["pairs_kept"] == 0
                continue   # (unbuilt until the build that follows)
            _assert_state(g, model, what)
            if op == "update_boundary_term":
                assert g.boundary_update_info()["arcs_changed"] == model.arcs_changed, (what, g.boundary_update_info(), model.arcs_changed)
            if op == "edit_nweights":   # the residuals of an edited pair: inside the pair's new capacities, and together all of them
                for a, b, c, r in zip(kw["i"].tolist(), kw["j"].tolist(), kw["cap"].tolist(), kw["rev"].tolist()):
                    rab, rba = g.get_edge(a, b), g.get_edge(b, a)
                    assert 0.0 <= rab <= c + r and 0.0 <= rba <= c + r, (what, a, b, rab, rba)
                    assert rab + rba == (c + r if exact else pytest.approx(c + r, rel=1e-9, abs=0.0)), (what, a, b, rab, rba)
    # the end of the session: a cold rebuild of the same handle, and a fresh handle of the model's final arrays
    flow = _assert_solve(g, model, "end")
    labels = g.labels().copy()
    model.build()
    g._build()
    _assert_state(g, model, "rebuilt")
    flow2 = _assert_solve(g, model, "rebuilt")
    assert (flow2 == flow if exact else flow2 == pytest.approx(flow, rel=1e-9)) and np.array_equal(g.labels(), labels)
    fresh = _open(model, from_arrays=True)
    flow3 = fresh.maxflow()
    assert (flow3 == flow if exact else flow3 == pytest.approx(flow, rel=1e-9)) and np.array_equal(fresh.labels(), labels)
    if exact:
        assert np.array_equal(sm.bits(fresh.tweights()), sm.bits(g.tweights()))
    fresh.close()
    g.close()


# ---- the sessions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("case", A_CASES, ids=_id)
def test_session_on_arrays(case, forms, monkeypatch):
    """family A: integer capacities, two equal walls, an integer store, a uint8 feature image of five values, markers on the two
    end faces.  On the full neighbourhoods the session opens with a store that a list edit alone filled, a rebuild, the binned
    update and a rebuild: tweight_edit_info()["dense_calls"] (which mgc_maxflow keys the 26-neighbourhood schedule on)
    is 0, 0, 1, 1, as the model's."""
    shape, conn, seed = case
    model, steps = sm.family_a(shape, conn, seed)
    _play(model, steps, forms, monkeypatch)


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("case", B_CASES, ids=_id)
def test_session_on_a_built_in_term(case, forms, monkeypatch):
    """family B: difference_division on an image of 0s and 3s (n-links 1, 1/2 and 1/4), a probability map of quarters, markers of
    weight 65535; update_boundary_term until the first edit_nweights, refused from there on"""
    shape, conn, seed = case
    model, steps = sm.family_b(shape, conn, seed)
    _play(model, steps, forms, monkeypatch)


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("case", C_CASES, ids=_id)
def test_session_on_the_histogram_term(case, forms, monkeypatch):
    """family C: the inputs of test_gpu_histogram_term.py; refits between marker, n-link and t-link edits, then the iterated refit"""
    shape, conn, kind, seed = case
    model, steps = sm.family_c(shape, conn, kind, seed)
    _play(model, steps, forms, monkeypatch)


# ---- what the 26- and 8-neighbourhood schedule is keyed on ------------------------------------------------------------------------------
def _kinds(g):
    return {k for k, v in g.launch_counts().items() if v}


FULL = [(s, c) for s, c in sm.FAMILY_A if c not in (None, 2 * len(s))]


@pytest.mark.parametrize("shape,conn", FULL, ids=[sm.case_id(s, c) for s, c in FULL])
def test_the_schedule_follows_dense_calls_through_edits_and_rebuilds(shape, conn):
    """a store that dense calls filled counts as a regional term when mgc_maxflow picks the schedule of the full
    neighbourhood, a store that only list edits filled does not.  The opening of the family A session: a list edit gives the
    handle its store and a rebuild follows -- the cold solve launches the kernel forms of a handle that was given the same list
    and built once; then update_tweights_binned and a rebuild -- the forms of a handle built cold from the expanded arrays by
    one dense call.  tweight_edit_info() says 0 dense calls in the first pair and 1 in the second."""
    model, steps = sm.family_a(shape, conn, 0)
    builds = [k for k, (op, _) in enumerate(steps) if op == "build"][:2]
    g = _open(model)
    seen = []
    for number, (op, kw) in enumerate(steps[:builds[1] + 2]):
        if op == "maxflow":
            assert g.maxflow() == model.solve()[0]
            if number - 1 in builds:   # the cold solve behind a rebuild
                cold = _open(model, from_arrays=True) if model.dense_calls else _open(sm.family_a(shape, conn, 0)[0])
                if not model.dense_calls:
                    edit = next(kw2 for op2, kw2 in steps if op2 == "edit_tweights")
                    cold.edit_tweights(edit["ids"], edit["source"], edit["sink"])
                    cold._build()
                assert cold.maxflow() == model.cut[0] and np.array_equal(cold.labels(), g.labels())
                assert cold.tweight_edit_info()["dense_calls"] == g.tweight_edit_info()["dense_calls"] == model.dense_calls
                print("dense_calls %d: %s" % (model.dense_calls, sorted(_kinds(g))))
                assert _kinds(g) == _kinds(cold), (model.dense_calls, sorted(_kinds(g)), sorted(_kinds(cold)))
                seen.append((model.dense_calls, _kinds(g)))
                cold.close()
        else:
            sm.apply_step(model, op, kw)
            _call(g, model, op, kw)
            assert g.tweight_edit_info() == model.tweight_info(), (number, op)
    assert [n for n, _ in seen] == [0, 1]
    assert seen[0][1] != seen[1][1], seen   # (k26_discharge on the general defaults, k26_discharge_w for a regional term: DESIGN 12, "Measured")
    g.close()
