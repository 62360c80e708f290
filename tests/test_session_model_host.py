"""The host model of a handle and the session scripts (tests/session_model.py), checked on the CPU against the BK oracle alone.

1. After every step the model's cut -- BK on ``merged()`` and ``capacities()`` -- equals the cut of a BK graph assembled from
   scratch by the straight-line code below, which goes through the history of calls and uses neither ``merge_tweights_into`` nor
   an override dict: the store as the two arrays of the one dense call it is equivalent to, fed to BK call by call in merge
   order, the n-links written arc by arc.  Family B takes its graph from oracle.pipeline.build_graph and moves the edited arcs
   on it.
2. The scripts are not vacuous: per committed seed the labels move at half of the solves at least, unique and ambiguous cuts both
   occur, a barrier closes and a glue raises an arc across the cut that is current, a tile gains its first t-link and one loses its
   last, and every refused call is refused by the model for the reason the script gives.
3. Family C: at every solve BK's ambiguity set is empty at tol 0 and at 64 ulp, the condition for comparing labels voxel for voxel.

Every session is replayed once per module and shared."""
import numpy as np
import pytest

import session_model as sm

_RUNS = {}

A_CASES = [("A", shape, conn, None, seed) for shape, conn in sm.FAMILY_A for seed in sm.seeds("A", shape)]
B_CASES = [("B", shape, conn, None, seed) for shape, conn in sm.FAMILY_B for seed in sm.seeds("B", shape)]
C_CASES = [("C", shape, conn, kind, seed) for shape, conn, kind in sm.FAMILY_C for seed in sm.seeds("C", shape)]


def _id(case):
    family, shape, conn, kind, seed = case
    return "%s_%s_seed%d" % (family, sm.case_id(shape, conn), seed)


def _script(case):
    family, shape, conn, kind, seed = case
    if family == "A":
        return sm.family_a(shape, conn, seed)
    if family == "B":
        return sm.family_b(shape, conn, seed)
    return sm.family_c(shape, conn, kind, seed)


# ---- the cold construction: straight-line code over the history of calls ---------------------------------------------------------------
def _cold_cut(model):
    from oracle import bk, cutcheck, energy_numpy, pipeline
    from medpy_amd.graphcut import histogram as H
    shape, n = model.shape, model.nvox
    first = model.history[0][1]
    S = K = None
    if first["store"] is not None:
        S, K = (np.array(a, np.float64).ravel() for a in first["store"])
    prob, fg, bg = first["prob"], first["fg"], first["bg"]
    boundary = None if first["boundary"] is None else dict(first["boundary"])
    edits = []

    def fit(fg_sel, bg_sel):
        nbins, lo, width = H.histogram_binning(model.feature, first["hist"]["bins"])
        b = H.histogram_bins(model.feature, nbins, lo, width)
        st, kt = H.histogram_tables(np.bincount(b[fg_sel], minlength=nbins), np.bincount(b[bg_sel], minlength=nbins), first["hist"]["lam"], first["hist"]["eps"])
        return st[b].ravel(), kt[b].ravel()
    if first["hist"] is not None:
        S, K = fit(fg, bg)
    for op, kw in model.history[1:]:
        if op == "edit_markers":
            fg, bg = fg.copy(), bg.copy()
            for v in kw["erase"]:
                fg.ravel()[v] = bg.ravel()[v] = False
            for v in kw["fg"]:
                fg.ravel()[v] = True
            for v in kw["bg"]:
                bg.ravel()[v] = True
        elif op == "update_markers":
            fg, bg = kw["fg"], kw["bg"]
        elif op == "update_regional_term":
            prob = (kw["prob"], kw["alpha"])
        elif op == "update_tweights_dense":
            S, K = kw["source"].ravel().copy(), kw["sink"].ravel().copy()
        elif op == "update_tweights_binned":
            S, K = kw["source_table"][kw["bins"]].ravel(), kw["sink_table"][kw["bins"]].ravel()
        elif op == "fit":
            S, K = fit(kw["fg_sel"], kw["bg_sel"])
        elif op == "edit_tweights":
            if S is None:
                S, K = np.zeros(n), np.zeros(n)
            for v, s, k in zip(kw["ids"], kw["source"], kw["sink"]):
                S[v], K[v] = s, k
        elif op == "edit_nweights":
            edits += list(zip(kw["i"].tolist(), kw["j"].tolist(), kw["cap"].tolist(), kw["rev"].tolist()))
        elif op == "clear_nweight_edits":
            edits = []
        elif op == "update_boundary_term":
            boundary = dict(boundary, image=kw["image"], sigma=kw["sigma"])
        else:
            assert op == "rebuild", op
    if boundary is None:
        g = bk.BKGraph(n, n * 13 + 16)
        if S is not None:
            g.add_tweights(None, S, K)
        nw = {o: (t.copy(), b.copy()) for o, (t, b) in first["nw"].items()}
        for i, j, c, r in edits:
            ci, cj = np.unravel_index(i, shape), np.unravel_index(j, shape)
            o = tuple(int(b) - int(a) for a, b in zip(ci, cj))
            if o in nw:
                nw[o][0][ci], nw[o][1][ci] = c, r
            else:
                o = tuple(-v for v in o)
                nw[o][0][cj], nw[o][1][cj] = r, c
        for o, (there, back) in nw.items():
            mask, i, j = sm.arcs(shape, o)
            g.sum_edges(i, j, there[mask], back[mask])
        for m, (s, t) in ((fg, (sm.MAX, 0.0)), (bg, (0.0, sm.MAX))):
            idx = np.flatnonzero(m.ravel())
            if idx.size:
                g.add_tweights(idx, np.full(idx.size, s), np.full(idx.size, t))
    else:
        # (exact arithmetic: the order of the t-link calls and a capacity moved by a difference change nothing)
        g = pipeline.build_graph(fg, bg, term=boundary["term"], image=boundary["image"], sigma=boundary["sigma"], prob=None if prob is None else prob[0],
                                 alpha=None if prob is None else prob[1], connectivity=model.conn)
        prob = None
        if S is not None:
            g.add_tweights(None, S, K)
        weights = energy_numpy.boundary_weights(boundary["term"], boundary["image"], boundary["sigma"])
        now = {}
        for i, j, c, r in edits:
            ci, cj = np.unravel_index(i, shape), np.unravel_index(j, shape)
            axis = next(k for k in range(len(shape)) if ci[k] != cj[k])
            w = float(weights[axis][ci if cj[axis] > ci[axis] else cj])
            old_c, old_r = now.get((i, j), w), now.get((j, i), w)
            g.sum_edges([i], [j], [c - old_c], [r - old_r])
            now[(i, j)], now[(j, i)] = c, r
    if prob is not None:
        p, alpha = prob
        g.add_tweights(None, (p * alpha).ravel().astype(np.float64), ((1 - p) * alpha).ravel().astype(np.float64))
    flow = g.maxflow()
    fs, ts, amb = cutcheck.ambiguity(g, tol=0.0)
    return flow, ~ts.reshape(shape), fs.reshape(shape), amb.reshape(shape)


def _crosses(model, labels, i, j, cap, rev):
    """per listed pair: (capacity before, capacity after) of its arc from the source side of ``labels`` to the sink side, or None"""
    out = []
    flat = labels.ravel()
    for a, b, c, r in zip(i.tolist(), j.tolist(), cap.tolist(), rev.tolist()):
        if flat[a] and not flat[b]:
            out.append((model.arc_capacity(a, b), c))
        elif flat[b] and not flat[a]:
            out.append((model.arc_capacity(b, a), r))
    return out


def _run(case):
    """the session replayed on a model, once: what the tests below look at"""
    if case in _RUNS:
        return _RUNS[case]
    model, steps = _script(case)
    exact = model.exact_k is not None
    out = dict(solves=0, moved=0, unique=0, ambiguous=0, barrier=0, glue=0, first_tlink=0, last_tlink=0, refused=[], amb64=[], ops=[op for op, _ in steps],
               cold_checks=0)
    labels_before = None
    for op, kw in steps:
        if op == "refused":
            snapshot, solved, info = model.snapshot, model.solved, (model.tweight_info(), len(model.overrides))
            tr, caps, history = model.merged(), model.capacities(), len(model.history)
            try:
                sm.apply_step(model, kw["op"], kw["kw"])
                out["refused"].append((kw["op"], kw["reason"], "accepted"))
            except sm.Refused as e:
                out["refused"].append((kw["op"], kw["reason"], e.reason))
            assert model.snapshot is snapshot and model.solved == solved and info == (model.tweight_info(), len(model.overrides)) and len(model.history) == history
            assert np.array_equal(tr[0], model.merged()[0]) and all(np.array_equal(caps[o][d], model.capacities()[o][d]) for o in caps for d in (0, 1))
            continue
        if op in sm.NOT_ON_THE_MODEL:
            continue
        tiles = model.tiles_with_tlinks()
        if op == "edit_nweights" and model.cut is not None:
            for old, new in _crosses(model, model.cut[1], kw["i"], kw["j"], kw["cap"], kw["rev"]):
                out["barrier"] += int(old > 0 and new == 0)
                out["glue"] += int(new > old)
        fresh = op in ("maxflow", "iterate") and not model.solved
        sm.apply_step(model, op, kw)
        after = model.tiles_with_tlinks()
        out["first_tlink"] += int((~tiles & after).any())
        out["last_tlink"] += int((tiles & ~after).any())
        if op in ("maxflow", "iterate") and (fresh or op == "iterate"):
            flow, labels, fs, amb = model.cut
            out["solves"] += 1
            out["moved"] += int(labels_before is not None and not np.array_equal(labels, labels_before))
            out["unique" if not amb.any() else "ambiguous"] += 1
            labels_before = labels
            if not exact:
                out["amb64"].append((int(amb.sum()), model.ambiguity_at(64 * 2.0 ** -52)))
        # 1. the model against the cold construction, after every step that changed it
        if op != "maxflow" or fresh:
            flow, labels, fs, amb = model.bk()
            cflow, clabels, cfs, camb = _cold_cut(model)
            if exact:
                assert flow == cflow, (op, flow, cflow)
            else:
                assert flow == pytest.approx(cflow, rel=1e-12), (op, flow, cflow)
            assert np.array_equal(labels, clabels) and np.array_equal(fs, cfs) and np.array_equal(amb, camb), op
            out["cold_checks"] += 1
    _RUNS[case] = out
    return out


# ---- the tests -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A_CASES + B_CASES + C_CASES, ids=_id)
def test_model_equals_cold_construction_after_every_step(case):
    out = _run(case)
    print(out["cold_checks"], "cold checks,", out["solves"], "solves,", len(out["ops"]), "steps")
    assert out["cold_checks"] >= out["solves"] > 0


@pytest.mark.parametrize("case", A_CASES + B_CASES, ids=_id)
def test_scripts_are_not_vacuous(case):
    out = _run(case)
    print({k: v for k, v in out.items() if k not in ("ops", "refused", "amb64")})
    assert 2 * out["moved"] >= out["solves"], (out["moved"], out["solves"])
    assert out["unique"] >= 1 and out["ambiguous"] >= 1
    assert out["barrier"] >= 1 and out["glue"] >= 1
    if case[0] == "A":   # (family B has no step that takes markers off a whole tile)
        assert out["first_tlink"] >= 1 and out["last_tlink"] >= 1
        assert 25 <= len(out["ops"])


@pytest.mark.parametrize("case", A_CASES + B_CASES, ids=_id)
def test_refused_calls_are_refused_for_the_reason_the_script_gives(case):
    out = _run(case)
    assert out["refused"]
    for op, reason, got in out["refused"]:
        assert got == reason and reason in sm.REASONS, (op, reason, got)
    if case[0] == "A":
        assert {"id out of range", "id twice", "pair twice", "weight not finite"} <= {r for _, r, _ in out["refused"]}
    else:
        assert "capacities held" in {r for _, r, _ in out["refused"]}


@pytest.mark.parametrize("case", C_CASES, ids=_id)
def test_family_c_cuts_are_unique_at_tol_0_and_at_64_ulp(case):
    out = _run(case)
    assert out["solves"] >= 6 and len(out["amb64"]) == out["solves"]
    assert all(a == (0, 0) for a in out["amb64"]), out["amb64"]
    assert out["moved"] >= 1


@pytest.mark.parametrize("family", ["A", "B"])
def test_seeds_change_the_order_of_the_steps_and_scripts_are_deterministic(family):
    cases = [c for c in A_CASES + B_CASES if c[0] == family and c[1] == (17, 9, 10)]
    orders = [tuple(_run(c)["ops"]) for c in cases]
    assert len(set(orders)) == len(orders)
    again = [op for op, _ in _script(cases[0])[1]]
    assert tuple(again) == orders[0]


def test_the_model_imports_and_builds_without_a_device():
    model, steps = sm.family_a((1, 1, 17), None, 0)
    tr, fc = model.merged()
    assert tr.shape == (1, 1, 17) and tr[0, 0, 0] == sm.MAX and tr[0, 0, -1] == -sm.MAX
    assert np.isnan(model.nweights_offset((0, 0, 1))[0, 0, -1]) and np.isnan(model.nweights_offset((0, 0, -1))[0, 0, 0])
    assert model.nweights_offset((0, 0, -1))[0, 0, 1] == model.capacities()[(0, 0, 1)][1][0, 0, 0]
