"""A host model of one VoxelGraph handle driven through a session of warm edits, and the session scripts both tiers replay
(tests/test_session_model_host.py on the CPU, tests/test_gpu_sessions.py on the device).  No tests in here; NumPy only (the BK
oracle is imported where a cut is asked for).

``HandleModel`` holds what a cold build would be given -- the n-links as per-offset (there, back) arrays or as a built-in term
with its image and sigma, the override dict of ``edit_nweights``, the explicit t-link store as (tr, share), the probability map,
the two marker masks, the feature image -- and one method per public call that applies the documented rule and
nothing cleverer.  It also tracks ``snapshot``: None, or the label volume ``changed_labels()`` compares against.

A session is a seeded list of steps ``(op, kwargs)``; ``family_a`` / ``family_b`` / ``family_c`` generate them and return
``(model as built, steps)``.  The generators run a model of their own while they draw, because several steps aim at the cut
that is current when they come (a barrier across it, a voxel on its far side).  ``apply_step`` replays one step on a model.

Families A and B are exact: every capacity and t-link times 2^k is a whole number for the session's k and all of them together stay
below 2^53 (``assert_exact``), so flow, labels and the two cut sets of every maximum flow are the same and no comparison needs
a tolerance.  Family C is the floating-point histogram term, compared as tests/test_gpu_histogram_term.py does."""
import itertools

import numpy as np

MAX = 65535.0   # GCGraph.MAX
TILE = 8


class Refused(Exception):
    """a call the library refuses before its first write; ``reason`` is one of the strings of REASONS"""

    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


REASONS = ("id out of range", "id twice", "pair twice", "weight not finite", "not neighbours", "capacities held")


# ---- the lattice ----------------------------------------------------------------------------------------------------------------------
def offsets(ndim, conn):
    """the forward half of the neighbourhood: every arc pair once"""
    if conn in (None, 2 * ndim):
        return [tuple(1 if k == a else 0 for k in range(ndim)) for a in range(ndim)]
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if o > (0,) * ndim]


def neg(off):
    return tuple(-o for o in off)


def arcs(shape, off):
    """(mask of the voxels p with p + off inside, ids of those p, ids of p + off)"""
    ids = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    mask = np.zeros(shape, bool)
    mask[src] = True
    return mask, ids[src].ravel(), ids[dst].ravel()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.int64)


def tile_ids(shape):
    """the number of the 8 x 8 x 8 tile of every voxel (volumes of fewer axes: leading axes of extent 1)"""
    shape3 = (1,) * (3 - len(shape)) + tuple(shape)
    grid = [(n + TILE - 1) // TILE for n in shape3]
    z, y, x = np.meshgrid(*[np.arange(n) // TILE for n in shape3], indexing="ij")
    return ((z * grid[1] + y) * grid[2] + x).reshape(shape), int(np.prod(grid))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class HandleModel(object):
    def __init__(self, shape, conn=None, nw=None, boundary=None, store=None, prob=None, fg=None, bg=None, feature=None, hist=None,
                 exact_k=None):
        """``nw``: {forward offset: (there, back)} or None; ``boundary``: dict(term="difference_division", image=, sigma=) or None;
        ``store``: (source, sink) of ONE dense call or None; ``prob``: (map, alpha) or None; ``hist``: dict(bins=, lam=, eps=) --
        the histogram term, fitted to the markers when the graph is built (then ``store`` must be None); ``exact_k``: the k of the
        exactness condition, None for a floating-point session"""
        self.shape, self.conn = tuple(shape), conn
        self.nvox = int(np.prod(self.shape))
        self.offsets = offsets(len(self.shape), conn)
        self.nw = None if nw is None else {o: (np.array(t, np.float64), np.array(b, np.float64)) for o, (t, b) in nw.items()}
        self.boundary = None if boundary is None else dict(boundary)
        self.overrides = {}                 # (i, j) with i < j -> (capacity i -> j, capacity j -> i)
        self.cap0 = nw is not None          # the handle holds its capacities as built (update_boundary_term is refused)
        self.tr = self.share = None         # the explicit t-link store
        self.dense_calls = self.list_entries = self.voxels_changed = 0
        self.prob = None if prob is None else (np.array(prob[0]), float(prob[1]))
        self.fg = np.zeros(self.shape, bool) if fg is None else np.array(fg, bool)
        self.bg = np.zeros(self.shape, bool) if bg is None else np.array(bg, bool)
        self.feature = None if feature is None else np.array(feature)
        self.hist = None
        self.exact_k = exact_k
        self.pairs_changed = 0
        self.arcs_changed = None            # of the last update_boundary_term
        self.solved, self.cut, self.snapshot = False, None, None
        self.history = [("build", dict(nw=self.nw, boundary=self.boundary, store=store, prob=self.prob, fg=self.fg.copy(), bg=self.bg.copy(),
                                       hist=None if hist is None else dict(hist)))]
        if store is not None:
            self._fresh_store(store[0], store[1])
        if hist is not None:
            from medpy_amd.graphcut import histogram as H
            self.hist = dict(hist, binning=H.histogram_binning(self.feature, hist["bins"]))
            self._fit(self.fg, self.bg)

    # -- the store
    def _fresh_store(self, source, sink):
        """what a cleared store and one add_tweights(source, sink) leave"""
        from medpy_amd.graphcut.graph import merge_tweights_into
        s, k = np.asarray(source, np.float64).ravel(), np.asarray(sink, np.float64).ravel()
        old = np.zeros(self.nvox) if self.tr is None else self.tr.copy()   # (a handle without a store gets a zeroed one first)
        self.tr = np.zeros(self.nvox)
        merge_tweights_into(self.tr, 0.0, np.arange(self.nvox), s, k)
        self.share = np.minimum(s, k)
        self.dense_calls = 1
        return int((bits(old) != bits(self.tr)).sum())

    def _fit(self, fg_sel, bg_sel):
        """the histogram term fitted to two selections of voxels (the markers, or the two sides of a cut)"""
        from medpy_amd.graphcut import histogram as H
        nbins, lo, width = self.hist["binning"]
        b = H.histogram_bins(self.feature, nbins, lo, width)
        fg_hist, bg_hist = np.bincount(b[fg_sel], minlength=nbins), np.bincount(b[bg_sel], minlength=nbins)
        st, kt = H.histogram_tables(fg_hist, bg_hist, self.hist["lam"], self.hist["eps"])
        changed = self._fresh_store(st[b], kt[b])
        return fg_hist, bg_hist, (st, kt), changed

    # -- what every change of the handle does to the solve and the snapshot
    def _list_edit(self):
        if self.solved:
            self.snapshot = self.cut[1].copy()
        self.solved = False

    def _whole_update(self):
        self.snapshot = None
        self.solved = False

    def _check_ids(self, ids):
        ids = np.asarray(ids, np.int64).ravel()
        if ids.size and (ids.min() < 0 or ids.max() >= self.nvox):
            raise Refused("id out of range")
        return ids

    # -- public calls
    def edit_markers(self, fg=None, bg=None, erase=None):
        lists = [self._check_ids(np.empty(0, np.int64) if a is None else a) for a in (fg, bg, erase)]
        self.history.append(("edit_markers", dict(fg=lists[0], bg=lists[1], erase=lists[2])))
        if not sum(a.size for a in lists):
            return
        fgm, bgm = self.fg.ravel().copy(), self.bg.ravel().copy()
        fgm[lists[2]] = False
        bgm[lists[2]] = False
        fgm[lists[0]] = True
        bgm[lists[1]] = True
        self.fg, self.bg = fgm.reshape(self.shape), bgm.reshape(self.shape)
        self._list_edit()

    def update_markers(self, fg, bg):
        self.fg = np.zeros(self.shape, bool) if fg is None else np.array(fg, bool)
        self.bg = np.zeros(self.shape, bool) if bg is None else np.array(bg, bool)
        self.history.append(("update_markers", dict(fg=self.fg.copy(), bg=self.bg.copy())))
        self._whole_update()

    def update_regional_term(self, prob, alpha):
        self.prob = (np.array(prob), float(alpha))
        self.history.append(("update_regional_term", dict(prob=self.prob[0], alpha=self.prob[1])))
        self._whole_update()

    def update_tweights_dense(self, source, sink):
        s, k = np.asarray(source), np.asarray(sink)
        if not (np.isfinite(s).all() and np.isfinite(k).all()):
            raise Refused("weight not finite")
        self.voxels_changed = self._fresh_store(s, k)
        self.list_entries = 0
        self.history.append(("update_tweights_dense", dict(source=s.astype(np.float64), sink=k.astype(np.float64))))
        self._whole_update()

    def edit_tweights(self, ids, source, sink):
        ids = self._check_ids(ids)
        s = np.broadcast_to(np.asarray(source, np.float64), ids.shape)
        k = np.broadcast_to(np.asarray(sink, np.float64), ids.shape)
        if not (np.isfinite(s).all() and np.isfinite(k).all()):
            raise Refused("weight not finite")
        if np.unique(ids).size != ids.size:
            raise Refused("id twice")
        if not ids.size:
            return
        if self.tr is None:
            self.tr, self.share = np.zeros(self.nvox), np.zeros(self.nvox)
        new = s - k
        self.voxels_changed = int((bits(self.tr[ids]) != bits(new)).sum())
        self.list_entries = int(ids.size)
        self.tr[ids] = new
        self.share[ids] = np.minimum(s, k)
        self.history.append(("edit_tweights", dict(ids=ids.copy(), source=s.copy(), sink=k.copy())))
        self._list_edit()

    def update_tweights_binned(self, source_table, sink_table, nbins, lo, width):
        from medpy_amd.graphcut import histogram as H
        st, kt = np.asarray(source_table, np.float64), np.asarray(sink_table, np.float64)
        if not (np.isfinite(st).all() and np.isfinite(kt).all()):
            raise Refused("weight not finite")
        b = H.histogram_bins(self.feature, nbins, lo, width)
        self.voxels_changed = self._fresh_store(st[b], kt[b])
        self.list_entries = 0
        self.history.append(("update_tweights_binned", dict(source_table=st, sink_table=kt, bins=b)))
        self._whole_update()

    def refit_regional_histogram(self):
        fg_hist, bg_hist, tables, changed = self._fit(self.fg, self.bg)
        self.voxels_changed, self.list_entries = changed, 0
        self.history.append(("fit", dict(fg_sel=self.fg.copy(), bg_sel=self.bg.copy())))
        self._whole_update()
        return fg_hist, bg_hist

    def iterate_regional_histogram(self, max_refits):
        """VoxelGraph.iterate_regional_histogram with stop_below = 0: the rounds' flows, and whether it converged"""
        from medpy_amd.graphcut import histogram as H
        assert self.solved
        flows, prev, converged = [], None, False
        nbins = self.hist["binning"][0]
        for r in range(max_refits + 1):
            labels = self.cut[1]
            fg_hist = np.bincount(H.histogram_bins(self.feature, *self.hist["binning"])[labels], minlength=nbins)
            if prev is not None and int(np.abs(fg_hist - prev).sum()) == 0:
                converged = True
                break
            if r == max_refits:
                break
            _, _, _, changed = self._fit(labels, ~labels)
            self.voxels_changed, self.list_entries = changed, 0
            self.history.append(("fit", dict(fg_sel=labels.copy(), bg_sel=~labels)))
            self._whole_update()
            flows.append(self.solve()[0])
            prev = fg_hist
        return flows, converged

    def _pair(self, i, j):
        """(forward offset, coordinates of the pair's tail, is i the tail) of two neighbours, or Refused"""
        ci, cj = np.unravel_index(i, self.shape), np.unravel_index(j, self.shape)
        o = tuple(int(b) - int(a) for a, b in zip(ci, cj))
        if o in self.offsets:
            return o, tuple(int(v) for v in ci), True
        if neg(o) in self.offsets:
            return neg(o), tuple(int(v) for v in cj), False
        raise Refused("not neighbours")

    def edit_nweights(self, i, j, cap, rev=None):
        i, j = self._check_ids(i), self._check_ids(j)
        cap = np.broadcast_to(np.asarray(cap, np.float64), i.shape)
        rev = cap if rev is None else np.broadcast_to(np.asarray(rev, np.float64), i.shape)
        if not (np.isfinite(cap).all() and np.isfinite(rev).all() and (cap >= 0).all() and (rev >= 0).all()):
            raise Refused("weight not finite")
        for a, b in zip(i, j):
            self._pair(int(a), int(b))
        keys = [(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(i, j)]
        if len(set(keys)) != len(keys):
            raise Refused("pair twice")
        if not i.size:
            return
        now = self.capacities()
        changed = 0
        for a, b, c, r, key in zip(i, j, cap, rev, keys):
            o, at, fwd = self._pair(int(a), int(b))
            there, back = (c, r) if fwd else (r, c)
            changed += int(bits(now[o][0][at])[0] != bits(there)[0] or bits(now[o][1][at])[0] != bits(back)[0])
            self.overrides[key] = (float(c), float(r)) if a < b else (float(r), float(c))
        self.pairs_changed = changed
        self.cap0 = True
        self.history.append(("edit_nweights", dict(i=i.copy(), j=j.copy(), cap=cap.copy(), rev=rev.copy())))
        self._list_edit()

    def clear_nweight_edits(self):
        self.overrides = {}
        self.history.append(("clear_nweight_edits", {}))
        self.solved = False

    def build(self):
        self.history.append(("rebuild", {}))
        self._whole_update()

    def update_boundary_term(self, image=None, sigma=None):
        if self.cap0:
            raise Refused("capacities held")
        before = self.capacities()
        if image is not None:
            self.boundary["image"] = np.array(image)
        if sigma is not None:
            self.boundary["sigma"] = float(sigma)
        after = self.capacities()
        self.arcs_changed = 0
        for o in self.offsets:
            mask = arcs(self.shape, o)[0]
            for d in (0, 1):
                self.arcs_changed += int((bits(before[o][d][mask]) != bits(after[o][d][mask])).sum())
        self.history.append(("update_boundary_term", dict(image=self.boundary["image"], sigma=self.boundary["sigma"])))
        self._list_edit()

    # -- outputs
    def base_capacities(self):
        """{forward offset: (there, back)} before the overrides: the arrays, or the built-in term of the image"""
        if self.nw is not None:
            return {o: (t.copy(), b.copy()) for o, (t, b) in self.nw.items()}
        assert self.boundary["term"] == "difference_division"
        img, sigma = np.asarray(self.boundary["image"], np.float64), float(self.boundary["sigma"])
        out = {}
        for o in self.offsets:
            src = tuple(slice(max(0, -v), n - max(0, v)) for v, n in zip(o, self.shape))
            dst = tuple(slice(max(0, v), n - max(0, -v)) for v, n in zip(o, self.shape))
            w = np.zeros(self.shape)
            w[src] = 1.0 / (np.abs(img[src] - img[dst]) / sigma + 1.0)
            out[o] = (w, w.copy())
        return out

    def capacities(self):
        """{forward offset: (there, back)} after the overrides"""
        out = self.base_capacities()
        for (a, b), (c, r) in self.overrides.items():
            o, at, _ = self._pair(a, b)
            out[o][0][at], out[o][1][at] = c, r
        return out

    def nweights_offset(self, off, caps=None):
        """what VoxelGraph.nweights_offset(off) reads: the capacity of p -> p + off, NaN where p + off is outside"""
        caps = self.capacities() if caps is None else caps
        off = tuple(off)
        out = np.full(self.shape, np.nan)
        src = tuple(slice(max(0, -v), n - max(0, v)) for v, n in zip(off, self.shape))
        dst = tuple(slice(max(0, v), n - max(0, -v)) for v, n in zip(off, self.shape))
        if off in caps:
            out[src] = caps[off][0][src]
        else:
            out[src] = caps[neg(off)][1][dst]   # the arc p -> p + off is the way back of the pair whose tail is p + off
        return out

    def arc_capacity(self, i, j):
        caps = self.capacities()
        o, at, fwd = self._pair(int(i), int(j))
        return float(caps[o][0 if fwd else 1][at])

    def merged(self):
        """(per-voxel t-link in the volume's shape, flow constant) in merge order: store, probability map, fg, bg"""
        from medpy_amd.graphcut.graph import merge_tweights_into
        tr = np.zeros(self.nvox) if self.tr is None else self.tr.copy()
        fc = 0.0 if self.share is None else float(np.sum(self.share))
        every = np.arange(self.nvox)
        if self.prob is not None:
            p, alpha = self.prob
            if p.dtype not in (np.float32, np.float64):
                p = p.astype(np.float64)
            fc = merge_tweights_into(tr, fc, every, (p * alpha).ravel().astype(np.float64), ((1 - p) * alpha).ravel().astype(np.float64))
        for m, (s, k) in ((self.fg, (MAX, 0.0)), (self.bg, (0.0, MAX))):
            idx = np.flatnonzero(m.ravel())
            fc = merge_tweights_into(tr, fc, idx, np.full(idx.size, s), np.full(idx.size, k))
        return tr.reshape(self.shape), fc

    def tweight_info(self):
        return dict(store_held=int(self.tr is not None), dense_calls=self.dense_calls, list_entries=self.list_entries,
                    voxels_changed=self.voxels_changed)

    def tiles_with_tlinks(self):
        """bool per tile: does any voxel of it hold a t-link after the merge"""
        tid, ntiles = tile_ids(self.shape)
        return np.bincount(tid.ravel(), weights=(self.merged()[0].ravel() != 0), minlength=ntiles) > 0

    def assert_exact(self):
        """the exactness condition of families A and B: c * 2^k is whole for every capacity and t-link, and all magnitudes together
        stay below 2^53 / 2^k"""
        k = self.exact_k
        assert k is not None
        values = [np.abs(self.merged()[0]).ravel(), np.array([self.merged()[1]])]
        if self.share is not None:
            values.append(np.abs(self.share))
        for o, (t, b) in self.capacities().items():
            mask = arcs(self.shape, o)[0]
            values += [t[mask], b[mask]]
        total = 0.0
        for v in values:
            scaled = v * 2.0 ** k
            assert np.array_equal(scaled, np.floor(scaled)), "a capacity that is no multiple of 2^-%d" % k
            total += float(scaled.sum())
        assert total < 2.0 ** 53, total

    def bk_from(self, tr, flow_const, caps, tol=0.0):
        from oracle import bk, cutcheck
        g = bk.BKGraph(self.nvox, self.nvox * 13 + 16)
        flat = np.asarray(tr, np.float64).ravel()
        g.add_tweights(None, np.maximum(flat, 0.0), np.maximum(-flat, 0.0))
        for o, (there, back) in caps.items():
            mask, i, j = arcs(self.shape, o)
            g.sum_edges(i, j, there[mask], back[mask])
        flow = g.maxflow() + flow_const
        fs, ts, amb = cutcheck.ambiguity(g, tol=tol)
        self._last_graph = g
        return flow, ~ts.reshape(self.shape), fs.reshape(self.shape), amb.reshape(self.shape)

    def bk(self):
        """(flow, labels, from_source, ambiguous) of a fresh BK graph of merged() and capacities()"""
        if self.exact_k is not None:
            self.assert_exact()
        tr, fc = self.merged()
        return self.bk_from(tr, fc, self.capacities())

    def solve(self):
        """maxflow(): the cut of the handle as it stands (computed once per state)"""
        if not self.solved:
            self.cut = self.bk()
            self.solved = True
        return self.cut

    def ambiguity_at(self, tol):
        """the size of BK's ambiguity set of the current solve at another tolerance"""
        from oracle import cutcheck
        assert self.solved
        return int(cutcheck.ambiguity(self._last_graph, tol=tol)[2].sum())


NOT_ON_THE_MODEL = ("refused", "check_current", "remember_nweights", "compare_nweights")   # steps that only assert


def apply_step(model, op, kw):
    """one step of a session on the model; returns what the call returns (Refused passes through)"""
    if op in NOT_ON_THE_MODEL:
        return None
    if op == "maxflow":
        return model.solve()
    if op == "build":
        return model.build()
    if op == "refit":
        return model.refit_regional_histogram()
    if op == "iterate":
        return model.iterate_regional_histogram(kw["max_refits"])
    return getattr(model, op)(**kw)


# ---- sessions -------------------------------------------------------------------------------------------------------------------------
WALLS = {(17, 9, 10): (2, 6), (9, 10, 11): (3, 7), (19, 26): (8, 16), (1, 1, 17): (5, 11), (20, 13, 27): (8, 17)}
FAMILY_A = [((17, 9, 10), None), ((9, 10, 11), 26), ((19, 26), 8), ((1, 1, 17), None), ((20, 13, 27), None)]
FAMILY_B = [((17, 9, 10), None), ((20, 13, 27), None)]
FAMILY_C = [((17, 9, 10), None, "u8"), ((9, 10, 11), 26, "i16"), ((19, 26), 8, "f32")]
SEEDS = (0, 1, 2)
SEEDS_OF = {("A", (1, 1, 17)): (0, 2, 3)}   # seed 1 of the chain moves the labels at 9 of 21 solves only: replaced (test_session_model_host.py)


def seeds(family, shape):
    """the committed seeds of a case: those for which the script meets every condition of tests/test_session_model_host.py"""
    return SEEDS_OF.get((family, tuple(shape)), SEEDS)
BINS = {"u8": None, "i16": 7, "f32": 16}


def case_id(shape, conn):
    return "x".join(map(str, shape)) + "_n%d" % (conn or 2 * len(shape))


def _end_faces(shape):
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[..., 0] = True
    bg[..., -1] = True
    return fg, bg


def _walls_inputs(shape, conn, seed):
    """integer capacities 0..8 on every offset, both directions on their own; the arcs across the planes behind the two walls carry
    ONE array of 0..2 (rolled by the wall's number along axis 0), diagonals across them 0: two walls of equal capacity"""
    rng = np.random.default_rng(1000 + seed)
    walls = WALLS[shape]
    wall_cap = rng.integers(0, 3, shape[:-1]).astype(np.float64)
    if wall_cap.size == 1:
        wall_cap[...] = 1.0 + seed % 2     # (a chain: a wall of capacity 0 would leave nothing to cut)
    nw = {}
    for o in offsets(len(shape), conn):
        axis_arc = sum(1 for v in o if v) == 1
        there, back = rng.integers(0, 9, shape).astype(np.float64), rng.integers(0, 9, shape).astype(np.float64)
        if o[-1]:
            for k, w in enumerate(walls):
                at = w if o[-1] > 0 else w + 1
                cap = (np.roll(wall_cap, k, axis=0) if len(shape) > 1 else wall_cap) if axis_arc else 0.0
                there[..., at] = cap
                back[..., at] = cap
        nw[o] = (there, back)
    x = np.arange(shape[-1])
    outside = np.broadcast_to((x <= walls[0]) | (x > walls[1]), shape)
    pick = outside & (rng.random(shape) < 0.04)
    which = rng.random(shape) < 0.5
    weight = rng.integers(1, 4, shape).astype(np.float64)
    source, sink = np.where(pick & which, weight, 0.0), np.where(pick & ~which, weight, 0.0)
    feature = rng.integers(0, 5, shape).astype(np.uint8)
    return nw, (source, sink), feature


class _Script(object):
    """the steps drawn so far and the generator's own model, kept in step"""

    def __init__(self, model, rng):
        self.model, self.rng, self.steps = model, rng, []

    def add(self, op, **kw):
        self.steps.append((op, kw))
        return apply_step(self.model, op, kw)

    def solve(self):
        return self.add("maxflow")

    def refused(self, op, reason, error, **kw):
        """a call the library must refuse; ``error``: ("ValueError", None) or ("MedpyHipError", "ERR_...")"""
        self.steps.append(("refused", dict(op=op, reason=reason, error=error, kw=kw)))

    def current(self):
        self.steps.append(("check_current", {}))

    def labels(self):
        """of the last solve (the model is not solved behind the script's back)"""
        return self.model.cut[1]

    def crossing(self, limit):
        """up to ``limit`` arcs (i, j) with capacity > 0 from the source side of the current cut to its sink side (where the cut
        crosses no such arc: the arcs of capacity 0 it crosses)"""
        labels = self.labels().ravel()
        caps = self.model.capacities()
        for least in (0.0, -1.0):
            found = []
            for o in self.model.offsets:
                mask, a, b = arcs(self.model.shape, o)
                for tail, head, w in ((a, b, caps[o][0][mask]), (b, a, caps[o][1][mask])):
                    sel = labels[tail] & ~labels[head] & (w > least)
                    found += list(zip(tail[sel].tolist(), head[sel].tolist()))
            if found:
                break
        seen, out = set(), []
        for k in self.rng.permutation(len(found)):
            a, b = found[k]
            if (min(a, b), max(a, b)) not in seen:
                seen.add((min(a, b), max(a, b)))
                out.append((a, b))
            if len(out) == limit:
                break
        return np.array([p[0] for p in out], np.int64), np.array([p[1] for p in out], np.int64)

    def side(self, source_side, count):
        """up to ``count`` unmarked voxels of one side of the current cut"""
        labels = self.labels().ravel()
        free = ~self.model.fg.ravel() & ~self.model.bg.ravel() & (labels == source_side)
        ids = np.flatnonzero(free)
        return np.sort(self.rng.choice(ids, min(count, ids.size), replace=False)) if ids.size else ids


def _tile_pairs(shape, conn):
    """arc pairs across a tile face and, in the full neighbourhood, across a tile edge and a tile corner: (i, j) lists"""
    nd = len(shape)
    out = []
    for o in offsets(nd, conn):
        crossing_axes = [k for k, v in enumerate(o) if v and shape[k] > TILE]
        if sum(1 for v in o if v) != len(crossing_axes) or any(v < 0 for v in o):
            continue
        p = tuple(TILE - 1 if o[k] else min(2, shape[k] - 1) for k in range(nd))
        q = tuple(a + b for a, b in zip(p, o))
        out.append((int(np.ravel_multi_index(p, shape)), int(np.ravel_multi_index(q, shape)), len(crossing_axes)))
    kinds = {}
    for i, j, n in out:
        kinds.setdefault(n, (i, j))
    return [kinds[n] for n in sorted(kinds)]


def family_a(shape, conn, seed):
    """the exact session on arrays; returns (model as built, steps).  On the full neighbourhoods the handle is built without a store
    and the session opens with the steps DESIGN 12's schedule rule is about (a store filled by a list edit alone, a rebuild, the
    binned update, a rebuild)."""
    shape = tuple(shape)
    nw, store, feature = _walls_inputs(shape, conn, seed)
    fg, bg = _end_faces(shape)
    full = conn not in (None, 2 * len(shape))
    kw = dict(shape=shape, conn=conn, nw=nw, store=None if full else store, fg=fg, bg=bg, feature=feature, exact_k=0)
    built = HandleModel(**kw)
    rng = np.random.default_rng(seed)
    s = _Script(HandleModel(**kw), rng)
    n, last = built.nvox, shape[-1]
    binning = dict(nbins=5, lo=0.0, width=1.0)

    def tables():
        return dict(source_table=rng.integers(0, 7, 5).astype(np.float64), sink_table=rng.integers(0, 7, 5).astype(np.float64), **binning)

    def dense(dtype, zero_tile=None):
        pick = rng.random(shape) < 0.15
        which = rng.random(shape) < 0.5
        w = rng.integers(1, 40, shape)
        src, snk = np.where(pick & which, w, 0).astype(dtype), np.where(pick & ~which, w, 0).astype(dtype)
        both = rng.random(shape) < 0.02          # weights on both sides: a share of the flow constant
        src[both] += 3
        snk[both] += 5
        if zero_tile is not None:
            src[zero_tile] = snk[zero_tile] = 0
        return src, snk

    s.solve()
    if full:
        ids = s.side(False, 12)
        s.add("edit_tweights", ids=ids, source=np.full(ids.size, 90.0), sink=np.full(ids.size, 2.0))
        s.solve()
        s.add("build")
        s.solve()
        s.add("update_tweights_binned", **tables())
        s.solve()
        s.add("build")
        s.solve()

    def b_edit_markers():
        f, b = s.side(False, 6), s.side(True, 6)
        b = np.concatenate([b, f[:1]])            # one voxel under both kinds of marker: weight on both sides, a share of the flow constant
        marked = np.flatnonzero(s.model.fg.ravel() | s.model.bg.ravel())
        s.add("edit_markers", fg=f, bg=b, erase=rng.choice(marked, min(5, marked.size), replace=False))
        s.solve()

    def b_update_markers():
        f, b = _end_faces(shape)
        f.ravel()[s.side(False, 8)] = True
        b.ravel()[s.side(True, 8)] = True
        s.add("update_markers", fg=f, bg=b)
        s.solve()

    def b_fill_markers():
        f, b = np.zeros(shape, bool), np.zeros(shape, bool)
        f[..., :last // 2] = True
        b[..., last // 2:] = True
        s.add("update_markers", fg=f, bg=b)     # every voxel under a marker: the cut is unique
        s.solve()
        f, b = _end_faces(shape)
        s.add("update_markers", fg=f, bg=b)
        s.solve()

    def b_edit_tweights():
        a, b = s.side(False, 10), s.side(True, 10)
        ids = np.concatenate([a, b])
        s.add("edit_tweights", ids=ids, source=np.concatenate([np.full(a.size, 100.0), rng.integers(0, 3, b.size).astype(float)]),
              sink=np.concatenate([rng.integers(0, 3, a.size).astype(float), np.full(b.size, 100.0)]))
        s.solve()

    def b_dense(dtype):
        def block():
            src, snk = dense(dtype)
            s.add("update_tweights_dense", source=src, sink=snk)
            s.solve()
        return block

    def b_binned():
        s.add("update_tweights_binned", **tables())
        s.solve()

    def b_barrier():
        i, j = s.crossing(12)
        s.add("edit_nweights", i=i, j=j, cap=np.zeros(i.size), rev=np.zeros(i.size))
        s.solve()

    def b_one_way():
        j, i = s.crossing(12)     # given from the sink side: the way in keeps 3, the way across the cut is closed
        s.add("edit_nweights", i=i, j=j, cap=np.full(i.size, 3.0), rev=np.zeros(i.size))
        s.solve()

    def b_glue():
        i, j = s.crossing(12)
        s.add("edit_nweights", i=i, j=j, cap=np.full(i.size, 64.0), rev=np.full(i.size, 64.0))
        s.solve()

    def b_tile_pairs():
        pairs = _tile_pairs(shape, conn) or [(0, 1)]
        i, j = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        s.add("edit_nweights", i=i, j=j, cap=np.full(i.size, 0.0), rev=np.full(i.size, 7.0))
        s.solve()
        # the same pairs again, the other way round, and one pair whose two capacities stay what they are bit for bit
        c = s.crossing(1)
        a, b = (int(c[0][0]), int(c[1][0])) if c[0].size else (0, 1)
        if (min(a, b), max(a, b)) in {(min(p), max(p)) for p in pairs}:
            a, b = n - 2, n - 1
        i2, j2 = np.concatenate([j, [a]]), np.concatenate([i, [b]])
        s.add("edit_nweights", i=i2, j=j2, cap=np.concatenate([np.full(i.size, 5.0), [s.model.arc_capacity(a, b)]]),
              rev=np.concatenate([np.full(i.size, 1.0), [s.model.arc_capacity(b, a)]]))
        s.solve()

    def b_clear():
        s.add("clear_nweight_edits")
        s.add("build")
        s.solve()

    def b_empty_lists():
        s.solve()
        e = np.empty(0, np.int64)
        s.add("edit_markers", fg=e, bg=e, erase=e)
        s.add("edit_tweights", ids=e, source=np.empty(0), sink=np.empty(0))
        s.add("edit_nweights", i=e, j=e, cap=np.empty(0), rev=np.empty(0))
        s.current()

    def b_refused():
        s.refused("edit_markers", "id out of range", ("ValueError", None), fg=np.array([3, n]), bg=None, erase=None)
        s.refused("edit_tweights", "id out of range", ("MedpyHipError", "ERR_INVALID"), ids=np.array([1, n]), source=np.ones(2), sink=np.ones(2))
        s.refused("edit_tweights", "id twice", ("MedpyHipError", "ERR_INVALID"), ids=np.array([4, 2, 4]), source=np.ones(3), sink=np.ones(3))
        s.refused("edit_tweights", "weight not finite", ("MedpyHipError", "ERR_INVALID"), ids=np.array([1, 2]), source=np.array([1.0, np.nan]), sink=np.ones(2))
        s.refused("edit_nweights", "id out of range", ("MedpyHipError", "ERR_INVALID"), i=np.array([0, n - 1]), j=np.array([1, n]), cap=np.ones(2), rev=np.ones(2))
        s.refused("edit_nweights", "pair twice", ("MedpyHipError", "ERR_INVALID"), i=np.array([0, 1]), j=np.array([1, 0]), cap=np.ones(2), rev=np.ones(2))
        s.refused("edit_nweights", "weight not finite", ("MedpyHipError", "ERR_INVALID"), i=np.array([0]), j=np.array([1]), cap=np.array([np.nan]), rev=np.ones(1))
        s.refused("update_tweights_dense", "weight not finite", ("MedpyHipError", "ERR_INVALID"), source=np.full(shape, np.nan), sink=np.zeros(shape))

    def b_several():
        s.solve()
        s.add("edit_markers", fg=s.side(False, 4), bg=None, erase=None)
        i, j = s.crossing(6)
        s.add("edit_nweights", i=i, j=j, cap=np.zeros(i.size), rev=np.full(i.size, 2.0))
        ids = s.side(True, 8)
        s.add("edit_tweights", ids=ids, source=np.zeros(ids.size), sink=np.full(ids.size, 80.0))
        s.solve()

    def b_list_then_whole():
        s.solve()
        ids = s.side(False, 5)
        s.add("edit_tweights", ids=ids, source=np.full(ids.size, 50.0), sink=np.zeros(ids.size))
        src, snk = dense(np.float64)
        s.add("update_tweights_dense", source=src, sink=snk)   # the whole-array update drops the snapshot the list edit took
        s.solve()
        s.add("edit_markers", fg=None, bg=s.side(True, 3), erase=None)   # not solved: the edit takes no snapshot either
        s.add("update_markers", fg=s.model.fg.copy(), bg=s.model.bg.copy())
        s.add("edit_markers", fg=s.model.fg.ravel().nonzero()[0][:1], bg=None, erase=None)
        s.solve()

    def b_tile():
        tid, ntiles = tile_ids(shape)
        t = int(rng.integers(0, ntiles))
        where = tid == t
        src, snk = dense(np.float64, zero_tile=where)
        s.add("update_tweights_dense", source=src, sink=snk)
        s.solve()
        marked = np.flatnonzero((where & (s.model.fg | s.model.bg)).ravel())
        s.add("edit_markers", fg=None, bg=None, erase=marked)      # the tile's last t-links go
        s.solve()
        v = np.flatnonzero(where.ravel())
        v = v[v.size // 2]
        side = bool(s.labels().ravel()[v])
        s.add("edit_tweights", ids=np.array([v]), source=np.array([0.0 if side else 120.0]), sink=np.array([120.0 if side else 0.0]))   # its first again
        s.solve()
        f, b = _end_faces(shape)
        s.add("update_markers", fg=f, bg=b)
        s.solve()

    blocks = [b_edit_markers, b_update_markers, b_fill_markers, b_edit_tweights, b_dense(np.float64), b_dense(np.float32), b_binned, b_barrier,
              b_one_way, b_glue, b_tile_pairs, b_clear, b_empty_lists, b_refused, b_several, b_list_then_whole, b_tile]
    # the overrides must exist when they are cleared (behind the barrier), and exist again when the session ends with its rebuild (the glue)
    order = [blocks[k] for k in rng.permutation(len(blocks)) if blocks[k] not in (b_clear, b_glue)]
    at = int(rng.integers(order.index(b_barrier) + 1, len(order) + 1))
    order.insert(at, b_clear)
    order.insert(int(rng.integers(at + 1, len(order) + 1)), b_glue)
    for block in order:
        block()
    return built, s.steps


def family_b(shape, conn, seed):
    """the exact session on a built-in term: difference_division on an image of 0s and 3s (sigma 1: n-links 1 and 1/4; sigma 3: 1 and
    1/2), a float32 probability map of quarters with alpha a power of two, markers of weight 65535"""
    shape = tuple(shape)
    rng = np.random.default_rng(2000 + seed)
    last = shape[-1]

    def image(lo, hi):
        img = np.zeros(shape, np.float32)
        img[..., lo:hi] = 3.0
        img[rng.random(shape) < 0.1] = 3.0
        return img

    def prob():
        return (rng.integers(0, 5, shape) / 4.0).astype(np.float32)
    fg, bg = _end_faces(shape)
    kw = dict(shape=shape, conn=conn, boundary=dict(term="difference_division", image=image(last // 3, 2 * last // 3), sigma=1.0),
              prob=(prob(), 2.0), fg=fg, bg=bg, exact_k=3)
    built = HandleModel(**kw)
    s = _Script(HandleModel(**kw), rng)
    n = built.nvox
    s.solve()

    def b_sigma():
        s.add("update_boundary_term", image=None, sigma=3.0 if s.model.boundary["sigma"] == 1.0 else 1.0)
        s.solve()

    def b_image():
        s.add("update_boundary_term", image=image(last // 4, last // 2), sigma=None)
        s.solve()

    def b_regional():
        s.add("update_regional_term", prob=prob(), alpha=float(rng.choice([1.0, 4.0])))
        s.solve()

    def b_update_markers():
        f, b = _end_faces(shape)
        f.ravel()[s.side(False, 8)] = True
        b.ravel()[s.side(True, 8)] = True
        s.add("update_markers", fg=f, bg=b)
        s.solve()

    def b_edit_markers():
        marked = np.flatnonzero(s.model.fg.ravel() | s.model.bg.ravel())
        s.add("edit_markers", fg=s.side(False, 6), bg=s.side(True, 6), erase=rng.choice(marked, 4, replace=False))
        s.solve()

    def b_list_then_sigma():
        s.add("edit_markers", fg=s.side(False, 3), bg=None, erase=None)
        s.add("update_boundary_term", image=None, sigma=3.0 if s.model.boundary["sigma"] == 1.0 else 1.0)   # both keep the snapshot
        s.solve()

    def b_fill_markers():
        f, b = np.zeros(shape, bool), np.zeros(shape, bool)
        f[..., :last // 2] = True
        b[..., last // 2:] = True
        s.add("update_markers", fg=f, bg=b)     # every voxel under a marker: the cut is unique
        s.solve()
        f, b = _end_faces(shape)
        s.add("update_markers", fg=f, bg=b)
        s.solve()

    first = [b_sigma, b_image, b_regional, b_update_markers, b_edit_markers, b_list_then_sigma, b_fill_markers]
    for k in rng.permutation(len(first)):
        first[k]()
    # the first edit by arc list: the handle holds its capacities from here on
    s.steps.append(("remember_nweights", {}))
    i, j = s.crossing(10)
    s.add("edit_nweights", i=i, j=j, cap=np.zeros(i.size), rev=np.full(i.size, 0.5))
    s.steps.append(("compare_nweights", dict(i=i, j=j)))
    s.refused("update_boundary_term", "capacities held", ("MedpyHipError", "ERR_UNSUPPORTED"), image=None, sigma=3.0 if s.model.boundary["sigma"] == 1.0 else 1.0)
    s.solve()

    def c_glue():
        i, j = s.crossing(10)
        s.add("edit_nweights", i=i, j=j, cap=np.full(i.size, 16.0), rev=np.full(i.size, 16.0))
        s.solve()

    def c_barrier():
        i, j = s.crossing(10)
        s.add("edit_nweights", i=i, j=j, cap=np.zeros(i.size), rev=np.zeros(i.size))
        s.solve()

    def c_tweights():
        a, b = s.side(False, 8), s.side(True, 8)
        s.add("edit_tweights", ids=np.concatenate([a, b]), source=np.concatenate([np.full(a.size, 64.0), np.full(b.size, 0.25)]),
              sink=np.concatenate([np.full(a.size, 0.5), np.full(b.size, 64.0)]))
        s.solve()

    def c_refused_again():
        s.refused("update_boundary_term", "capacities held", ("MedpyHipError", "ERR_UNSUPPORTED"), image=image(0, 2), sigma=None)
        s.refused("edit_nweights", "pair twice", ("MedpyHipError", "ERR_INVALID"), i=np.array([0, 1]), j=np.array([1, 0]), cap=np.ones(2), rev=np.ones(2))
        s.refused("edit_tweights", "id out of range", ("MedpyHipError", "ERR_INVALID"), ids=np.array([n]), source=np.ones(1), sink=np.ones(1))

    second = [c_glue, c_barrier, c_tweights, b_update_markers, b_edit_markers, b_regional, c_refused_again]
    for k in rng.permutation(len(second)):
        second[k]()
    return built, s.steps


def _c_inputs(shape, conn, kind):
    """the inputs of tests/test_gpu_histogram_term.py: uniform(0.05, 1) n-links, its three images, the fg box and the far bg face"""
    rng = np.random.default_rng(23)
    nw = {o: (rng.uniform(0.05, 1.0, shape), rng.uniform(0.05, 1.0, shape)) for o in offsets(len(shape), conn)}
    rng = np.random.default_rng(11)
    block = tuple(slice(0, max(1, (n + 1) // 2)) for n in shape[:-1]) + (slice(0, max(1, shape[-1] // 2)),)
    if kind == "u8":
        img = rng.integers(0, 40, shape).astype(np.uint8)
        img[block] += 60
    elif kind == "i16":
        img = rng.integers(-200, 200, shape).astype(np.int16)
        img[block] += 300
    else:
        img = rng.normal(0.0, 1.0, shape).astype(np.float32)
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[tuple(slice(n // 3, n // 3 + 2) for n in shape[:-1]) + (slice(1, 3),)] = True
    bg[..., -1] = True
    return nw, img, fg, bg


def family_c(shape, conn, kind, seed):
    """the floating-point session on the histogram term: refit, edit_markers, refit, edit_nweights, refit, edit_tweights on a few
    voxels, a refit that overwrites them, two rounds of iterate_regional_histogram; the seed moves the strokes and the arcs"""
    shape = tuple(shape)
    nw, img, fg, bg = _c_inputs(shape, conn, kind)
    lam = 4.0 if conn == 26 else 1.0
    kw = dict(shape=shape, conn=conn, nw=nw, fg=fg, bg=bg, feature=img, hist=dict(bins=BINS[kind], lam=lam, eps=0.5))
    built = HandleModel(**kw)
    rng = np.random.default_rng(3000 + seed)
    s = _Script(HandleModel(**kw), rng)
    s.solve()
    s.add("refit")
    s.solve()
    s.add("edit_markers", fg=s.side(False, 5), bg=s.side(True, 5), erase=None)
    s.add("refit")
    s.solve()
    i, j = s.crossing(8)
    s.add("edit_nweights", i=i, j=j, cap=rng.uniform(2.0, 4.0, i.size), rev=np.zeros(i.size))
    s.solve()
    s.add("refit")
    s.solve()
    ids = s.side(False, 6)
    s.add("edit_tweights", ids=ids, source=rng.uniform(20.0, 30.0, ids.size), sink=rng.uniform(0.0, 1.0, ids.size))
    s.solve()
    s.add("refit")      # the binned update overwrites the voxels the list edit set
    s.solve()
    s.add("iterate", max_refits=2)
    s.add("build")
    s.solve()
    return built, s.steps
