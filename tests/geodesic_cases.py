"""The statement of the geodesic distance transform and the cases both test tiers hold the code to.

``expected_geodesic`` is Dijkstra's algorithm with a heap in plain Python, with exactly the association of mgc_geo.h: Python floats
are IEEE f64 and every operation below is rounded on its own.  ``expected_term`` is the regional term on top of two transforms.
The cases are small on purpose: one tile, partial tiles on every axis, eight tiles meeting in a corner, flat and thin volumes, and
three wall images whose best paths make a schedule of tile visits work for its answer.  Every comparison is ``==``.
"""
import functools
import heapq
import itertools
import math

import numpy as np

INF = float("inf")
SWEEP_CAP = 64   # MGC_GEO_SWEEP_CAP


def offsets(ndim, full):
    return [d for d in itertools.product((-1, 0, 1), repeat=ndim) if any(d) and (full or sum(map(abs, d)) == 1)]


def step_length(d, spacing, step):
    """e_d = fl(step * sqrt(fl(fl(fl(a_x^2) + fl(a_y^2)) + fl(a_z^2)))), a_k = fl(spacing_k * |d_k|), x the last axis"""
    acc = None
    for k in range(len(d) - 1, -1, -1):
        a = float(spacing[k]) * float(abs(d[k]))
        t = a * a
        acc = t if acc is None else acc + t
    return float(step) * math.sqrt(acc)


def expected_geodesic(image, seeds, gamma, step, spacing, full):
    """D of the issue: float64 array of the shape of ``seeds``.  ``image`` is not read when gamma == 0 (it may be None)."""
    seeds = np.asarray(seeds)
    shape, nd, n = seeds.shape, seeds.ndim, seeds.size
    sp = [1.0] * nd if spacing is None else [float(s) for s in spacing]
    gamma = float(gamma)
    val = None if gamma == 0 else np.asarray(image).astype(np.float64).ravel().tolist()
    strides = [int(np.prod(shape[k + 1:])) for k in range(nd)]
    arcs = [(d, sum(a * b for a, b in zip(d, strides)), step_length(d, sp, step)) for d in offsets(nd, full)]
    coords = list(np.ndindex(*shape))
    dist = [INF] * n
    heap = []
    for s in np.flatnonzero(seeds.ravel()).tolist():
        dist[s] = 0.0
        heap.append((0.0, s))
    heapq.heapify(heap)
    while heap:
        d, p = heapq.heappop(heap)
        if d > dist[p]:
            continue
        cp = coords[p]
        for off, flat, e in arcs:
            ok = True
            for c, o, m in zip(cp, off, shape):
                if not 0 <= c + o < m:
                    ok = False
                    break
            if not ok:
                continue
            q = p + flat
            w = e if val is None else e + gamma * abs(val[p] - val[q])
            c = d + w
            if c < dist[q]:
                dist[q] = c
                heapq.heappush(heap, (c, q))
    return np.array(dist, dtype=np.float64).reshape(shape)


def expected_term(d_f, d_b, lam):
    """(S, K) of the issue's table, element by element in Python floats"""
    d_f, d_b = np.asarray(d_f, dtype=np.float64), np.asarray(d_b, dtype=np.float64)
    lam = float(lam)
    s, k = np.zeros(d_f.size), np.zeros(d_f.size)
    for i, (f, b) in enumerate(zip(d_f.ravel().tolist(), d_b.ravel().tolist())):
        if f == INF and b == INF:
            continue
        if f == INF:
            k[i] = lam
        elif b == INF:
            s[i] = lam
        else:
            t = f + b
            if t == 0:
                s[i] = k[i] = lam * 0.5
            else:
                s[i], k[i] = lam * (b / t), lam * (f / t)
    return s.reshape(d_f.shape), k.reshape(d_f.shape)


# ---- images -------------------------------------------------------------------------------------------------------------------

def _seed_of(text):
    return sum((i + 1) * ord(c) for i, c in enumerate(text)) % (1 << 31)


def make_image(kind, shape):
    rng = np.random.default_rng([_seed_of(kind)] + list(shape))
    n = int(np.prod(shape))
    if kind == "constant":
        return np.full(shape, 7, dtype=np.uint8)
    if kind == "ramp":
        return (np.arange(n, dtype=np.int32) % 251).reshape(shape)
    if kind == "u8_ties":
        return rng.integers(0, 4, size=shape).astype(np.uint8)
    if kind == "i16":
        return rng.integers(-3000, 3000, size=shape).astype(np.int16)
    if kind == "u16":
        return rng.integers(0, 65536, size=shape).astype(np.uint16)
    if kind == "f32":
        return rng.normal(0, 10, size=shape).astype(np.float32)
    if kind == "f64_decades":
        return (10.0 ** rng.uniform(-6, 6, size=shape)).astype(np.float64)
    if kind == "checker":
        return (np.indices(shape).sum(axis=0) % 2 * 50).astype(np.uint8)
    raise KeyError(kind)


IMAGE_KINDS = ("constant", "ramp", "u8_ties", "i16", "u16", "f32", "f64_decades", "checker")


def make_seeds(kind, shape):
    rng = np.random.default_rng([_seed_of(kind)] + list(shape))
    s = np.zeros(shape, dtype=bool)
    if kind == "first":
        s.flat[0] = True
    elif kind == "last":
        s.flat[-1] = True
    elif kind == "pair":   # two seeds at the same distance from the centre, on opposite sides of it
        p = tuple((m - 1) // 4 for m in shape)
        s[p] = True
        s[tuple(m - 1 - c for c, m in zip(p, shape))] = True
    elif kind == "all":
        s[...] = True
    elif kind == "none":
        pass
    elif kind == "bernoulli_002":
        s = rng.random(shape) < 0.002
    elif kind == "bernoulli_30":
        s = rng.random(shape) < 0.3
    elif kind == "borders":   # only voxels that another tile reads as halo cells; the lowest such corner among them
        idx = np.indices(shape)
        edge = np.zeros(shape, dtype=bool)
        for a, m in enumerate(shape):
            if m > 8:
                edge |= (idx[a] % 8 == 7) & (idx[a] + 1 < m)
                edge |= (idx[a] % 8 == 0) & (idx[a] > 0)
        s = edge & (rng.random(shape) < 0.1)
        if edge.any():
            s[tuple(7 if m > 8 else 0 for m in shape)] = True
    else:
        raise KeyError(kind)
    return s


SEED_KINDS = ("first", "last", "pair", "all", "none", "bernoulli_002", "bernoulli_30", "borders")
SHAPES = ((8, 8, 8), (9, 17, 20), (16, 16, 16), (1, 13, 31), (7, 1, 9), (33, 70), (100,))
GAMMAS = (0.0, 0.37, 1.0, 1000.0)
STEPS = (1.0, 0.5, 0.0)
SPACINGS = (None, (2.5, 0.7, 0.7), (3.3, 1.1, 0.9))


def cut_spacing(spacing, ndim):
    return None if spacing is None else tuple(spacing[:ndim])


# ---- walls --------------------------------------------------------------------------------------------------------------------

WALL = 1000


def _serpentine(xs, zs=(1, 3, 5, 7)):
    """A one-voxel-wide corridor through a block of 8 x 8 x len(xs) cells, as the list of its cells (z, y, x) from one end to the
    other: the rows y = 7, 5, 3, 1 of the layers zs, joined by one-cell doors at alternating ends.  Every other cell is wall, so the
    corridor's cells touch only their predecessor and successor, also across diagonals (rows and layers lie two apart)."""
    cells, ys, row = [], [7, 5, 3, 1], list(xs)
    for zi, z in enumerate(zs):
        for yi, y in enumerate(ys):
            cells += [(z, y, x) for x in row]
            row = row[::-1]
            if yi < 3:
                cells.append((z, (y + ys[yi + 1]) // 2, row[0]))
        if zi + 1 < len(zs):
            cells.append((z + 1, ys[-1], row[0]))
        ys = ys[::-1]
    return cells


def wall_corridor_2d():
    """(a), (33, 70): a corridor that runs along the border between the tile rows 0 and 1 (y = 7 | 8) and changes sides every three
    columns: its best path crosses the same tile borders back and forth, so a tile that has settled is woken again and again."""
    shape = (33, 70)
    img = np.full(shape, WALL, dtype=np.int16)
    prev = 7
    for x in range(shape[1]):
        y = 7 if (x // 3) % 2 == 0 else 8
        img[y, x] = 0
        img[prev, x] = 0
        prev = y
    seeds = np.zeros(shape, dtype=bool)
    seeds[7, 0] = True
    return img, seeds


def wall_serpentine():
    """(b), (8, 8, 8): the serpentine through the one tile, 142 arcs from end to end -- more than two visits' worth of sweeps"""
    shape = (8, 8, 8)
    img = np.full(shape, WALL, dtype=np.int16)
    path = _serpentine(range(7, -1, -1))
    for c in path:
        img[c] = 0
    seeds = np.zeros(shape, dtype=bool)
    seeds[path[0]] = True
    return img, seeds


def wall_diagonal():
    """(c), (16, 16, 16): a corridor whose only opening into the chamber [8, 12)^3 of the last tile is the diagonal step
    (7, 7, 7) -> (8, 8, 8).  The corridor starts deep in the tile beside the first one, winds through it and through the first tile
    and ends in that corner cell; a second seed sits in the wall itself, in the last tile, so that every wall voxel has its small
    final value early and the chamber's tile hears of the corridor from the corner cell alone, late.  At the full neighbourhood the
    chamber is a step of sqrt(3) from the corridor's end; at the face neighbourhood the only ways in lead through the wall."""
    shape = (16, 16, 16)
    img = np.full(shape, WALL, dtype=np.int16)
    first = _serpentine(range(7, -1, -1))                       # (1, 7, 7) ... (7, 7, 7)
    beside = [(z, y, x) for z, y, x in _serpentine(range(9, 16), zs=(1, 3, 5))]   # (1, 7, 9) ... (5, 1, 9): x = 8 stays wall but for the link
    path = beside[::-1] + [(1, 7, 8)] + first
    for c in path:
        img[c] = 0
    img[8:12, 8:12, 8:12] = 0
    assert path[-1] == (7, 7, 7)
    seeds = np.zeros(shape, dtype=bool)
    seeds[path[0]] = True
    seeds[15, 15, 15] = True
    return img, seeds


WALLS = {"wall_corridor_2d": wall_corridor_2d, "wall_serpentine": wall_serpentine, "wall_diagonal": wall_diagonal}


# ---- the cases ----------------------------------------------------------------------------------------------------------------

class Case(object):
    def __init__(self, name, shape, image_kind, seed_kind, gamma, step, spacing, full):
        self.name, self.shape, self.image_kind, self.seed_kind = name, tuple(shape), image_kind, seed_kind
        self.gamma, self.step, self.spacing, self.full = float(gamma), float(step), cut_spacing(spacing, len(shape)), int(full)

    def __repr__(self):
        return self.name

    @property
    def connectivity(self):
        return len(self.shape) if self.full else 1

    def inputs(self):
        """(image, seeds): the image as the handle gets it (its own dtype), the seeds as a bool array"""
        return _inputs(self.image_kind, self.seed_kind, self.shape)

    def expected(self):
        return _expected(self)


@functools.lru_cache(maxsize=None)
def _inputs(image_kind, seed_kind, shape):
    if image_kind in WALLS:
        img, seeds = WALLS[image_kind]()
    else:
        img, seeds = make_image(image_kind, shape), make_seeds(seed_kind, shape)
    img.setflags(write=False)
    seeds.setflags(write=False)
    return img, seeds


@functools.lru_cache(maxsize=None)
def _expected(case):
    img, seeds = case.inputs()
    out = expected_geodesic(img, seeds, case.gamma, case.step, case.spacing, case.full)
    out.setflags(write=False)
    return out


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        tag = "x".join(map(str, shape))
        for i in range(16):   # every image kind at both neighbourhoods, every seed kind twice, the parameters in rotation
            j = i // 8
            image_kind, seed_kind = IMAGE_KINDS[i % 8], SEED_KINDS[(i + 3 * j + si) % 8]
            gamma, step, spacing, full = GAMMAS[(i + j + si) % 4], STEPS[(i + si) % 3 if i % 5 else 0], SPACINGS[(i + j + si) % 3], (i + j) % 2
            if step == 0 and gamma == 0:
                gamma = 0.37   # (the two zeros together have cases of their own below)
            out.append(Case("%s-%s-%s-g%g-s%g-sp%d-%s" % (tag, image_kind, seed_kind, gamma, step, (i + j + si) % 3, "full" if full else "face"), shape, image_kind,
                            seed_kind, gamma, step, spacing, full))
        for full in (0, 1):   # step = 0 and gamma = 0 together: everything a seed connects to is 0
            out.append(Case("%s-zero-%s" % (tag, "full" if full else "face"), shape, "u8_ties", "bernoulli_002" if full else "first", 0.0, 0.0, None, full))
    for kind, shape in (("wall_corridor_2d", (33, 70)), ("wall_serpentine", (8, 8, 8)), ("wall_diagonal", (16, 16, 16))):
        for full in (0, 1):
            for gamma in (1000.0, 1.0):
                out.append(Case("%s-g%g-%s" % (kind, gamma, "full" if full else "face"), shape, kind, kind, gamma, 1.0, None, full))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
