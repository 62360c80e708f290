"""The cases of the seeded watershed and of the minimum filter of its markers, and the definition of
medpy_amd/csrc/mgc_ws.h stated once more in NumPy and heapq, independently of the C++ lines:

  statement(image, markers, mask)    T (the arrival words), the parents and the labels: Dijkstra over the words (H, D)
  meyer_flood(image, markers, mask)  the literal priority flood: a heap keyed by (I, insertion age), a voxel labelled when first pushed
  minima_statement(image, size)      image == minimum_filter(image, size) with the `reflect` border, window placed as SciPy places it

Shared by the CPU tier (test_watershed_cases_host.py), the GPU tier (test_gpu_watershed.py) and tools/gen_watershed_golden.py.
Results of the statement are computed once per case and kept (``solved``): nobody may change them."""
import collections
import functools
import heapq

import numpy as np

INF = (1 << 64) - 1
NONE = 0xFFFFFFFF
SWEEP_CAP = 64
DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32")
DTYPE_ID = {"uint8": 0, "int8": 1, "uint16": 2, "int16": 3, "uint32": 4, "int32": 5, "uint64": 6, "int64": 7, "float32": 8, "float64": 9}

Case = collections.namedtuple("Case", "name image markers mask distinct")
MinCase = collections.namedtuple("MinCase", "name image size")


def keys_of(image):
    """the order-preserving uint32 key of every value, as uint64 (mgc_ws_key)"""
    a = np.ascontiguousarray(image)
    if a.dtype == np.float32:
        b = a.view(np.uint32).astype(np.uint64)
        b = np.where(b == 0x80000000, 0, b)
        neg = (b & 0x80000000) != 0
        return np.where(neg, (~b) & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)
    if a.dtype.kind == "i":
        return (a.astype(np.int64) + (1 << 31)).astype(np.uint64)
    assert a.dtype.kind == "u" and a.dtype.itemsize <= 4, a.dtype
    return a.astype(np.uint64)


def _neighbours(shape):
    """per flat index the flat indices of the face neighbours inside the volume, in rising order"""
    shape = tuple(shape)
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    out = [[] for _ in range(idx.size)]
    strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
    coords = np.unravel_index(np.arange(idx.size), shape)
    for sign in (-1, 1):
        for a in (range(len(shape)) if sign < 0 else reversed(range(len(shape)))):
            ok = coords[a] + sign >= 0 if sign < 0 else coords[a] + sign < shape[a]
            for p in np.flatnonzero(ok):
                out[p].append(int(p) + sign * strides[a])
    return out


def statement(image, markers, mask=None):
    """(T as a uint64 array with INF where no seed connects, parents as uint32 with NONE, labels as int32): points 1 to 3 of the
    definition, T by Dijkstra over the words -- ext is monotone and inflationary, so popping the smallest word settles it"""
    image, markers = np.asarray(image), np.asarray(markers)
    shape = image.shape
    key = [int(k) for k in keys_of(image).ravel()]
    mk = [int(m) for m in markers.ravel()]
    inside = [True] * len(key) if mask is None else [bool(m) for m in np.asarray(mask).ravel()]
    nb = _neighbours(shape)
    n = len(key)
    T = [INF] * n
    seed = [inside[p] and mk[p] > 0 for p in range(n)]
    heap = []
    for p in range(n):
        if seed[p]:
            T[p] = key[p] << 32
            heap.append((T[p], p))
    heapq.heapify(heap)
    while heap:
        t, p = heapq.heappop(heap)
        if t != T[p]:
            continue
        h = t >> 32
        for q in nb[p]:
            if not inside[q] or seed[q]:
                continue
            cand = (key[q] << 32) if key[q] > h else t + 1
            if cand < T[q]:
                T[q] = cand
                heapq.heappush(heap, (cand, q))
    parent = [NONE] * n
    label = [0] * n
    for p in sorted(range(n), key=lambda p: T[p]):
        if T[p] == INF:
            break
        if seed[p]:
            parent[p], label[p] = p, mk[p]
            continue
        best = min((T[q], q) for q in nb[p] if T[q] < T[p])   # outside the mask T is INF
        parent[p], label[p] = best[1], label[best[1]]
    return (np.array(T, dtype=np.uint64).reshape(shape), np.array(parent, dtype=np.uint32).reshape(shape), np.array(label, dtype=np.int32).reshape(shape))


def meyer_flood(image, markers, mask=None):
    """Meyer's flood, literally: the seeds enter a heap keyed by (value, insertion age) in flat order; the smallest leaves, and each
    unlabelled neighbour takes its label and enters"""
    image, markers = np.asarray(image), np.asarray(markers)
    key = [int(k) for k in keys_of(image).ravel()]
    mk = [int(m) for m in markers.ravel()]
    inside = [True] * len(key) if mask is None else [bool(m) for m in np.asarray(mask).ravel()]
    nb = _neighbours(image.shape)
    label = [0] * len(key)
    heap, age = [], 0
    for p in range(len(key)):
        if inside[p] and mk[p] > 0:
            label[p] = mk[p]
            heap.append((key[p], age, p))
            age += 1
    heapq.heapify(heap)
    while heap:
        _, _, p = heapq.heappop(heap)
        for q in nb[p]:
            if inside[q] and label[q] == 0:
                label[q] = label[p]
                heapq.heappush(heap, (key[q], age, q))
                age += 1
    return np.array(label, dtype=np.int32).reshape(image.shape)


def reflect(j, n):
    """position j of an axis of n entries under scipy.ndimage's `reflect` border (d c b a | a b c d | d c b a)"""
    m = np.mod(j, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def minimum_filter_statement(image, size):
    """scipy.ndimage.minimum_filter(image, size=size), mode `reflect`: one pass per axis, the window of position i covers
    i - size // 2 .. i - size // 2 + size - 1"""
    out = np.asarray(image)
    for a in range(out.ndim):
        n = out.shape[a]
        idx = reflect(np.arange(n)[:, None] - size // 2 + np.arange(size)[None, :], n)   # [n, size]
        out = np.moveaxis(np.moveaxis(out, a, 0)[idx].min(axis=1), 0, a)
    return out


def minima_statement(image, size):
    image = np.asarray(image)
    return image == minimum_filter_statement(image, size)


def local_minima_statement(image, size):
    """what medpy.filter.image.local_minima returns, with a STABLE sort (the reference's argsort is not: equal values may come in
    another order there)"""
    image = np.asarray(image)
    m = minima_statement(image, size)
    idx, val = np.transpose(m.nonzero()), image[m]
    order = np.argsort(val, kind="stable")
    return idx[order], val[order]


# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


def _perm(shape, rng, dtype="uint32"):
    n = int(np.prod(shape))
    return rng.permutation(n).reshape(shape).astype(dtype)


def _seeds(shape, rng, k, first=1):
    m = np.zeros(shape, np.int32)
    n = int(np.prod(shape))
    for i, p in enumerate(rng.choice(n, size=min(k, n), replace=False)):
        m.flat[p] = first + i
    return m


def _make():
    cases = []

    def add(name, image, markers, mask=None, distinct=False):
        image = np.ascontiguousarray(image)
        markers = np.ascontiguousarray(markers, dtype=np.int32)
        assert image.shape == markers.shape and (mask is None or mask.shape == image.shape)
        cases.append(Case(name, image, markers, None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8), distinct))

    # extents 1, 2, 7, 8, 9, 17 on each axis in turn; tie-heavy and distinct-valued in turn; every second one with a mask
    k = 0
    for axis in range(3):
        for e in (1, 2, 7, 8, 9, 17):
            shape = [5, 9, 10]
            shape[axis] = e
            name = "extent_a%d_%d" % (axis, e)
            rng = _rng(name)
            distinct = k % 2 == 1
            image = _perm(shape, rng) if distinct else rng.integers(0, 4, shape).astype(np.uint8)
            mask = (rng.random(shape) < 0.8) if k % 4 >= 2 else None
            add(name, image, _seeds(shape, rng, 3), mask, distinct)
            k += 1
    for shape in ((1,), (20,), (1, 1), (13, 18), (1, 1, 1)):
        for distinct in (False, True):
            name = "dim%d_%s_%s" % (len(shape), "x".join(map(str, shape)), "perm" if distinct else "ties")
            rng = _rng(name)
            image = _perm(shape, rng, "uint16") if distinct else rng.integers(0, 4, shape).astype(np.uint8)
            add(name, image, _seeds(shape, rng, 2), None, distinct)
    # a plateau of equal values over three tiles: D crosses two borders, from one end and from both
    m = np.zeros((4, 4, 24), np.int32)
    m[1, 2, 0] = 7
    add("plateau_one_seed", np.full((4, 4, 24), 9, np.int16), m)
    m = m.copy()
    m[3, 0, 23] = 4
    add("plateau_two_seeds", np.full((4, 4, 24), 9, np.int16), m)
    # a corridor cut by the mask that winds inside ONE tile for more cells than the sweep cap: a snake in every second slice
    mask = np.zeros((8, 8, 8), np.uint8)
    path = []
    for z in (0, 2, 4, 6):
        rows = []
        for r, y in enumerate((0, 2, 4, 6)):
            xs = list(range(8)) if r % 2 == 0 else list(range(7, -1, -1))
            rows += [(z, y, x) for x in xs]
            if y < 6:
                rows.append((z, y + 1, xs[-1]))
        if (z // 2) % 2 == 1:
            rows.reverse()
        path += rows
        if z < 6:
            path.append((z + 1,) + rows[-1][1:])
    for c in path:
        mask[c] = 1
    assert len(path) == len(set(path)) and len(path) > 2 * SWEEP_CAP
    m = np.zeros((8, 8, 8), np.int32)
    m[path[0]] = 3
    add("corridor_winds_in_one_tile", np.zeros((8, 8, 8), np.uint8), m, mask)
    rng = _rng("corridor_winds_rising")
    image = np.zeros((8, 8, 8), np.uint8)
    for i, c in enumerate(path):
        image[c] = i // 3
    add("corridor_winds_rising", image, m, mask)
    CORRIDOR.append(len(path))
    # a corridor that leaves a tile and re-enters it
    mask = np.zeros((1, 10, 16), np.uint8)
    mask[0, 0, :11] = 1
    mask[0, 1, 10] = 1
    mask[0, 2, :11] = 1
    m = np.zeros((1, 10, 16), np.int32)
    m[0, 0, 0] = 5
    add("corridor_leaves_and_reenters", np.full((1, 10, 16), 2, np.uint8), m, mask)
    # two seeds whose floods meet exactly on a tile face, and one voxel later (the tie goes to the lower index)
    for n in (16, 17):
        m = np.zeros((1, 1, n), np.int32)
        m[0, 0, 0], m[0, 0, n - 1] = 1, 2
        add("meet_on_face_%d" % n, np.zeros((1, 1, n), np.uint8), m)
    m = np.zeros((16, 3, 3), np.int32)
    m[0, 1, 1], m[15, 1, 1] = 2, 1
    add("meet_on_face_z", np.zeros((16, 3, 3), np.uint8), m)
    # a ridge voxel between two basins takes the lower side
    for name, row in (("ridge_left_lower", [0, 1, 5, 2, 0]), ("ridge_right_lower", [0, 2, 5, 1, 0]), ("ridge_level", [0, 1, 5, 1, 0])):
        add(name, np.array(row, np.int8), np.array([1, 0, 0, 0, 2], np.int32))
    # masks and seeds
    rng = _rng("masks")
    shape = (3, 9, 12)
    image = rng.integers(0, 4, shape).astype(np.uint8)
    mask = np.ones(shape, np.uint8)
    mask[:, :, 6] = 0                                      # a wall: the far side has no seed
    m = np.zeros(shape, np.int32)
    m[1, 4, 2] = 1
    add("mask_cuts_a_region_off", image, m, mask)
    m2 = m.copy()
    m2[1, 4, 6] = 2                                        # a seed on the wall is no seed
    add("seed_outside_the_mask", image, m2, mask)
    add("no_seeds", image, np.zeros(shape, np.int32))
    add("no_seeds_masked", image, np.zeros(shape, np.int32), mask)
    add("one_seed", image, m)
    add("one_seed_perm", _perm(shape, rng), m, None, True)
    add("mask_all_zero", image, m, np.zeros(shape, np.uint8))
    add("every_voxel_a_seed", image, np.arange(1, image.size + 1, dtype=np.int32).reshape(shape))
    shape = (3, 20, 20)
    add("markers_above_255", _rng("k300").integers(0, 4, shape).astype(np.uint8), _seeds(shape, _rng("k300s"), 300), None)
    add("markers_above_255_perm", _perm(shape, _rng("k300p")), _seeds(shape, _rng("k300s"), 300, first=2 ** 31 - 300), None, True)
    # every dtype at its extremes
    shape = (3, 9, 10)
    for dt in DTYPES[:-1]:
        info = np.iinfo(dt)
        pool = [info.min, info.min + 1, info.max - 1, info.max, 0, 1] + ([-1, -2] if info.min < 0 else [info.max // 2, info.max // 2 + 1])
        rng = _rng("extremes_" + dt)
        image = np.array(pool, dtype=dt)[rng.integers(0, len(pool), shape)]
        add("extremes_" + dt, image, _seeds(shape, rng, 4), (rng.random(shape) < 0.9))
    rng = _rng("uint32_above_2_31")
    add("uint32_above_2_31", (rng.integers(0, 6, shape).astype(np.uint32) + np.uint32(2 ** 31 - 3)), _seeds(shape, rng, 3))
    pool = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, -1.5, 1.5, -3e38, 3e38, 1.17549435e-38, -1.17549435e-38], dtype=np.float32)
    rng = _rng("float32_zeros_denormals")
    add("float32_zeros_denormals", pool[rng.integers(0, len(pool), shape)], _seeds(shape, rng, 4))
    image = np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    add("float32_signed_zeros", image, _seeds(shape, rng, 3))
    add("float32_distinct", (_perm(shape, rng).astype(np.float32) - 100.0) * np.float32(0.37), _seeds(shape, rng, 4), None, True)
    # tie-heavy and distinct-valued over several tiles, with and without a mask
    shape = (9, 17, 10)
    for distinct in (False, True):
        for masked in (False, True):
            name = "tiles_%s%s" % ("perm" if distinct else "ties", "_masked" if masked else "")
            rng = _rng(name)
            image = _perm(shape, rng) if distinct else rng.integers(0, 4, shape).astype(np.uint8)
            add(name, image, _seeds(shape, rng, 5), (rng.random(shape) < 0.75) if masked else None, distinct)
    # the largest: smooth hills of few levels, a dozen seeds, a mask with holes
    shape = (40, 40, 72)
    rng = _rng("largest")
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    image = (20 + 12 * np.sin(z / 5.0) * np.cos(y / 7.0) + 8 * np.sin(x / 9.0 + y / 11.0)).astype(np.uint16)
    add("largest_hills", image, _seeds(shape, rng, 12), (rng.random(shape) < 0.97))
    return cases


CORRIDOR = []
CASES = _make()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# where the two doctored builds of tests/hostsim/ws_main.cpp must fail, and where their fault cannot show
RISE_RESET_FAILS = ("corridor_winds_rising", "tiles_perm", "largest_hills")
RISE_RESET_PASSES = ("plateau_two_seeds", "meet_on_face_16", "corridor_winds_in_one_tile")      # nothing ever rises: constant images
SELF_WAKE_FAILS = ("corridor_winds_in_one_tile", "corridor_winds_rising")
SELF_WAKE_PASSES = ("plateau_two_seeds", "tiles_perm", "extremes_int16")                          # no visit reaches the cap


@functools.lru_cache(maxsize=None)
def solved(name):
    """(T, parents, labels) of the statement for case ``name``: computed once, read-only"""
    c = BY_NAME[name]
    out = statement(c.image, c.markers, c.mask)
    for a in out:
        a.setflags(write=False)
    return out


def _make_min():
    cases = []
    shapes = ((7,), (3,), (1,), (5, 6), (2, 9), (1, 4), (4, 5, 6), (2, 3, 9), (1, 1, 3), (2, 1, 2))
    for shape in shapes:
        for size in (1, 2, 3, 4, 5):
            name = "min_%s_s%d" % ("x".join(map(str, shape)), size)
            cases.append(MinCase(name, _rng(name).integers(0, 6, shape).astype(np.uint8), size))
    for dt in DTYPES + ("uint64", "int64", "float64"):
        for size in (2, 3):
            name = "min_%s_s%d" % (dt, size)
            rng = _rng(name)
            shape = (4, 7, 9)
            if dt.startswith("float"):
                pool = np.array([-0.0, 0.0, -1.5, 2.5, 1e-40, -1e-40, 7.0], dtype=dt)
            else:
                # scipy.ndimage filters work in float64 whatever the dtype, so beyond 2**53 the reference's mask is no longer that of
                # the exact values (neighbouring integers fall together, uint64's maximum does not survive the way back): the 64-bit
                # cases stay inside +-2**53, where the reference is exact; the device compares exact ranks everywhere
                info = np.iinfo(dt)
                lo, hi = max(info.min, -(2 ** 53)), min(info.max, 2 ** 53)
                pool = np.array([lo, lo + 1, hi, hi - 1, 0, 1, 2], dtype=dt)
            cases.append(MinCase(name, pool[rng.integers(0, len(pool), shape)], size))
    name = "min_wide_16x17x18_s4"
    cases.append(MinCase(name, _rng(name).integers(0, 40, (16, 17, 18)).astype(np.int16), 4))
    return cases


MIN_CASES = _make_min()
MIN_NAMES = [c.name for c in MIN_CASES]
MIN_BY_NAME = {c.name: c for c in MIN_CASES}
assert len(MIN_BY_NAME) == len(MIN_CASES)


def golden_mask(golden, name):
    """the minima mask of case ``name`` from the reference's recorded (indices, values) pair"""
    c = MIN_BY_NAME[name]
    idx = golden[name + "/indices"]
    m = np.zeros(c.image.shape, dtype=bool)
    m[tuple(idx.T)] = True
    return m
