"""Cases of the connected components and of the cleaning rule, shared by the CPU tier (test_cc_cases_host.py) and the
GPU tier (test_gpu_components.py): label patterns as functions of a shape, marker sets, and a plain NumPy / SciPy statement of the
semantics -- expected_components and expected_clean, built on scipy.ndimage.label."""
import numpy as np
from scipy import ndimage

SHAPES = [(8, 8, 8), (16, 8, 8), (9, 10, 11), (17, 16, 31), (24, 24, 24), (40, 33), (70,), (3, 1, 5)]

FLAG_FG, FLAG_BG, FLAG_BORDER = 1, 2, 4
INFO_KEYS = ("components", "voxels", "largest_size", "largest_id", "tiles_skipped", "tiles_processed", "unions", "longest_walk")
CLEAN_KEYS = ("fg_components", "survivors", "voxels_removed", "cavities_filled", "voxels_filled", "voxels_changed", "list_written")


# ---- patterns: shape -> uint8 array, or None where the pattern needs a shape it has not got ---------------------------------------
def zeros(shape):
    return np.zeros(shape, np.uint8)


def ones(shape):
    return np.ones(shape, np.uint8)


def bernoulli(p, seed=0):
    def make(shape):
        return (np.random.default_rng([seed, int(p * 100)] + list(shape)).random(shape) < p).astype(np.uint8)
    make.__name__ = "bernoulli_%02d" % int(p * 100)
    return make


def checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2 == 0).astype(np.uint8)


def _snake(shape):
    """(mask, start, end): a path one voxel wide that visits every second slab of every axis, so it runs through every tile"""
    if len(shape) == 1:
        return np.ones(shape, np.uint8), (0,), (shape[0] - 1,)
    sub, s, e = _snake(shape[1:])
    m = np.zeros(shape, np.uint8)
    start = end = None
    for k, i in enumerate(range(0, shape[0], 2)):
        m[i] = sub
        a, b = (s, e) if k % 2 == 0 else (e, s)
        if start is None:
            start = (i,) + a
        end = (i,) + b
        if i + 2 < shape[0]:
            m[(i + 1,) + b] = 1   # the link to the slab after the next: where this slab's path ends the next one's begins
    return m, start, end


def serpentine(shape):
    return _snake(shape)[0]


def comb(shape):
    """teeth along axis 0 on every second position of the other axes, joined only in the last slab"""
    m = np.zeros(shape, np.uint8)
    m[(slice(None),) + (slice(None, None, 2),) * (len(shape) - 1)] = 1
    if len(shape) == 1:
        m[:] = 0
        m[::2] = 1
    m[-1] = 1
    return m


def shells(shape):
    """nested shells: the layer at distance d from the border of the volume is foreground for odd d -- a cavity in a cavity"""
    d = None
    for ax, n in enumerate(shape):
        if n == 1:
            continue
        i = np.arange(n)
        di = np.minimum(i, n - 1 - i).reshape([n if a == ax else 1 for a in range(len(shape))])
        d = di if d is None else np.minimum(d, di)
    return (np.broadcast_to(d, shape) % 2 == 1).astype(np.uint8)


def corner_touch(shape):
    """two voxels that touch only across a tile corner"""
    if len(shape) < 2 or min(shape) < 9:
        return None
    m = np.zeros(shape, np.uint8)
    m[(7,) * len(shape)] = m[(8,) * len(shape)] = 1
    return m


def edge_touch(shape):
    """pairs of voxels that touch only across a tile edge: (7, 7, z) - (8, 8, z)"""
    if len(shape) != 3 or shape[0] < 9 or shape[1] < 9:
        return None
    m = np.zeros(shape, np.uint8)
    for z in {0, shape[2] - 1}:
        m[7, 7, z] = m[8, 8, z] = 1
    return m


def row_wrap(shape):
    """the last voxel of every even row and the first of the next: consecutive ids, no neighbours"""
    if len(shape) < 2 or shape[-1] < 3:
        return None
    m = np.zeros(shape, np.uint8).reshape(-1, shape[-1])
    m[::2, -1] = 1
    m[1::2, 0] = 1
    return m.reshape(shape)


def bytes_plane(shape):
    """a caller's plane whose foreground bytes are 2 .. 255"""
    rng = np.random.default_rng([7] + list(shape))
    return ((rng.random(shape) < 0.5) * rng.integers(2, 256, shape)).astype(np.uint8)


PATTERNS = [zeros, ones, bernoulli(0.2), bernoulli(0.31), bernoulli(0.5), bernoulli(0.8), checkerboard, serpentine, comb, shells, corner_touch, edge_touch, row_wrap,
            bytes_plane]
CASES = [(p, s) for s in SHAPES for p in PATTERNS if p(s) is not None]


def case_id(case):
    return "%s-%s" % (case[0].__name__, "x".join(str(n) for n in case[1]))


def sparse_markers(shape, seed=3, p=0.02):
    rng = np.random.default_rng([seed] + list(shape))
    fg = (rng.random(shape) < p).astype(np.uint8)
    bg = ((rng.random(shape) < p) & (fg == 0)).astype(np.uint8)
    return fg, bg


# ---- the semantics ----------------------------------------------------------------------------------------------------------------
def border_mask(shape):
    idx = np.indices(shape)
    axes = [a for a, n in enumerate(shape) if n > 1]
    if not axes:
        return np.ones(shape, bool)
    b = np.zeros(shape, bool)
    for a in axes:
        b |= (idx[a] == 0) | (idx[a] == shape[a] - 1)
    return b


def expected_components(mask, side, full, fg=None, bg=None):
    """(ids int32 of the mask's shape, first int64[K], size int64[K], flags uint8[K]) of the components of the foreground (side 1)
    or the background (side 0) of ``mask`` (any byte but 0 is foreground) at the face / full neighbourhood"""
    mask = np.asarray(mask) != 0
    m = mask if side else ~mask
    ids, K = ndimage.label(m, structure=ndimage.generate_binary_structure(m.ndim, m.ndim if full else 1))
    ids = ids.astype(np.int32)
    flat = ids.ravel()
    at = np.flatnonzero(flat)
    _, where = np.unique(flat[at], return_index=True)
    first = at[where].astype(np.int64)
    assert first.size == K and (np.diff(first) > 0).all()   # scipy numbers the components by their first voxel
    size = np.bincount(flat, minlength=K + 1)[1:].astype(np.int64)
    flags = np.zeros(K + 1, np.uint8)
    for bit, plane in ((FLAG_FG, fg), (FLAG_BG, bg), (FLAG_BORDER, border_mask(mask.shape))):
        if plane is not None:
            flags[np.unique(flat[np.asarray(plane).ravel() != 0])] |= bit
    return ids, first, size, flags[1:]


def rule(fg_full=0, min_size=1, largest=0, seeded=0, fill_holes=0, hole_full=0):
    return dict(fg_full=fg_full, min_size=min_size, largest=largest, seeded=seeded, fill_holes=fill_holes, hole_full=hole_full)


def rule_keep(size, flags, min_size=1, largest=0, seeded=0):
    """step 1 of the rule on a table: the kept components as a bool array"""
    passing = [k for k in range(len(size)) if size[k] >= min_size and (not seeded or flags[k] & FLAG_FG)]
    if largest > 0:
        passing = sorted(passing, key=lambda k: (-size[k], k))[:largest]
    keep = np.zeros(len(size), bool)
    keep[passing] = True
    return keep


def expected_clean(mask, r, fg=None, bg=None):
    """(cleaned bool array, ascending changed ids int64, counts dict) of the rule ``r`` (see rule()) applied to ``mask``"""
    F = np.asarray(mask) != 0
    ids, _, size, flags = expected_components(F, 1, r["fg_full"], fg, bg)
    keep = rule_keep(size, flags, r["min_size"], r["largest"], r["seeded"])
    F1 = np.concatenate([[False], keep])[ids]
    info = dict(fg_components=int(size.size), survivors=int(keep.sum()), voxels_removed=int(size[~keep].sum()), cavities_filled=0, voxels_filled=0)
    F2 = F1
    if r["fill_holes"]:
        ids0, _, size0, flags0 = expected_components(F1, 0, r["hole_full"], fg, bg)
        fill = (flags0 & (FLAG_BORDER | FLAG_BG)) == 0
        F2 = F1 | np.concatenate([[False], fill])[ids0]
        info.update(cavities_filled=int(fill.sum()), voxels_filled=int(size0[fill].sum()))
    changed = np.flatnonzero(F2.ravel() != F.ravel()).astype(np.int64)
    info["voxels_changed"] = int(changed.size)
    return F2, changed, info
