"""The cases of the anisotropic diffusion (medpy_amd/csrc/mgc_diffuse.h) and its *statement*: the definition in NumPy
float32 with shifted slices, written from the definition, not from the reference's text.  tests/golden/diffusion.npz holds the
reference's output of every case (tools/gen_diffusion_golden.py); the statement, the host program of the header's lines and the
device are compared with it: ``==`` on every voxel for options 2 and 3, the measured bound for option 1."""
import collections
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "diffusion.npz")

# the brick of one workgroup of k_diffuse (MGC_AD_BZ, MGC_AD_BY, MGC_AD_BX of mgc_diffuse.h; the host test compares)
BZ, BY, BX = 8, 8, 64

# Option 1: e = max|a - golden| / ptp(golden) of the statement (f64 exp, rounded) against the golden file (NumPy's float32 exp),
# the largest over the option-1 cases, measured on the CPU with NumPy 2.2.6 (profiles/diffusion.jsonl has every case; written by
# tools/gen_diffusion_golden.py --measure).  Every option-1 comparison (host program, device) is bounded by 8 x this: the device's
# and glibc's f64 exp may each differ from NumPy's by a last bit before rounding, the roundings compound over niter, and NumPy
# builds differ in their float32 exp.
E1_MEASURED = 2.210518101969579e-07
E1_BOUND = 8 * E1_MEASURED

Case = collections.namedtuple("Case", "name shape dtype pattern seed niter kappa gamma spacing option")

DTYPES = ("uint8", "int16", "uint16", "float32", "float64")
NITERS = (0, 1, 2, 5, 8)
PAIRS = ((50.0, 0.1), (20.5, 0.25), (7.25, 0.05))   # (kappa, gamma)
KAPPA_RAMP = 3.0 / 2 ** 0.5                        # kappa_s = f32(KAPPA_RAMP * 2**0.5) = 3 exactly: the ramp's step
assert np.float32(KAPPA_RAMP * 2 ** 0.5) == np.float32(3.0)

# the smallest shapes at which the brick can go wrong: extents 1 and 2 on every axis, B - 1, B, B + 1 on every axis, 2 Bx + 3,
# x extents that are and are not multiples of 4 (the float4 rows), 1-D and 2-D
SHAPES = [
    (1, 1, 1), (1, 1, 5), (3, 1, 4), (2, 2, 2), (1, 2, 1), (2, 1, 1), (1, 1, 2), (3, 9, 70),
    (2, 3, BX - 1), (2, 3, BX), (2, 3, BX + 1), (1, 2, 2 * BX + 3), (3, BY + 1, BX + 4), (1, BY + 1, 2 * BX),
    (2, BY - 1, 5), (2, BY, 5), (2, BY + 1, 5), (BZ - 1, 3, 5), (BZ, 3, 5), (BZ + 1, 3, 5), (BZ + 1, BY + 1, BX + 1),
    (17, 33), (BY + 1, BX + 1), (1, 7), (7, 1), (BY, BX), (2, 2), (3, 2 * BX + 3),
    (40,), (1,), (2,), (BX - 1,), (BX,), (BX + 1,), (2 * BX + 3,),
]


def _name(shape, dtype, pattern, niter, kappa, gamma, spacing, option):
    s = "x".join(str(n) for n in shape) + "-%s-%s-n%d-k%g-g%g-o%d" % (dtype, pattern, niter, kappa, gamma, option)
    return s + ("-sp" + "_".join("%g" % v for v in spacing) if spacing else "")


def _cases():
    out = []

    def add(shape, dtype, pattern, seed, niter, kappa, gamma, spacing, option):
        out.append(Case(_name(shape, dtype, pattern, niter, kappa, gamma, spacing, option), tuple(shape), dtype, pattern, seed, niter, float(kappa), float(gamma),
                        None if spacing is None else tuple(float(v) for v in spacing), option))

    for k, shape in enumerate(SHAPES):   # noise on every shape, every option; dtype, niter and the pair rotate
        for option in (1, 2, 3):
            kappa, gamma = PAIRS[(k + option) % 3]
            add(shape, DTYPES[(k + option) % 5], "noise", 100 + k, NITERS[(k + 2 * option) % 5], kappa, gamma, None, option)
    for option in (1, 2, 3):             # every iteration count (both buffer parities) and every dtype on shapes of several bricks
        for niter in NITERS:
            add((2, BY + 1, BX + 4), "float32", "noise", 7, niter, 50.0, 0.1, None, option)
            add((BY + 1, BX + 1), "uint16", "noise", 8, niter, 20.5, 0.25, None, option)
        for dtype in DTYPES:
            add((BZ + 1, 3, 5), dtype, "noise", 9, 2, 50.0, 0.1, None, option)
            add((40,), dtype, "noise", 10, 5, 7.25, 0.05, None, option)
        for shape in ((2, 3, 9), (4, 6), (11,), (1, 1, 1)):   # a constant image comes back unchanged
            add(shape, "int16", "constant", 0, 5, 50.0, 0.25, None, option)
        # non-unit spacing on each axis in turn, then on all
        for sp in ((2.0, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.0, 3.3), (1.5, 0.7, 2.2)):
            add((2, 9, 66), "uint8", "noise", 11, 2, 50.0, 0.1, sp, option)
        for sp in ((0.7, 1.0), (1.0, 1.9), (0.7, 1.9)):
            add((17, 33), "int16", "noise", 12, 5, 20.5, 0.25, sp, option)
        add((40,), "float64", "noise", 13, 8, 7.25, 0.05, (2.5,), option)
    # option 3: a step higher than kappa_s, whose two sides may not mix (flat sides: unchanged; noisy sides: each on its own), along
    # every axis; a ramp whose |d| equals kappa_s exactly
    for axis, shape in ((0, (BZ + 2, 3, 5)), (1, (2, BY + 2, 5)), (2, (2, 3, BX + 6)), (0, (12, 7)), (1, (3, BX + 2)), (0, (2 * BX + 3,))):
        add(shape, "uint8", "step%d" % axis, 0, 5, 50.0, 0.25, None, 3)
        add(shape, "uint8", "noisy_step%d" % axis, 14, 5, 50.0, 0.25, None, 3)
    for shape in ((2, BY + 1, BX + 1), (9, 70), (BX + 3,)):
        for dtype in ("int16", "float32"):
            add(shape, dtype, "ramp", 0, 2, KAPPA_RAMP, 0.1, None, 3)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


def image(case):
    """the input of a case, in its dtype"""
    rng = np.random.default_rng(case.seed)
    shape, dt = case.shape, np.dtype(case.dtype)
    if case.pattern == "noise":
        if dt == np.float64:
            return rng.normal(100.0, 40.0, shape) + 1.0 / 3.0          # values float32 cannot hold
        if dt == np.float32:
            return rng.normal(100.0, 40.0, shape).astype(np.float32)
        if dt == np.int16:
            return rng.integers(-120, 121, shape).astype(dt)
        return rng.integers(0, 256, shape).astype(dt)
    if case.pattern == "constant":
        return np.full(shape, 37, dtype=dt)
    if case.pattern.startswith("step") or case.pattern.startswith("noisy_step"):
        axis = int(case.pattern[-1])
        idx = np.indices(shape)[axis]
        a = np.where(idx < shape[axis] // 2, 10, 200)
        if case.pattern.startswith("noisy"):
            a = a + rng.integers(-4, 5, shape)
        return a.astype(dt)
    if case.pattern == "ramp":
        return (3 * np.indices(shape).sum(axis=0)).astype(dt)          # d = 3 = kappa_s along every axis
    raise ValueError(case.pattern)


def exp_f64_rounded(x):
    """option 1's exponential: exp in float64, rounded once (mgc_ad_exp)"""
    return np.exp(x.astype(np.float64)).astype(np.float32)


def statement(img, niter, kappa, gamma, spacing, option):
    """The definition, voxel by voxel with shifted slices, every operation a float32 operation rounded on its own."""
    u = np.array(img, dtype=np.float32)
    n = u.ndim
    k, ks, g = np.float32(float(kappa)), np.float32(float(kappa) * 2 ** 0.5), np.float32(float(gamma))
    s = [np.float32(float(v)) for v in (spacing if spacing is not None else (1.0,) * n)]
    one, half, zero = np.float32(1), np.float32(0.5), np.float32(0)
    with np.errstate(all="ignore"):
        for _ in range(niter):
            m = []
            for i in range(n):
                lo = tuple(slice(None, -1) if j == i else slice(None) for j in range(n))   # p with p_i < N_i - 1
                hi = tuple(slice(1, None) if j == i else slice(None) for j in range(n))    # p + e_i there; also: p with p_i >= 1
                d = np.zeros_like(u)
                d[lo] = u[hi] - u[lo]
                q = d / (ks if option == 3 else k)
                qq = q * q
                if option == 1:
                    c = exp_f64_rounded(-qq) / s[i]
                elif option == 2:
                    c = (one / (one + qq)) / s[i]
                else:
                    t = one - qq
                    c = np.where(np.abs(d) <= ks, (half * (t * t)) / s[i], zero)
                phi = c * d
                mi = phi.copy()
                mi[hi] = phi[hi] - phi[lo]
                assert mi.dtype == np.float32
                m.append(mi)
            acc = m[0]
            for mi in m[1:]:
                acc = acc + mi
            u = u + g * acc
    assert u.dtype == np.float32
    return u


def error_measure(a, gold):
    """e = max|a - golden| / ptp(golden); a golden image without a range must be met exactly"""
    diff = float(np.max(np.abs(a.astype(np.float64) - gold.astype(np.float64)))) if gold.size else 0.0
    ptp = float(np.ptp(gold.astype(np.float64)))
    if ptp == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / ptp


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

_golden = None


def golden(name):
    """the reference's output of a case (read once, shared, not to be written to)"""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        _golden = {k: z[k] for k in z.files}
        for a in _golden.values():
            a.setflags(write=False)
    return _golden[name]


def check(got, case, what=""):
    """``got`` against the golden output of ``case``: == for options 2 and 3, the bound for option 1"""
    gold = golden(case.name)
    assert got.dtype == np.float32 and got.shape == gold.shape, (what, case.name, got.dtype, got.shape)
    if case.option == 1:
        e = error_measure(got, gold)
        assert e <= E1_BOUND, (what, case.name, e, E1_BOUND)
    else:
        assert np.array_equal(got, gold), (what, case.name, int((got != gold).sum()), error_measure(got, gold))
