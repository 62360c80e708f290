"""What the seeded watershed and the minima of its markers cost on the device (mgc_watershed_image, mgc_local_minima_image;
DESIGN 21; profiles/README).

For every size N (N^3 voxels) and --mindist: a smoothed-noise gradient map (uint16: Gaussian-smoothed noise, the sum of its absolute
forward differences, scaled to 0..4095), markers from medpy_amd.filter.minima_markers, then 3 warm-up calls and 7 timed calls of
mgc_watershed_image: the median, minimum and maximum of flood_ms, parent_ms and resolve_ms (HIP events on the call's stream, read
from the note the call leaves in mgc_last_error) and of upload_ms / download_ms / the whole call (host clock), next to the rounds,
tile visits, sweeps, capped visits, reached voxels and jump rounds of out8, the number of markers, and the ms of minima_markers and
of mgc_local_minima_image alone.
  host:  (--host N, once) the literal Meyer flood of tests/watershed_cases.py (pure Python, a heap) on this machine's host at N^3 with
         the same kind of map and markers -- for scale only: it is the statement's reference point, not an optimised host watershed.
Nothing is gated on a time: the file is the record.  Every size runs in a child process of its own under a time limit; the first
that fails or runs out of time ends the run.

  python tools/gpu_watershed.py [--sizes 256 512] [--mindist 2 8] [--limit 500] [--host 128] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS = 3, 7
OUT8 = ("seeds", "rounds", "tile_visits", "sweeps", "capped_visits", "reached", "jump_rounds")


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def note_ms(note):
    return {k: float(v) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", note)}


def gradient_map(n):
    """smoothed noise -> the sum of the absolute forward differences along the three axes, as uint16 in 0..4095"""
    import numpy as np
    import scipy.ndimage as ndi
    rng = np.random.default_rng(7)
    s = ndi.gaussian_filter(rng.normal(0.0, 1.0, (n, n, n)).astype(np.float32), 2.0)
    g = np.zeros_like(s)
    for a in range(3):
        d = np.abs(np.diff(s, axis=a, append=np.take(s, [-1], axis=a)))
        g += d
    return np.round(g * (4095.0 / float(g.max()))).astype(np.uint16)


def run(n, mindists):
    import numpy as np
    from medpy_amd import _lib
    from medpy_amd import filter as flt
    lib = _lib.load()
    image = gradient_map(n)
    shp = (C.c_int64 * 3)(n, n, n)
    labels = np.empty((n, n, n), np.int32)
    out8 = np.zeros(8, np.int64)
    mask8 = np.empty((n, n, n), np.uint8)
    for md in mindists:
        row = {"kind": "gpu", "shape": [n, n, n], "dtype": "uint16", "mindist": md, "warmup": WARMUP, "repeats": REPEATS}
        t0 = time.perf_counter()
        _lib.check(None, lib.mgc_local_minima_image(0, 3, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], md, _lib.ptr(mask8), None))
        _lib.check(None, lib.mgc_local_minima_image(0, 3, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], md, _lib.ptr(mask8), None))
        row["local_minima_second_call"] = note_ms(lib.mgc_last_error(None).decode())
        t0 = time.perf_counter()
        markers = flt.minima_markers(image, md)
        row["minima_markers_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        row["markers"] = int(markers.max())
        ms = {k: [] for k in ("upload_ms", "flood_ms", "parent_ms", "resolve_ms", "download_ms", "call_ms")}
        for r in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            _lib.check(None, lib.mgc_watershed_image(0, 3, shp, _lib.ptr(image), _lib.DTYPE_IDS[image.dtype], _lib.ptr(markers), None, _lib.ptr(labels), _lib.ptr(out8)))
            call = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                note = note_ms(lib.mgc_last_error(None).decode())
                for k in ms:
                    ms[k].append(call if k == "call_ms" else note[k])
        row.update({k: summary(v) for k, v in ms.items()})
        row.update(zip(OUT8, out8.tolist()))
        row["regions"] = int(np.unique(labels).size)
        row["flood_us_per_round"] = round(1e3 * row["flood_ms"]["median"] / max(1, row["rounds"]), 2)
        print(json.dumps(row), flush=True)


def host(n):
    import numpy as np
    import scipy.ndimage as ndi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import watershed_cases as wc
    image = gradient_map(n)
    markers = ndi.label(wc.minima_statement(image, 2))[0].astype(np.int32)
    t0 = time.perf_counter()
    wc.meyer_flood(image, markers)
    return {"kind": "host_meyer_flood", "what": "tests/watershed_cases.py:meyer_flood (pure Python and heapq, ours; for scale only)", "shape": [n, n, n], "mindist": 2,
            "markers": int(markers.max()), "ms": round((time.perf_counter() - t0) * 1e3, 1), "numpy": np.__version__}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--mindist", nargs="*", type=int, default=[2, 8])
    ap.add_argument("--limit", type=int, default=500, help="seconds per size")
    ap.add_argument("--host", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        run(int(args.child), args.mindist)
        return 0
    lines, rc = [], 0
    for n in args.sizes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--mindist"] + [str(m) for m in args.mindist], capture_output=True, text=True,
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("size %s ran out of time: the run ends here" % n, file=sys.stderr)
            rc = 1
            break
        if r.returncode != 0:
            print("size %s failed (%d): the run ends here\n%s" % (n, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            rc = 1
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.host and not rc:
        lines.append(json.dumps(host(args.host)))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    print(text, end="")
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
