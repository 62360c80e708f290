"""What the geodesic distance transform and the regional term on top of it cost on the device (mgc_geodesic_distance,
mgc_add_tweights_geodesic / mgc_update_tweights_geodesic; profiles/README).

For every case a volume of bench.py (the headline sphere volume, or the ct_uint16 volume) is built with its exponential boundary
term and its markers, so that image and markers are resident.  Then:
  transform:  mgc_geodesic_distance from the foreground markers where they lie, nothing brought down (out NULL): face and full
              neighbourhood, gamma 0 and 1 -- rounds, tile visits, sweeps and host-API ms per call; once with the f64 volume
              brought down through the public call
  round:      a cold build + solve with the geodesic term, and the warm refit + solve after a stroke of 200 voxels, next to the same
              round with the histogram term
  scipy:      (--scipy N, once) scipy.sparse.csgraph.dijkstra on this machine's host at N^3 for scale
Host-API times from a host clock around calls that end in a device synchronise; medians, minima and maxima over the repeats after
the warm-up calls.  Nothing is gated on a time: the file is the record.

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.

  python tools/gpu_geodesic.py [--cases sphere:256 ct:256 sphere:512 ct:512] [--repeats 10] [--warmup 2] [--limit 500] [--scipy 128] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(repeats, warmup, call):
    ms, last = [], None
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        last = call()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms), last


def stroke_of(labels, fg, bg, count=200):
    """`count` neighbouring voxels of the background side that hold no marker, along the last axis"""
    import numpy as np
    free = np.flatnonzero(~labels.ravel() & ~bg.ravel() & ~fg.ravel())
    mid = free.size // 2
    return free[mid:mid + count]


def run(case, n, repeats, warmup):
    import numpy as np
    from medpy_amd import _lib, graphcut, synthetic
    from medpy_amd.graphcut import energy_voxel
    shape = (n, n, n)
    row = {"case": case, "shape": list(shape), "repeats": repeats, "warmup": warmup}
    s = (synthetic.sphere if case == "sphere" else synthetic.ct)(shape)
    boundary = dict(boundary_term=energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], **boundary)
    lib = _lib.load()
    out8 = np.zeros(8, np.int64)
    for full in (0, 1):
        for gamma in (0.0, 1.0):
            def call():
                _lib.check(g._h, lib.mgc_geodesic_distance(g._h, None, 1, full, gamma, 1.0, None, None, _lib.ptr(out8)))
            t0 = time.perf_counter()
            call()
            first = (time.perf_counter() - t0) * 1e3
            reps = repeats if first < 2000.0 else max(1, repeats // 5)   # (a call of seconds is not repeated ten times)
            ms, _ = timed(reps, warmup if first < 2000.0 else 0, call)
            row["transform_%s_gamma%g" % ("full" if full else "face", gamma)] = dict(
                api_ms=ms, first_ms=round(first, 3), repeats=reps, **dict(zip(graphcut.VoxelGraph.GEODESIC_INFO_KEYS, out8.tolist())))
    t0 = time.perf_counter()
    d = g.geodesic_distance("fg", 1.0)
    row["public_call_with_download_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    row["finite_max"] = float(d.max())
    del d
    g.close()
    lam = 1.0
    terms = {"geodesic": (energy_voxel.regional_geodesic, (1.0, lam)), "histogram": (energy_voxel.regional_histogram, (s["image"], 64, lam, 0.5))}
    for name, (term, args) in terms.items():
        t0 = time.perf_counter()
        g = graphcut.graph_from_voxels(s["fg"], s["bg"], regional_term=term, regional_term_args=args, **boundary)
        t1 = time.perf_counter()
        note = lib.mgc_last_error(g._h).decode() if name == "geodesic" else ""
        flow = g.maxflow()
        t2 = time.perf_counter()
        labels = np.asarray(g.labels()).reshape(shape).astype(bool)
        stroke = stroke_of(labels, s["fg"], s["bg"])
        t3 = time.perf_counter()
        g.edit_markers(fg=stroke)
        if name == "geodesic":
            g.refit_regional_geodesic()
            note2 = lib.mgc_last_error(g._h).decode()
        else:
            g.refit_regional_histogram()
            note2 = ""
        t4 = time.perf_counter()
        flow2 = g.maxflow()
        t5 = time.perf_counter()
        after = np.asarray(g.labels()).reshape(shape).astype(bool)
        changed = int((after != labels).sum())
        if name == "geodesic":   # (the geodesic refit keeps the label snapshot; the histogram refit drops it)
            assert int(g.changed_labels().size) == changed
        row["round_" + name] = {"cold_build_ms": round((t1 - t0) * 1e3, 3), "cold_solve_api_ms": round((t2 - t1) * 1e3, 3), "flow": flow, "fg_voxels": int(labels.sum()),
                                "stroke": int(stroke.size), "edit_and_refit_ms": round((t4 - t3) * 1e3, 3), "warm_solve_api_ms": round((t5 - t4) * 1e3, 3), "flow_after": flow2,
                                "labels_changed": changed, "solve_ms": round(g.stats()["solve_ms"], 4), "note_build": note, "note_refit": note2}
        g.close()
    return row


def run_scipy(n):
    import numpy as np
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    from medpy_amd import synthetic
    shape = (n, n, n)
    s = synthetic.sphere(shape)
    val = s["image"].astype(np.float64)
    ids = np.arange(val.size).reshape(shape)
    rows, cols, w = [], [], []
    t0 = time.perf_counter()
    for a in range(3):
        for o in (-1, 1):
            src = tuple(slice(max(0, -o), n - max(0, o)) if k == a else slice(None) for k in range(3))
            dst = tuple(slice(max(0, o), n - max(0, -o)) if k == a else slice(None) for k in range(3))
            rows.append(ids[src].ravel())
            cols.append(ids[dst].ravel())
            w.append(1.0 + np.abs(val[src] - val[dst]).ravel())
    m = csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(val.size, val.size))
    t1 = time.perf_counter()
    d = dijkstra(m, indices=np.flatnonzero(s["fg"].ravel()), min_only=True)
    t2 = time.perf_counter()
    return {"case": "scipy_dijkstra_host", "shape": list(shape), "neighbourhood": "face", "gamma": 1.0, "matrix_ms": round((t1 - t0) * 1e3, 1),
            "dijkstra_ms": round((t2 - t1) * 1e3, 1), "finite_max": float(d.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["sphere:256", "ct:256", "sphere:512", "ct:512"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=500, help="seconds a case may take")
    ap.add_argument("--scipy", type=int, default=0, help="edge of the cube scipy's Dijkstra runs on the host, once (0: not run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        case, n = a.child.split(":")
        print(json.dumps(run_scipy(int(n)) if case == "scipy" else run(case, int(n), a.repeats, a.warmup)))
        return 0
    with open(a.out, "a") as f:
        for spec in a.cases + (["scipy:%d" % a.scipy] if a.scipy else []):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", spec, "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            if out.returncode != 0:
                print("case %s ended with status %d: the run stops here\n%s" % (spec, out.returncode, out.stderr[-2000:]), file=sys.stderr)
                return out.returncode
            line = out.stdout.strip().splitlines()[-1]
            print(line)
            f.write(line + "\n")
            f.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
