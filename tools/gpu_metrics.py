"""What scoring a cut against a ground truth costs on the device (mgc_distance_transform / mgc_surface_distances / mgc_overlap_counts,
medpy_amd.metric.binary; profiles/README).

For every case the headline graph (synthetic.sphere, 6-neighbourhood, exponential term, markers only: bench.py's flagship) is built and
solved; the ground truth is a copy of its labels shifted by (3, 2, 1).  Then, repeat by repeat, through the public interface:
  distance_transform:   g.distance_transform(squared=True)        the transform of the resident cut, the f64 volume down
  surface_distances:    g.surface_distances(truth)                borders, transform, gathering; the truth up, the list down
  overlap_counts:       g.overlap_counts(truth)
  hd_with_graph:        binary.hd(None, truth, graph=g)           both directions on the solved handle
  hd_without_graph:     binary.hd(labels, truth)                  the same on a handle created for the call and closed: the difference is
                                                                  what creating an ordinary handle (it reserves the solver's state) costs
  create_close:         VoxelGraph(shape).close()                 that cost on its own
Host-API times from a host clock around calls that end in a device synchronise; medians, minima and maxima over the repeats after the
warm-up calls, the solve's own time next to them and, for scale, the same Hausdorff distance by scipy.ndimage on this machine's host
(binary_erosion and distance_transform_edt, once).  Nothing is gated on a time: the file is the record.

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.

  python tools/gpu_metrics.py [--cases headline:256 headline:512] [--repeats 10] [--warmup 2] [--limit 500] [--out FILE]
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


def scipy_hd(a, b):
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(a.ndim, 1)
    ra, rb = a ^ ndimage.binary_erosion(a, structure=st), b ^ ndimage.binary_erosion(b, structure=st)
    return max(ndimage.distance_transform_edt(~rb)[ra].max(), ndimage.distance_transform_edt(~ra)[rb].max()), int(ra.sum()), int(rb.sum())


def run(case, n, repeats, warmup):
    import numpy as np
    from medpy_amd import graphcut, synthetic
    from medpy_amd.metric import binary
    shape = (n, n, n)
    row = {"case": case, "shape": list(shape), "repeats": repeats, "warmup": warmup}
    s = synthetic.sphere(shape)
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                   boundary_term_args=(s["image"], s["sigma"], False))
    t0 = time.perf_counter()
    g.maxflow()
    row.update(solve_api_ms_first=round((time.perf_counter() - t0) * 1e3, 3), solve_ms=round(g.stats()["solve_ms"], 4))
    labels = np.ascontiguousarray(np.asarray(g.labels()).reshape(shape).astype(bool))
    truth = np.zeros(shape, bool)
    truth[3:, 2:, 1:] = labels[:-3, :-2, :-1]
    bytes_before = g.stats()["device_bytes"]
    row["distance_transform_api_ms"], dt = timed(repeats, warmup, lambda: g.distance_transform(squared=True))
    row["edt_info"] = g.edt_info()
    row["surface_distances_api_ms"], sds = timed(repeats, warmup, lambda: g.surface_distances(truth))
    row["overlap_counts_api_ms"], counts = timed(repeats, warmup, lambda: g.overlap_counts(truth))
    row["hd_with_graph_api_ms"], hd1 = timed(repeats, warmup, lambda: binary.hd(None, truth, graph=g))
    row["device_bytes_before"], row["device_bytes_after"] = bytes_before, g.stats()["device_bytes"]
    row["hd_without_graph_api_ms"], hd2 = timed(repeats, warmup, lambda: binary.hd(labels, truth))
    row["create_close_api_ms"], _ = timed(repeats, warmup, lambda: graphcut.VoxelGraph(shape).close())
    t0 = time.perf_counter()
    ref, na, nb = scipy_hd(labels, truth)
    row["scipy_hd_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    row.update(border_voxels=[int(sds.size), nb], counts=list(counts), hd=float(hd1), hd_equal_without_graph=bool(hd1 == hd2), hd_equal_scipy=bool(hd1 == ref),
               borders_equal_scipy=bool(sds.size == na), voxels_of_the_cut=int(labels.sum()))
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["headline:256", "headline:512"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=500, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        case, n = a.child.split(":")
        print(json.dumps(run(case, int(n), a.repeats, a.warmup)))
        return 0
    with open(a.out, "a") as f:
        for spec in a.cases:
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
