"""What the connected components of a cut and the cleaning by them cost next to the solve (mgc_components / mgc_clean_labels, DESIGN 16;
profiles/README).

For every case one handle is built and solved; then, repeat by repeat, through the public methods:
  counts:    components(ids=False)                                         the labelling and the table; no volume comes down
  ids:       components()                                                  the same plus the int32 id volume
  changed:   clean_labels(seeded=True, fill_holes=True, changed_only=True) two labellings, the rule on the host, the list of changed ids
  volume:    clean_labels(seeded=True, fill_holes=True)                    the same with the cleaned volume down
Host-API times from a host clock around calls that end in a device synchronise; medians, minima and maxima over the repeats, the
solve's own time (mgc_get_stats) next to them and, for scale, scipy.ndimage.label on the downloaded labels on this machine's host
(once).  ``bernoulli`` cases label a caller's random plane of density 0.31 on an unbuilt handle: the adversarial case, K in the
millions; K, unions and the longest parent walk are reported.  Nothing is gated on a time: the file is the record.

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.

  python tools/gpu_components.py [--cases headline:256 headline:512 config3:512 bernoulli:256] [--repeats 10] [--warmup 2] [--limit 240] [--out FILE]

cases: headline = synthetic.sphere, 6-neighbourhood, exponential term, markers only (bench.py's flagship); config3 = sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3); bernoulli = a random plane, face neighbourhood.
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


def run(case, n, repeats, warmup):
    import numpy as np
    from scipy import ndimage
    from medpy_amd import graphcut, synthetic
    shape = (n, n, n)
    row = {"case": case, "shape": list(shape), "repeats": repeats}
    if case == "bernoulli":
        plane = (np.random.default_rng(31).random(shape) < 0.31).astype(np.uint8)
        g = graphcut.VoxelGraph(shape)
        row["connectivity"] = 6
        row["components_counts_only_api_ms"], res = timed(repeats, warmup, lambda: g.components(plane, ids=False))
        row["components_with_ids_api_ms"], res = timed(repeats, warmup, lambda: g.components(plane))
        row["info"] = res.info
        t0 = time.perf_counter()
        _, k = ndimage.label(plane)
        row["scipy_label_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["scipy_components"] = int(k)
        g.close()
        return row
    s = synthetic.sphere(shape)
    conn = 26 if case == "config3" else None
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    if case == "config3":
        reg = synthetic.regional(shape)
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]), connectivity=26)
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)
    t0 = time.perf_counter()
    g.maxflow()
    row.update(connectivity=conn or 6, solve_api_ms_first=round((time.perf_counter() - t0) * 1e3, 3), solve_ms=round(g.stats()["solve_ms"], 4))
    bytes_before = g.stats()["device_bytes"]
    row["components_counts_only_api_ms"], res = timed(repeats, warmup, lambda: g.components(ids=False))
    row["info"] = res.info
    row["components_with_ids_api_ms"], res = timed(repeats, warmup, lambda: g.components())
    rule = dict(seeded=True, fill_holes=True)
    row["clean_changed_only_api_ms"], changed = timed(repeats, warmup, lambda: g.clean_labels(changed_only=True, **rule))
    row["clean_info"] = g.clean_info()
    row["clean_volume_api_ms"], cleaned = timed(repeats, warmup, lambda: g.clean_labels(**rule))
    row["device_bytes_before"], row["device_bytes_after"] = bytes_before, g.stats()["device_bytes"]
    labels = g.labels()
    t0 = time.perf_counter()
    ids, k = ndimage.label(labels, structure=ndimage.generate_binary_structure(3, 3 if conn else 1))
    row["scipy_label_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    row["ids_equal_scipy"] = bool(np.array_equal(res.ids, ids)) and int(k) == res.info["components"]
    row["changed_list_is_the_difference"] = bool(np.array_equal(changed, np.flatnonzero(cleaned.ravel() != labels.ravel())))
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["headline:256", "headline:512", "config3:512", "bernoulli:256"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.jsonl"))
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
