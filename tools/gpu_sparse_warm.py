"""One round of an interactive edit on the sparse-graph solver -- t-links changed, graph cut again, result seen -- warm against
cold ("The sparse-graph solver"; profiles/README).

For every (workload, edit) one graph is built and solved with its inputs A; then, repeat by repeat, alternating on that handle
and each time from the solved state A (restored and solved, untimed):
  warm:  the edit + maxflow + labels(out=labels of A)     msg_update_tweights folds the changed t-links into the resident preflow,
                                                          msg_maxflow skips the CSR build, the flipped labels come back as a list
  cold:  set_param("warm", 0), the same calls             the t-links are stored, msg_maxflow sorts the arcs and builds the CSR
                                                          again and solves from zero flow, all labels come back
Host-API times come from a host clock around calls that end in a device synchronise; device times are the library's own HIP events
(msg_get_stats: build_ms + solve_ms; the fold kernel, one thread per changed node, is in neither).  The label SHA-256 and the flow
of the two modes must agree in every repeat.  One JSON line per case with median / min / max over the repeats.

  python tools/gpu_sparse_warm.py [--workloads regions graphdouble] [--edits ...] [--n 256] [--repeats 12] [--warmup 2] [--out FILE]

workloads: regions = the n^3 sphere cut into ragged super-voxels of block 4 (tools/bench_labels.py: ~270 k regions at 256^3),
boundary_stawiaski, edited through RegionGraph.edit_markers by voxel ids; graphdouble = a random GraphDouble graph of 200 000 nodes
and ~1.2 M edges with float capacities, edited through update_tweights.  edits: bg_inside (a background stroke inside the
object), fg_outside (a foreground stroke outside it), identical (nothing changes).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut, synthetic  # noqa: E402
from medpy_amd.graphcut import energy_label as el  # noqa: E402
from tools.gpu_stroke_edit import stroke  # noqa: E402


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


class Regions(object):
    """graph_from_labels on the super-voxel partition; an edit is a stroke of voxels"""

    def __init__(self, n):
        shape = (n, n, n)
        s = synthetic.sphere(shape)
        idx = np.indices(shape)
        coarse = tuple((idx[d] + (idx[(d + 1) % 3] // 9)) // 4 for d in range(3))
        flat = np.ravel_multi_index(coarse, [int(c.max()) + 1 for c in coarse])
        _, lab = np.unique(flat, return_inverse=True)
        self.lab = (lab.reshape(shape) + 1).astype(np.int32)
        del idx, coarse, flat
        grad = np.abs(np.gradient(s["image"].astype(np.float32))[0]).astype(np.float32)
        self.fg, self.bg = s["fg"], s["bg"]
        self.name = "%d^3 volume, %d super-voxel regions, boundary_stawiaski" % (n, int(self.lab.max()))
        self.g = graphcut.graph_from_labels(self.lab, self.fg, self.bg, boundary_term=el.boundary_stawiaski, boundary_term_args=grad)
        self.strokes = {"bg_inside": dict(bg=np.flatnonzero(stroke(shape, 0.15, 0.25))), "fg_outside": dict(fg=np.flatnonzero(stroke(shape, 0.35, 0.45))),
                        "identical": dict()}

    def restore(self):
        self.g.update_markers(self.fg, self.bg)

    def edit(self, name):
        self.g.edit_markers(**self.strokes[name])


class RandomGraph(object):
    """GraphDouble on a random graph; an edit replaces the t-links of 50 nodes"""

    def __init__(self, nodes=200000, edges=1200000):
        rng = np.random.default_rng(7)
        i, j = rng.integers(0, nodes, edges), rng.integers(0, nodes, edges)
        keep = i != j
        i, j = i[keep], j[keep]
        self.tr = np.where(rng.random(nodes) < 0.3, rng.normal(0, 2, nodes), 0.0)
        self.name = "random GraphDouble graph, %d nodes, %d edges, float capacities" % (nodes, i.size)
        self.g = graphcut.GraphDouble(nodes, i.size)
        self.g._add_edges(i, j, rng.random(i.size) + 1e-3, rng.random(i.size) + 1e-3)
        self.g.update_tweights(np.arange(nodes), self.tr)
        self.g.maxflow()
        side = self.g.labels()
        self.lists = {"bg_inside": (np.flatnonzero(side)[:50], -50.0), "fg_outside": (np.flatnonzero(~side)[:50], 50.0), "identical": (np.zeros(0, np.int64), 0.0)}

    def restore(self):
        ids = np.concatenate([v[0] for v in self.lists.values()])
        self.g.update_tweights(ids, self.tr[ids])

    def edit(self, name):
        ids, value = self.lists[name]
        self.g.update_tweights(ids, np.full(ids.size, value))


def run(w, edit, repeats, warmup, out):
    g = w.g
    g.set_param("warm", 1)
    w.restore()
    g.maxflow()
    labels_a = g.labels().copy()
    rows = []
    for rep in range(warmup + repeats):
        row = {}
        for mode in ("warm", "cold"):
            g.set_param("warm", 1)
            w.restore()   # back to A (a solve of its own, untimed)
            g.maxflow()
            g.set_param("warm", 1 if mode == "warm" else 0)
            prev = labels_a.copy()
            t0 = time.perf_counter()
            w.edit(edit)
            ta = time.perf_counter()
            flow = g.maxflow()
            tb = time.perf_counter()
            lab = g.labels(out=prev) if mode == "warm" else g.labels()
            t1 = time.perf_counter()
            st, info = g.stats(), g.warm_info()
            assert info["skipped_build"] == (mode == "warm"), (mode, info)
            row[mode + "_api_ms"] = 1e3 * (t1 - t0)
            row[mode + "_api_edit_ms"], row[mode + "_api_maxflow_ms"], row[mode + "_api_read_ms"] = 1e3 * (ta - t0), 1e3 * (tb - ta), 1e3 * (t1 - tb)
            row[mode + "_device_ms"] = st["build_ms"] + st["solve_ms"]
            row[mode + "_build_ms"], row[mode + "_solve_ms"] = st["build_ms"], st["solve_ms"]
            row[mode + "_rounds"] = st["rounds"]
            row[mode + "_sha"] = sha(lab)
            row[mode + "_flow"] = flow
            if mode == "warm":
                row["flipped"] = int(g.changed_nodes().size)
        if rep >= warmup:
            rows.append(row)
    st = g.stats()
    res = {"workload": w.name, "edit": edit, "nodes": st["nodes"], "arcs": st["arcs"], "repeats": repeats, "warmup": warmup,
           **{k: summary([r[k] for r in rows]) for k in rows[0] if k.endswith("_ms")},
           "warm_rounds": rows[0]["warm_rounds"], "cold_rounds": rows[0]["cold_rounds"], "labels_flipped": rows[0]["flipped"],
           "labels_equal": all(r["warm_sha"] == r["cold_sha"] for r in rows) and len({r["warm_sha"] for r in rows}) == 1,
           "flow_equal": all(r["warm_flow"] == r["cold_flow"] for r in rows),
           "label_sha256_16": rows[0]["warm_sha"], "flow": rows[0]["warm_flow"]}
    res["warm_over_cold_api"] = round(res["warm_api_ms"]["median"] / res["cold_api_ms"]["median"], 3)
    res["warm_over_cold_device"] = round(res["warm_device_ms"]["median"] / res["cold_device_ms"]["median"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["regions", "graphdouble"])
    ap.add_argument("--edits", nargs="+", default=["bg_inside", "fg_outside", "identical"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for name in a.workloads:
        w = Regions(a.n) if name == "regions" else RandomGraph()
        for edit in a.edits:
            r = run(w, edit, a.repeats, a.warmup, a.out)
            ok = ok and r["labels_equal"] and r["flow_equal"]
        w.g.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
