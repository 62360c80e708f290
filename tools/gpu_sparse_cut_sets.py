"""What the cut sets of a graph on the sparse-graph solver cost (msg_cut_sets / msg_cut_sets_tol; profiles/README).

One line per graph goes to profiles/sparse_cut_sets.jsonl, nothing is gated on a time:

  region   graph_from_labels (Stawiaski term) on a synthetic 256^3 volume cut into 4 x 8 x 4 blocks: 131 072 regions
  lattice4 graph_from_voxels on a 32^4 float32 image (1 048 576 nodes, 8 neighbours each)
  hub      the star of tests/sparse_cases.py:hub5000 with 500 000 leaves: ONE row of 500 000 arcs, 10^6 arcs in all
  path     a chain of 100 000 nodes, excess at one end and no sink: the solve is over at its first count, the forward flood has
           to walk the whole chain, one node a pass -- the worst case of a flood driven by the topology alone

Per graph: the solve (msg_get_stats), then counts-only calls without a tolerance and at ULP64, repeat by repeat; the library's note of
the call splits its device time into scale, open, forward flood (seeding included), backward flood (seeding included) and read-out
(both cut values included).  The stamps are events on the stream, so the floods' host round trips (one look every 8 passes) are inside
forward_ms / backward_ms; wall_ms is the host clock around the whole call.  Medians, minima, maxima.

  python tools/gpu_sparse_cut_sets.py [--graphs region lattice4 hub path] [--repeats 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut  # noqa: E402
from medpy_amd.graphcut import ULP64, GraphDouble  # noqa: E402

PHASES = ("device_ms", "scale_ms", "open_ms", "forward_ms", "backward_ms", "readout_ms")
COUNTS = ("from_source", "to_sink", "ambiguous", "forward_passes", "forward_seeds", "backward_passes", "backward_seeds", "arcs_closed", "tlinks_closed")


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def region(side=256):
    rng = np.random.default_rng(256)
    shape = (side, side, side)
    z, y, x = np.indices(shape, dtype=np.int32)
    nb = (side // 4, side // 8, side // 4)
    lab = ((z // 4) * (nb[1] * nb[2]) + (y // 8) * nb[2] + (x // 4) + 1).astype(np.int32)
    del z, y, x
    grad = rng.integers(0, 8, shape).astype(np.float32)
    c = side // 2
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    fg[c - 8:c + 8, c - 8:c + 8, c - 8:c + 8] = True
    bg[0], bg[-1], bg[:, 0], bg[:, -1], bg[:, :, 0], bg[:, :, -1] = True, True, True, True, True, True
    return graphcut.graph_from_labels(lab, fg, bg, boundary_term=graphcut.energy_label.boundary_stawiaski, boundary_term_args=grad)


def lattice4(side=32):
    rng = np.random.default_rng(32)
    shape = (side,) * 4
    img = rng.random(shape).astype(np.float32)
    fg, bg = np.zeros(shape, bool), np.zeros(shape, bool)
    c = side // 2
    fg[c - 2:c + 2, c - 2:c + 2, c - 2:c + 2, c - 2:c + 2] = True
    bg[0], bg[-1] = True, True
    return graphcut.graph_from_voxels(fg, bg, boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(img, 0.25, False))


def hub(m=500000):
    rng = np.random.default_rng(5000)
    g = GraphDouble(m + 1, m)
    g._add_edges(np.zeros(m, np.int64), np.arange(1, m + 1), rng.integers(1, 5, m).astype(float), rng.integers(0, 5, m).astype(float))
    g._set_tweights_merged(np.concatenate([[0.0], rng.integers(-3, 4, m).astype(float)]), 0.0)
    return g


def path(n=100000):
    rng = np.random.default_rng(100000)
    k = np.arange(n - 1)
    g = GraphDouble(n, n - 1)
    g._add_edges(k, k + 1, rng.integers(2, 9, n - 1).astype(float), rng.integers(2, 9, n - 1).astype(float))
    tr = np.zeros(n)
    tr[0] = 10.0
    g._set_tweights_merged(tr, 0.0)
    return g


GRAPHS = {"region": region, "lattice4": lattice4, "hub": hub, "path": path}


def note_ms(g):
    return dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))


def measure(name, repeats, warmup):
    g = GRAPHS[name]()
    t0 = time.perf_counter()
    flow = g.maxflow()
    solve_wall = (time.perf_counter() - t0) * 1e3
    st = g.stats()
    row = {"kind": "timing", "graph": name, "nodes": st["nodes"], "arcs": st["arcs"], "repeats": repeats, "flow": flow, "build_ms": round(st["build_ms"], 4),
           "solve_ms": round(st["solve_ms"], 4), "maxflow_wall_ms": round(solve_wall, 4), "solve_rounds": st["rounds"], "solve_relabel_passes": st["relabel_passes"]}
    for key, tol in (("cut_sets", None), ("cut_sets_tol_ulp64", ULP64)):
        ms, wall = {k: [] for k in PHASES}, []
        for r in range(warmup + repeats):
            g.__dict__["_cut_sets_cache"] = {}
            t0 = time.perf_counter()
            g.cut_sets_unique(tol)
            w = (time.perf_counter() - t0) * 1e3
            note = note_ms(g)
            if r >= warmup:
                wall.append(w)
                for k in PHASES:
                    ms[k].append(note.get(k, float("nan")))
        g.cut_sets_unique(tol)
        info = g.__dict__["_cut_sets_cache"][("info", None if tol is None else float(tol))]
        row[key] = dict({k: summary(v) for k, v in ms.items()}, wall_ms=summary(wall), **{k: info[k] for k in COUNTS},
                        source_cut=info["source_cut"], sink_cut=info["sink_cut"], scale_max=info["scale_max"])
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="*", default=["region", "lattice4", "hub", "path"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_cut_sets.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        for name in a.graphs:
            row = measure(name, a.repeats, a.warmup)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
