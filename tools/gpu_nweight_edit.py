"""One round of a local n-link correction -- a barrier or glue drawn on a few hundred arcs, graph cut again, result seen -- warm
through the arc list and cold through the weight arrays ("Edits of n-links by list"; profiles/README).

For every case one handle is built and solved in state A; then, repeat by repeat, alternating:
  warm:  edit_nweights(the stroke's arcs) + maxflow() + labels(out=labels of A)       24 bytes per arc pair cross the ABI, 8 per flipped label come down
         (afterwards, untimed: the same arcs set back to their capacities of A + maxflow())
  cold:  graph_from_voxels over the edited weight arrays + maxflow() + labels()       one array per offset up, 1 volume down
Host-API times come from a host clock around calls that end in a device synchronise; device times from the library's own HIP
events: the note of mgc_edit_nweights (cap0_fill_ms of the first edit, fold_ms, refresh_ms) and mgc_get_stats (solve_ms,
delta_ms; the cold round: build_ms, solve_ms).  The label SHA-256 and the flow of the two rounds must agree in every repeat.
One JSON line per (case, edit) with median / min / max over the repeats, device_bytes before and after the first edit, and what
mgc_get_nweight_edit_info said (first_edit: of the very first edit of the handle, which meets the flow of the first solve; later
rounds meet arcs that an earlier round has emptied).  Nothing is gated on a time: the file is the record.

  python tools/gpu_nweight_edit.py [--cases headline:512 config3:512 precomputed:512] [--edits barrier glue] [--repeats 20] [--warmup 2] [--out FILE]

cases: headline = synthetic.sphere, 6-neighbourhood, exponential term, markers only (bench.py's flagship); config3 = sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3); precomputed = the headline's weights handed over as arrays
(boundary_precomputed): a handle with a dense store.  edits: barrier = a disc of about 200 z-arcs inside the object set to 0
both ways; glue = the same arcs raised x 100.
"""
import argparse
import hashlib
import itertools
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut, synthetic  # noqa: E402


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def offsets(conn):
    if conn != 26:
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]


def boundary_arrays(graph, args):
    """boundary term of the cold round: one symmetric weight array per forward offset, as whole arrays"""
    (arrays,) = args
    for off, w in arrays.items():
        graph.set_nweights_dense(off, w)


def graph(s, reg, conn, arrays=None):
    if arrays is None:
        kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    else:
        kw = dict(boundary_term=boundary_arrays, boundary_term_args=(arrays,))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)


def disc(shape, radius=8):
    """flat ids of the tails of the stroke's z-arcs (p, p + e_z): a disc in the plane a fifth of the way from the centre to the rim"""
    n = shape[0]
    z, c = n // 2 + n // 10, (n - 1) / 2.0
    y, x = np.ogrid[0:shape[1], 0:shape[2]]
    m = (y - c) ** 2 + (x - c) ** 2 <= radius ** 2
    return np.flatnonzero(m) + z * shape[1] * shape[2], z, m


def row_flipped(g):
    return int(g.changed_labels().size)


def note_ms(g):
    return dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))


def run(case, n, edits, repeats, warmup, out):
    shape = (n, n, n)
    s = synthetic.sphere(shape)
    reg = synthetic.regional(shape) if case == "config3" else None
    conn = 26 if case == "config3" else None
    g = graph(s, reg, conn)
    g.maxflow()
    # the weights of state A as arrays (entries whose neighbour lies outside the volume: 0, the library ignores them)
    arrays = {o: np.nan_to_num(g.nweights_offset(o)) for o in offsets(conn)}
    if case == "precomputed":
        g.close()
        g = graph(s, None, None, arrays)
        g.maxflow()
    labels_a = g.labels().copy()
    flow_a = g.maxflow()
    tails, z, m = disc(shape)
    heads = tails + shape[1] * shape[2]
    wz = arrays[(1, 0, 0)]
    old = wz[z][m].copy()
    bytes_before = g.stats()["device_bytes"]
    first = None
    for edit in edits:
        new = np.zeros_like(old) if edit == "barrier" else old * 100.0
        edited = dict(arrays)
        edited[(1, 0, 0)] = wz.copy()
        edited[(1, 0, 0)][z][m] = new
        rows = []
        lab = clab = None
        for rep in range(warmup + repeats):
            row = {}
            lab = clab = None  # (the volumes read last go back to the allocator outside the clock)
            prev = labels_a.copy()
            t0 = time.perf_counter()
            g.edit_nweights(tails, heads, new)
            ta = time.perf_counter()
            note = note_ms(g)
            info = g.nweight_edit_info()
            tn = time.perf_counter()
            flow = g.maxflow()
            tb = time.perf_counter()
            lab = g.labels(out=prev)
            t1 = time.perf_counter()
            st = g.stats()
            if first is None:
                first = {"cap0_fill_ms": note.get("cap0_fill_ms"), "api_ms": round(1e3 * (ta - t0), 3), "device_bytes_after": int(st["device_bytes"]), "edit_info": info,
                         "labels_flipped": row_flipped(g)}
            row["warm_api_ms"] = 1e3 * ((t1 - t0) - (tn - ta))
            row["warm_api_edit_ms"], row["warm_api_maxflow_ms"], row["warm_api_read_ms"] = 1e3 * (ta - t0), 1e3 * (tb - tn), 1e3 * (t1 - tb)
            row["warm_fold_ms"], row["warm_refresh_ms"] = note["fold_ms"], note["refresh_ms"]
            row["warm_solve_ms"], row["warm_delta_ms"] = st["solve_ms"], st["delta_ms"]
            row["warm_sha"], row["warm_flow"], row["flipped"] = sha(lab), flow, int(g.changed_labels().size)
            row["info"] = info
            g.edit_nweights(tails, heads, old)   # back to A (a warm solve of its own, untimed)
            back = g.maxflow()
            row["back_to_a"] = back == flow_a and sha(g.labels(out=lab)) == sha(labels_a)   # (by the delta: no label volume is read or cached)
            t0 = time.perf_counter()
            c = graph(s, reg, conn, edited)
            ta = time.perf_counter()
            cflow = c.maxflow()
            tb = time.perf_counter()
            clab = c.labels()
            t1 = time.perf_counter()
            cst = c.stats()
            row["cold_api_ms"] = 1e3 * (t1 - t0)
            row["cold_api_build_ms"], row["cold_api_maxflow_ms"], row["cold_api_read_ms"] = 1e3 * (ta - t0), 1e3 * (tb - ta), 1e3 * (t1 - tb)
            row["cold_build_ms"], row["cold_solve_ms"] = cst["build_ms"], cst["solve_ms"]
            row["cold_sha"], row["cold_flow"] = sha(clab), cflow
            c.close()
            c = None
            if rep >= warmup:
                rows.append(row)
        res = {"case": case, "n": n, "edit": edit, "repeats": repeats, "warmup": warmup, "arcs": int(tails.size),
               **{k: summary([r[k] for r in rows]) for k in rows[0] if k.endswith("_ms")},
               "labels_flipped": rows[0]["flipped"], "edit_info": rows[0]["info"], "bytes_up": 24 * int(tails.size),
               "bytes_down": 8 * rows[0]["flipped"] + 8, "first_edit": first, "device_bytes_before_first_edit": int(bytes_before),
               "labels_equal": all(r["warm_sha"] == r["cold_sha"] for r in rows) and len({r["warm_sha"] for r in rows}) == 1,
               "flow_equal": all(r["warm_flow"] == r["cold_flow"] for r in rows), "back_to_a": all(r["back_to_a"] for r in rows),
               "label_sha256_16": rows[0]["warm_sha"], "flow": rows[0]["warm_flow"], "flow_a": flow_a}
        res["warm_over_cold_api"] = round(res["warm_api_ms"]["median"] / res["cold_api_ms"]["median"], 4)
        line = json.dumps(res)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")
        yield res
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["headline:512", "config3:512", "precomputed:512"])
    ap.add_argument("--edits", nargs="+", default=["barrier", "glue"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for case in a.cases:
        name, n = case.split(":")
        for r in run(name, int(n), a.edits, a.repeats, a.warmup, a.out):
            ok = ok and r["labels_equal"] and r["flow_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
