"""One round of an interactive edit -- markers changed, graph cut again, result seen -- through whole masks and through lists
("Edits by list"; profiles/README).

For every (configuration, size, edit) one handle is built and solved with the inputs A of the configuration; then, repeat by
repeat, alternating on that handle and each time from the solved state A (update_markers(A) + maxflow, untimed):
  masks:  update_markers(full masks of B) + maxflow + labels()                       2 volumes up, 1 volume down
  lists:  edit_markers(the ids that differ) + maxflow + labels(out=labels of A)      9 bytes per id up, 8 per flipped label down
Host-API times come from a host clock around calls that end in a device synchronise; device times from the library's own HIP
events (mgc_get_stats: update_ms -- the fold, plus the scatter on the list path --, solve_ms, delta_ms); *_api_edit_ms,
*_api_maxflow_ms and *_api_read_ms split the host-API time of a round by its three calls.  The label SHA-256 and
the flow of the two paths must agree in every repeat.  One JSON line per case with median / min / max over the repeats.

  python tools/gpu_stroke_edit.py [--sizes 256 512] [--configs headline config3] [--edits ...] [--repeats 20] [--warmup 2] [--out FILE]

configurations: headline = synthetic.sphere, 6-neighbourhood, markers only (bench.py's flagship); config3 = synthetic.sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3).  edits: leak_fix (background stroke inside the ball), fg_outside
(foreground stroke outside it), face_removed (the z = 0 face of the background markers erased: a list of a whole plane).
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


def stroke(shape, lo, hi):
    """voxels on the ray from the centre along the last axis at distances [lo * n, hi * n), two or three voxels wide across it"""
    n = min(shape)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    m = np.ones(shape, dtype=bool)
    for k, (g, s) in enumerate(zip(grids, shape)):
        c = (s - 1) / 2.0
        m = m & (((g - c) >= lo * n) & ((g - c) < hi * n) if k == len(shape) - 1 else np.abs(g - c) <= 1)
    return m


def edited(edit, s):
    """(fg, bg) masks of the edit and the same edit as keyword arguments of edit_markers"""
    fg, bg = s["fg"], s["bg"]
    if edit == "leak_fix":
        m = stroke(fg.shape, 0.15, 0.25)
        return fg, bg | m, dict(bg=np.flatnonzero(m))
    if edit == "fg_outside":
        m = stroke(fg.shape, 0.35, 0.45)
        return fg | m, bg, dict(fg=np.flatnonzero(m))
    if edit == "face_removed":
        nf = bg.copy()
        nf[0] = False
        return fg, nf, dict(erase=np.flatnonzero(bg[0]))  # (plane 0: its flat ids are the ids inside the plane)
    raise ValueError(edit)


def graph(fg, bg, s, reg, conn):
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(fg, bg, **kw)


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run(config, n, edit, repeats, warmup, out):
    s = synthetic.sphere((n, n, n))
    reg = synthetic.regional((n, n, n)) if config == "config3" else None
    conn = 26 if config == "config3" else None
    fg_b, bg_b, lists = edited(edit, s)
    ids_sent = int(sum(np.unique(v).size for v in lists.values()))
    g = graph(s["fg"], s["bg"], s, reg, conn)
    g.maxflow()
    labels_a = g.labels().copy()
    bytes_before = g.stats()["device_bytes"]
    rows = []
    for rep in range(warmup + repeats):
        row = {}
        for path in ("masks", "lists"):
            g.update_markers(s["fg"], s["bg"])  # back to A (a warm solve of its own, untimed)
            g.maxflow()
            lab = None  # (the volume read last goes back to the allocator outside the clock)
            prev = labels_a.copy()
            t0 = time.perf_counter()
            if path == "masks":
                g.update_markers(fg_b, bg_b)
                ta = time.perf_counter()
                flow = g.maxflow()
                tb = time.perf_counter()
                lab = g.labels()
            else:
                g.edit_markers(**lists)
                ta = time.perf_counter()
                flow = g.maxflow()
                tb = time.perf_counter()
                lab = g.labels(out=prev)
            t1 = time.perf_counter()
            st = g.stats()
            row[path + "_api_ms"] = 1e3 * (t1 - t0)
            row[path + "_api_edit_ms"], row[path + "_api_maxflow_ms"], row[path + "_api_read_ms"] = 1e3 * (ta - t0), 1e3 * (tb - ta), 1e3 * (t1 - tb)
            row[path + "_update_ms"] = st["update_ms"]
            row[path + "_solve_ms"] = st["solve_ms"]
            row[path + "_sha"] = sha(lab)
            row[path + "_flow"] = flow
            if path == "lists":
                row["lists_delta_ms"] = st["delta_ms"]
                row["flipped"] = int(g.changed_labels().size)
        if rep >= warmup:
            rows.append(row)
    bytes_after = g.stats()["device_bytes"]
    g.close()
    nvox = n ** 3
    flipped = rows[0]["flipped"]
    res = {"config": config, "n": n, "edit": edit, "repeats": repeats, "warmup": warmup,
           **{k: summary([r[k] for r in rows]) for k in rows[0] if k.endswith("_ms")},
           "ids_sent": ids_sent, "labels_flipped": flipped,
           "masks_bytes_up": 2 * nvox, "masks_bytes_down": nvox, "lists_bytes_up": 9 * ids_sent, "lists_bytes_down": 8 * flipped + 8,
           "device_bytes_before_first_list_edit": bytes_before, "device_bytes_after": bytes_after,
           "labels_equal": all(r["masks_sha"] == r["lists_sha"] for r in rows) and len({r["lists_sha"] for r in rows}) == 1,
           "flow_equal": all(r["masks_flow"] == r["lists_flow"] for r in rows),
           "label_sha256_16": rows[0]["lists_sha"]}
    res["lists_over_masks_api"] = round(res["lists_api_ms"]["median"] / res["masks_api_ms"]["median"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--configs", nargs="+", default=["headline", "config3"])
    ap.add_argument("--edits", nargs="+", default=["leak_fix", "fg_outside", "face_removed"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for config in a.configs:
        for n in a.sizes:
            for edit in a.edits:
                r = run(config, n, edit, a.repeats, a.warmup, a.out)
                ok = ok and r["labels_equal"] and r["flow_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
