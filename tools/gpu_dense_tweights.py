"""What a regional term of the caller's own costs when it reaches the tile solver as whole arrays, and what a list edit of it costs
(profiles/README).  One JSON line per (part, size); nothing is gated on a time: the file is the record.

  calls    per mgc_add_tweights call (two calls, float32 arrays, on a fresh handle): host-API time and the library's own split of it
           (upload, check, accumulate: a host clock around stretches that end in a stream synchronise; accumulate includes the
           pass over the share plane that sums the flow constant), the bytes the merge kernel moves and its bytes/s next to a
           plain device-to-device copy of as many bytes (torch, HIP events, a process of its own, the same run).
  config3  the config-3-shaped volume (synthetic.sphere + synthetic.regional, 26-neighbourhood) built and solved twice: with
           regional_probability_map, and with the same term as dense t-links -- p * alpha and (1 - p) * alpha evaluated on the
           host in the map's dtype, through regional_precomputed.  Labels SHA-256 and flow must be equal; build_ms, solve_ms,
           launch counts and device_bytes of both are recorded (the schedule choices keyed on the probability map do not apply
           to the dense handle).
  edit     on the dense config-3 handle, 2 warm-up + 20 timed rounds, warm and cold alternating, each from the solved state A:
             warm:  edit_tweights(stroke ids, background-leaning weights) + maxflow() + labels(out=labels of A)
             cold:  _clear_tweights() + _add_tweights(the edited arrays) + _build() + maxflow() + labels()
           median (min - max) of the host-API time of a round and of its device parts; labels and flow of the two must agree.
  stroke   the marker-stroke round of tools/gpu_stroke_edit.py (config3, leak_fix: the same stroke as background markers) in the
           same run: the yardstick the list edit should land near.

  python tools/gpu_dense_tweights.py [--sizes 256 512] [--parts calls config3 edit stroke] [--repeats 20] [--warmup 2] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from medpy_amd import graphcut, synthetic  # noqa: E402
from medpy_amd.graphcut.graph import VoxelGraph  # noqa: E402


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def device_copy_gbs(nbytes_moved):
    """a plain device copy that moves as many bytes, in a process of its own (tools/gpu_dense_nweights.py --copy-bytes), or None"""
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_dense_nweights.py"), "--copy-bytes", str(nbytes_moved)],
                           capture_output=True, text=True, timeout=120)
        return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    except Exception:  # noqa: BLE001
        return None


def dense_terms(reg):
    """the regional probability map as source / sink weights, in the map's dtype (energy_voxel.regional_probability_map)"""
    p, alpha = reg["prob"], reg["alpha"]
    return p * alpha, (1 - p) * alpha


def solved(g):
    t0 = time.perf_counter()
    flow = g.maxflow()
    api_ms = (time.perf_counter() - t0) * 1e3
    st = g.stats()
    return {"flow": flow, "labels_sha256": sha(g.labels()), "maxflow_api_ms": round(api_ms, 3), "build_ms": round(st["build_ms"], 3),
            "solve_ms": round(st["solve_ms"], 3), "device_bytes": int(st["device_bytes"]), "global_relabels": int(st["global_relabels"]),
            "phases": int(st["phases"]), "launches": {k: v for k, v in g.launch_counts().items() if v}}


def part_calls(n, out):
    shape = (n, n, n)
    src, snk = dense_terms(synthetic.regional(shape))
    nvox = n ** 3
    # the merge kernel reads both arrays and reads and writes both planes of the store
    moved = 2 * nvox * src.dtype.itemsize + 4 * nvox * 8
    g = VoxelGraph(shape)
    calls = []
    for _ in range(2):
        t0 = time.perf_counter()
        g._add_tweights(src, snk)
        api_ms = (time.perf_counter() - t0) * 1e3
        note = dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))
        note["api_ms"] = round(api_ms, 3)
        note["merge_bytes"] = moved
        if note.get("accumulate_ms"):   # (merge + the pass that sums the flow constant; the first call also clears the new store)
            note["accumulate_gbs"] = round((moved + nvox * 8) / note["accumulate_ms"] / 1e6, 1)
        calls.append(note)
    rec = {"part": "calls", "size": n, "voxels": nvox, "dtype": src.dtype.name, "add_tweights_calls": calls,
           "device_bytes": int(g.stats()["device_bytes"]), "info": g.tweight_edit_info()}
    g.close()
    copy = device_copy_gbs(moved + nvox * 8)
    if copy:
        rec["device_copy_same_bytes"] = copy
    emit(rec, out)


def config3_graph(s, reg, dense):
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False), connectivity=26)
    if dense:
        kw.update(regional_term=graphcut.energy_voxel.regional_precomputed, regional_term_args=dense_terms(reg))
    else:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    t0 = time.perf_counter()
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)
    return g, (time.perf_counter() - t0) * 1e3


def part_config3(n, out):
    shape = (n, n, n)
    s, reg = synthetic.sphere(shape), synthetic.regional(shape)
    rec = {"part": "config3", "size": n}
    for name, dense in (("probability_map", False), ("dense_tlinks", True)):
        g, api_ms = config3_graph(s, reg, dense)
        rec[name] = dict(solved(g), graph_from_voxels_api_ms=round(api_ms, 3), store_held=g.tweight_edit_info()["store_held"])
        g.close()
    rec["labels_equal"] = rec["dense_tlinks"]["labels_sha256"] == rec["probability_map"]["labels_sha256"]
    rec["flow_equal"] = rec["dense_tlinks"]["flow"] == rec["probability_map"]["flow"]
    rec["flow_rel_diff"] = abs(rec["dense_tlinks"]["flow"] - rec["probability_map"]["flow"]) / max(abs(rec["probability_map"]["flow"]), 1e-300)
    emit(rec, out)
    return rec["labels_equal"]


def part_edit(n, repeats, warmup, out):
    from gpu_stroke_edit import stroke
    shape = (n, n, n)
    s, reg = synthetic.sphere(shape), synthetic.regional(shape)
    src_a, snk_a = dense_terms(reg)
    ids = np.flatnonzero(stroke(shape, 0.15, 0.25))   # (the leak_fix stroke of tools/gpu_stroke_edit.py: inside the ball)
    w_src, w_snk = 0.0, 100.0 * reg["alpha"]          # background-leaning, as a re-scored patch would be
    src_b, snk_b = src_a.copy(), snk_a.copy()
    src_b.ravel()[ids] = w_src
    snk_b.ravel()[ids] = w_snk
    g, _ = config3_graph(s, reg, True)
    g.maxflow()
    labels_a = g.labels().copy()
    old = (src_a.ravel()[ids].astype(np.float64), snk_a.ravel()[ids].astype(np.float64))
    rows = []
    for rep in range(warmup + repeats):
        row = {}
        for path in ("warm", "cold"):
            if path == "warm":   # back to A: the old values by list (a warm solve of its own, untimed)
                g.edit_tweights(ids, *old)
            else:
                g._clear_tweights()
                g._add_tweights(src_a, snk_a)
                g._build()
            g.maxflow()
            lab = None
            prev = labels_a.copy()
            t0 = time.perf_counter()
            if path == "warm":
                g.edit_tweights(ids, w_src, w_snk)
                ta = time.perf_counter()
                flow = g.maxflow()
                tb = time.perf_counter()
                lab = g.labels(out=prev)
            else:
                g._clear_tweights()
                g._add_tweights(src_b, snk_b)
                g._build()
                ta = time.perf_counter()
                flow = g.maxflow()
                tb = time.perf_counter()
                lab = g.labels()
            t1 = time.perf_counter()
            st = g.stats()
            row[path + "_api_ms"] = 1e3 * (t1 - t0)
            row[path + "_api_edit_ms"], row[path + "_api_maxflow_ms"], row[path + "_api_read_ms"] = 1e3 * (ta - t0), 1e3 * (tb - ta), 1e3 * (t1 - tb)
            row[path + "_solve_ms"] = st["solve_ms"]
            row[path + ("_update_ms" if path == "warm" else "_build_ms")] = st["update_ms"] if path == "warm" else st["build_ms"]
            row[path + "_sha"] = sha(lab)
            row[path + "_flow"] = flow
            if path == "warm":
                row["warm_delta_ms"] = st["delta_ms"]
                row["flipped"] = int(g.changed_labels().size)
        if rep >= warmup:
            rows.append(row)
    info = g.tweight_edit_info()
    g.close()
    res = {"part": "edit", "config": "config3 as dense t-links", "size": n, "repeats": repeats, "warmup": warmup, "ids_sent": int(ids.size),
           "labels_flipped": rows[0]["flipped"], **{k: summary([r[k] for r in rows]) for k in rows[0] if k.endswith("_ms")},
           "labels_equal": all(r["warm_sha"] == r["cold_sha"] for r in rows) and len({r["warm_sha"] for r in rows}) == 1,
           "flow_rel_diff_max": max(abs(r["warm_flow"] - r["cold_flow"]) / max(abs(r["cold_flow"]), 1e-300) for r in rows),
           "label_sha256_16": rows[0]["warm_sha"], "info": info}
    res["warm_over_cold_api"] = round(res["warm_api_ms"]["median"] / res["cold_api_ms"]["median"], 4)
    emit(res, out)
    return res["labels_equal"]


def part_stroke(n, repeats, warmup, out):
    import gpu_stroke_edit
    res = gpu_stroke_edit.run("config3", n, "leak_fix", repeats, warmup, None)
    emit({"part": "stroke", "size": n, "marker_stroke_round": res}, out)
    return res["labels_equal"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--parts", nargs="+", default=["calls", "config3", "edit", "stroke"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for n in a.sizes:
        if "calls" in a.parts:
            part_calls(n, a.out)
        if "config3" in a.parts:
            ok = part_config3(n, a.out) and ok
        if "edit" in a.parts:
            ok = part_edit(n, a.repeats, a.warmup, a.out) and ok
        if "stroke" in a.parts:
            ok = part_stroke(n, a.repeats, a.warmup, a.out) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
