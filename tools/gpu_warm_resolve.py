"""Warm re-solve after marker / regional-term edits against a cold build of the same inputs (profiles/README).

For every (configuration, edit) one handle is built and solved with the inputs A of the configuration; then, repeat by repeat,
alternating warm and cold on the same device:
  warm:  update_markers / update_regional_term to the edited inputs B, maxflow, labels      (then back to A, untimed)
  cold:  graph_from_voxels(B), maxflow, labels                                                 (a fresh handle, closed after)
Device times come from the library's own HIP events (mgc_get_stats: update_ms, build_ms, solve_ms, relabel_ms, discharge_ms),
host-API times from a host clock around calls that end in a device synchronise (labels() copies the volume back).  The label
SHA-256 of warm and cold must agree.  One JSON line per (configuration, edit) with median / min / max over the repeats.

  python tools/gpu_warm_resolve.py [--sizes 256 512] [--configs headline config3] [--edits ...] [--repeats 5] [--out FILE]

configurations: headline = synthetic.sphere, 6-neighbourhood, markers only (bench.py's flagship); config3 = synthetic.sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3).  edits: leak_fix (background stroke inside the ball), fg_outside
(foreground stroke outside it), face_removed (the z = 0 face of the background markers taken away), identical (a no-op update),
new_alpha (regional configurations: alpha 0.5 -> 0.7), new_map (regional: another seed of the map).
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

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E (spec)


def stroke(shape, lo, hi):
    """voxels on the ray from the centre along the last axis at distances [lo * n, hi * n), two or three voxels wide across it"""
    n = min(shape)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    m = np.ones(shape, dtype=bool)
    for k, (g, s) in enumerate(zip(grids, shape)):
        c = (s - 1) / 2.0
        m = m & (((g - c) >= lo * n) & ((g - c) < hi * n) if k == len(shape) - 1 else np.abs(g - c) <= 1)
    return m


def inputs(config, n):
    s = synthetic.sphere((n, n, n))
    reg = synthetic.regional((n, n, n)) if config == "config3" else None
    return s, reg, (26 if config == "config3" else None)


def edited(edit, s, reg):
    """(fg, bg, reg) of the edit"""
    fg, bg = s["fg"], s["bg"]
    if edit == "leak_fix":
        return fg, bg | stroke(fg.shape, 0.15, 0.25), reg
    if edit == "fg_outside":
        return fg | stroke(fg.shape, 0.35, 0.45), bg, reg
    if edit == "face_removed":
        nf = bg.copy()
        nf[0] = False
        return fg, nf, reg
    if edit == "identical":
        return fg, bg, reg
    if edit == "new_alpha":
        return fg, bg, dict(prob=reg["prob"], alpha=0.7)
    if edit == "new_map":
        return fg, bg, synthetic.regional(fg.shape, seed=2)
    raise ValueError(edit)


def graph(fg, bg, s, reg, conn):
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(fg, bg, **kw)


def update(g, to, now):
    """warm update of g from the inputs `now` to `to` (fg, bg, reg): the regional term if it changed, the markers if they changed
    (or if nothing did: the no-op update)"""
    (fg, bg, reg), (fg0, bg0, reg0) = to, now
    new_reg = reg is not None and (reg["alpha"] != reg0["alpha"] or reg["prob"] is not reg0["prob"])
    if new_reg:
        g.update_regional_term(reg["prob"], reg["alpha"])
    if fg is not fg0 or bg is not bg0 or not new_reg:
        g.update_markers(fg, bg)


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run(config, n, edit, repeats, out):
    s, reg_a, conn = inputs(config, n)
    fg_b, bg_b, reg_b = edited(edit, s, reg_a)
    w = graph(s["fg"], s["bg"], s, reg_a, conn)
    w.maxflow()
    rows = []
    for rep in range(repeats + 1):  # repeat 0: warm-up of every shape and path, not reported
        update(w, (s["fg"], s["bg"], reg_a), (fg_b, bg_b, reg_b))  # back to A (a warm solve of its own, untimed)
        w.maxflow()
        t0 = time.perf_counter()
        update(w, (fg_b, bg_b, reg_b), (s["fg"], s["bg"], reg_a))
        wflow = w.maxflow()
        wlab = w.labels()
        t1 = time.perf_counter()
        ws = w.stats()
        t2 = time.perf_counter()
        c = graph(fg_b, bg_b, s, reg_b, conn)
        cflow = c.maxflow()
        clab = c.labels()
        t3 = time.perf_counter()
        cs = c.stats()
        row = {"warm_update_ms": ws["update_ms"], "warm_solve_ms": ws["solve_ms"], "warm_relabel_ms": ws["relabel_ms"],
               "warm_discharge_ms": ws["discharge_ms"], "warm_phases": ws["phases"], "warm_global_relabels": ws["global_relabels"],
               "warm_device_ms": ws["update_ms"] + ws["solve_ms"], "cold_build_ms": cs["build_ms"], "cold_solve_ms": cs["solve_ms"],
               "cold_relabel_ms": cs["relabel_ms"], "cold_discharge_ms": cs["discharge_ms"], "cold_phases": cs["phases"],
               "cold_global_relabels": cs["global_relabels"], "cold_device_ms": cs["build_ms"] + cs["solve_ms"],
               "warm_api_ms": 1e3 * (t1 - t0), "cold_api_ms": 1e3 * (t3 - t2),
               "warm_sha": sha(wlab), "cold_sha": sha(clab), "flow_equal": wflow == cflow}
        c.close()
        if rep:
            rows.append(row)
    w.close()
    keys = [k for k in rows[0] if k.endswith("_ms") or k.endswith("_phases") or k.endswith("_relabels")]
    res = {"config": config, "n": n, "edit": edit, "repeats": repeats, **{k: summary([r[k] for r in rows]) for k in keys}}
    res["warm_over_cold_device"] = round(res["warm_device_ms"]["median"] / res["cold_device_ms"]["median"], 3)
    res["warm_over_cold_api"] = round(res["warm_api_ms"]["median"] / res["cold_api_ms"]["median"], 3)
    res["labels_equal"] = all(r["warm_sha"] == r["cold_sha"] for r in rows)
    res["flow_equal"] = all(r["flow_equal"] for r in rows)
    res["label_sha256_16"] = rows[0]["warm_sha"]
    # the least the update kernel has to stream: marker bytes + excess everywhere (+ the map; + tr0 / sink everywhere in the
    # full neighbourhood, where they are not kept per tile) -- over HBM peak, a floor for the update_ms (which includes its sum)
    per_vox = 2 + 8 + (4 if reg_b is not None else 0) + (16 if conn == 26 else 0)
    res["update_floor_bytes_per_voxel"] = per_vox
    res["update_floor_ms"] = round(1e3 * per_vox * n ** 3 / HBM_PEAK, 4)
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
    ap.add_argument("--edits", nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for config in a.configs:
        edits = a.edits or ["leak_fix", "fg_outside", "face_removed", "identical", "new_alpha", "new_map"]
        if config != "config3":
            edits = [e for e in edits if e not in ("new_alpha", "new_map")]  # (no regional term to edit)
        for n in a.sizes:
            if config == "config3" and n < 512 and 512 in a.sizes:
                continue  # config 3 is defined at 512^3
            for edit in edits:
                r = run(config, n, edit, a.repeats, a.out)
                ok = ok and r["labels_equal"] and r["flow_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
