"""Warm re-solve after a change of the boundary term against a cold build of the new arguments ("The boundary term";
profiles/README).

For every (configuration, edit) one handle is built and solved with the arguments A of the configuration; then, repeat by repeat,
alternating warm and cold on the same device:
  warm:  update_boundary_term to the edited arguments B, maxflow, changed_labels applied to the caller's copy   (then back to A, untimed)
  cold:  graph_from_voxels(B), maxflow, labels                                                                  (a fresh handle, closed after)
Device times come from the library's own HIP events (mgc_get_stats: update_ms = the fold kernel, build_ms, solve_ms, delta_ms),
host-API times from a host clock around calls that end in a device synchronise.  The label SHA-256 and the flow of warm and cold
must agree.  One JSON line per (configuration, edit) with median / min / max over the repeats; fold_ms next to build_ms of a cold
build on the same handle (both evaluate g(.) once per arc pair).

  python tools/gpu_boundary_warm.py [--sizes 256 512] [--configs headline config3] [--edits ...] [--repeats 5] [--out FILE]

configurations: headline = synthetic.sphere, 6-neighbourhood, markers only (bench.py's flagship); config3 = synthetic.sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3, defined at 512^3).  edits: sigma_down (15 -> 10), sigma_up (15 -> 25),
division (difference_exponential -> difference_division), noisy_image (the image replaced by itself plus noise of a tenth of its own).
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

EDITS = ["sigma_down", "sigma_up", "division", "noisy_image"]


def inputs(config, n):
    s = synthetic.sphere((n, n, n))
    reg = synthetic.regional((n, n, n)) if config == "config3" else None
    return s, reg, (26 if config == "config3" else None)


def edited(edit, a):
    """the boundary arguments of the edit: dict(term, image, sigma)"""
    if edit == "sigma_down":
        return dict(a, sigma=10.0)
    if edit == "sigma_up":
        return dict(a, sigma=25.0)
    if edit == "division":
        return dict(a, term="difference_division")
    if edit == "noisy_image":
        rng = np.random.default_rng(7)
        return dict(a, image=(a["image"] + rng.normal(0.0, 1.0, a["image"].shape)).astype(a["image"].dtype))
    raise ValueError(edit)


def term_call(b, image):
    return getattr(graphcut.energy_voxel, "boundary_" + b["term"]), (image, b["sigma"], False)


def graph(s, b, reg, conn):
    fn, args = term_call(b, b["image"])
    kw = dict(boundary_term=fn, boundary_term_args=args)
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)


def update(g, to, now):
    """warm update of g from the arguments `now` to `to`: the image goes up only where it is another one"""
    fn, args = term_call(to, to["image"] if to["image"] is not now["image"] else None)
    g.update_boundary_term(fn, args)


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run(config, n, edit, repeats, out):
    s, reg, conn = inputs(config, n)
    a = dict(term=s["term"], image=s["image"], sigma=s["sigma"])
    b = edited(edit, a)
    w = graph(s, a, reg, conn)
    w.maxflow()
    rows = []
    for rep in range(repeats + 1):  # repeat 0: warm-up of every shape and path, not reported
        update(w, a, b)  # back to A (a warm solve of its own, untimed)
        w.maxflow()
        mine = w.labels().copy()  # the caller's copy of the labels of A
        t0 = time.perf_counter()
        update(w, b, a)
        wflow = w.maxflow()
        w.labels(out=mine)
        t1 = time.perf_counter()
        ws = w.stats()
        info = w.boundary_update_info()
        t2 = time.perf_counter()
        c = graph(s, b, reg, conn)
        cflow = c.maxflow()
        clab = c.labels()
        t3 = time.perf_counter()
        cs = c.stats()
        row = {"fold_ms": ws["update_ms"], "warm_solve_ms": ws["solve_ms"], "warm_relabel_ms": ws["relabel_ms"], "warm_discharge_ms": ws["discharge_ms"],
               "warm_delta_ms": ws["delta_ms"], "warm_phases": ws["phases"], "warm_global_relabels": ws["global_relabels"],
               "warm_device_ms": ws["update_ms"] + ws["solve_ms"] + ws["delta_ms"], "cold_build_ms": cs["build_ms"], "cold_solve_ms": cs["solve_ms"],
               "cold_phases": cs["phases"], "cold_global_relabels": cs["global_relabels"], "cold_device_ms": cs["build_ms"] + cs["solve_ms"],
               "warm_api_ms": 1e3 * (t1 - t0), "cold_api_ms": 1e3 * (t3 - t2),
               "warm_sha": sha(mine), "cold_sha": sha(clab), "flow_equal": wflow == cflow, "info": info}
        c.close()
        if rep:
            rows.append(row)
    # k_build of the arguments A on the handle the fold ran on (a cold rebuild in place)
    w._build()
    build_here = w.stats()["build_ms"]
    w.close()
    keys = [k for k in rows[0] if k.endswith("_ms") or k.endswith("_phases") or k.endswith("_relabels")]
    res = {"config": config, "n": n, "edit": edit, "repeats": repeats, **{k: summary([r[k] for r in rows]) for k in keys}}
    res["build_ms_same_handle"] = round(build_here, 4)
    res["fold_over_build"] = round(res["fold_ms"]["median"] / build_here, 3)
    res["warm_over_cold_device"] = round(res["warm_device_ms"]["median"] / res["cold_device_ms"]["median"], 3)
    res["warm_over_cold_api"] = round(res["warm_api_ms"]["median"] / res["cold_api_ms"]["median"], 3)
    res["labels_equal"] = all(r["warm_sha"] == r["cold_sha"] for r in rows)
    res["flow_equal"] = all(r["flow_equal"] for r in rows)
    res["label_sha256_16"] = rows[0]["warm_sha"]
    res["update_info"] = rows[0]["info"]
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
    ap.add_argument("--edits", nargs="+", default=EDITS)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for config in a.configs:
        for n in a.sizes:
            if config == "config3" and n < 512 and 512 in a.sizes:
                continue  # config 3 is defined at 512^3
            for edit in a.edits:
                r = run(config, n, edit, a.repeats, a.out)
                ok = ok and r["labels_equal"] and r["flow_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
