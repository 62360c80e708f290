"""What the source-side cut and the ambiguity set of a solved volume cost next to the solve (mgc_cut_sets; profiles/README).

For every case one handle is built and solved; then, repeat by repeat:
  counts:   cut_is_unique()                  the flood, the read-out and the cut value on the device; 72 bytes come down
  volumes:  source_side() + ambiguous()      the same twice more, each with one byte per voxel through the staged copy
Host-API times come from a host clock around calls that end in a device synchronise; ``device_ms`` is the library's own note of the
call (everything up to the last kernel, the looks at the list length included).  One JSON line per case with median / min / max over
the repeats, the solve's own time (mgc_get_stats) next to them, the passes, tile visits, tiles seeded and skipped of the flood, the
three counts, and the capacity of the cut around the source side next to the flow.  ``--oracle`` cases are small floating-point
volumes that are also cut by the BK oracle: its counts at tol = 0 go next to the device's (they need not agree: DESIGN 13).  Nothing
is gated on a time: the file is the record.

  python tools/gpu_cut_sets.py [--cases headline:256 headline:512 config3:512] [--oracle sphere:48 hard:40] [--repeats 10] [--warmup 2] [--out FILE]

cases: headline = synthetic.sphere, 6-neighbourhood, exponential term, markers only (bench.py's flagship); config3 = sphere +
synthetic.regional, 26-neighbourhood (BASELINE config 3).
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut, synthetic  # noqa: E402


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def graph(s, reg, conn):
    kw = dict(boundary_term=graphcut.energy_voxel.boundary_difference_exponential, boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)


def note_ms(g):
    return dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))


def forget(g):
    g.__dict__["_cut_sets_cache"] = {}


def run(case, n, repeats, warmup, oracle=False):
    shape = (n, n, n)
    s = getattr(synthetic, "sphere" if case in ("headline", "config3") else case)(shape)
    reg = synthetic.regional(shape) if case == "config3" else None
    conn = 26 if case == "config3" else None
    g = graph(s, reg, conn)
    t0 = time.perf_counter()
    flow = g.maxflow()
    solve_api_ms = (time.perf_counter() - t0) * 1e3
    st = g.stats()
    bytes_before = st["device_bytes"]
    counts_ms, device_ms, volumes_ms, download_ms = [], [], [], []
    for r in range(warmup + repeats):
        forget(g)
        t0 = time.perf_counter()
        g.cut_is_unique()
        t1 = time.perf_counter()
        note = note_ms(g)
        forget(g)
        t2 = time.perf_counter()
        fs = g.source_side()
        down = note_ms(g).get("download_ms", 0.0)
        amb = g.ambiguous()
        t3 = time.perf_counter()
        down += note_ms(g).get("download_ms", 0.0)
        if r >= warmup:
            counts_ms.append((t1 - t0) * 1e3)
            device_ms.append(note.get("device_ms", float("nan")))
            volumes_ms.append((t3 - t2) * 1e3)
            download_ms.append(down)
    info = g.cut_sets_info()
    labels = g.labels()
    row = {"case": case, "shape": list(shape), "connectivity": conn or 6, "repeats": repeats,
           "solve_ms": round(st["solve_ms"], 4), "solve_api_ms_first": round(solve_api_ms, 3),
           "cut_sets_device_ms": summary(device_ms), "cut_sets_api_ms_counts_only": summary(counts_ms),
           "cut_sets_api_ms_both_volumes": summary(volumes_ms), "download_ms_both_volumes": summary(download_ms),
           "flow": flow, "source_cut": info["source_cut"], "source_cut_rel_diff": abs(info["source_cut"] - flow) / abs(flow) if flow else 0.0,
           "device_bytes_before": bytes_before, "device_bytes_after": g.stats()["device_bytes"],
           "from_source_within_labels": bool(not (fs & ~labels).any()), "ambiguous_within_labels": bool(not (amb & ~labels).any()),
           "fg_markers_from_source": bool(fs[s["fg"]].all())}
    row.update({k: info[k] for k in ("from_source", "to_sink", "ambiguous", "flood_passes", "tile_visits", "tiles_seeded", "tiles_skipped")})
    row["tiles"] = st["ntiles"]
    if oracle:
        from oracle import cutcheck, pipeline
        cut = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"])
        o_fs, o_ts, o_amb = cutcheck.ambiguity(cut.graph, tol=0.0)
        row["oracle_tol0"] = {"from_source": int(o_fs.sum()), "to_sink": int(o_ts.sum()), "ambiguous": int(o_amb.sum()), "flow": cut.flow,
                              "labels_differ": int((labels.ravel() != cut.labels.ravel()).sum())}
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["headline:256", "headline:512", "config3:512"])
    ap.add_argument("--oracle", nargs="*", default=["sphere:48", "hard:40"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_sets.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        for spec, oracle in [(c, False) for c in a.cases] + [(c, True) for c in a.oracle]:
            case, n = spec.split(":")
            row = run(case, int(n), a.repeats, a.warmup, oracle)
            print(json.dumps(row))
            f.write(json.dumps(row) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
