"""What the cut sets at a rounding tolerance cost and what they say (mgc_cut_sets_tol; profiles/README).

Three kinds of line go to profiles/cut_sets_tol.jsonl, nothing is gated on a time or on a count:

  timing   headline 256^3 / 512^3 and config 3: one handle built and solved, then counts-only calls at ULP64, repeat by repeat.  The
           library's note of the call splits its device time into scale, open, forward flood (seeding included), backward flood
           (seeding included) and read-out (both cut values included); each phase ends on a drained stream, so the five add up to
           device_ms less the allocations.  Medians, minima, maxima; mgc_cut_sets' own device_ms and the solve next to them.
  counts   the integer-valued volumes ct (uint16) and ties at 96^3: from_source / to_sink / ambiguous, arcs and t-links closed, at tol 0,
           ULP64 and 1e-12.
  b0       the reference's notebook image with --boundary diff_div (tests/golden/reference_b0.npz): how many voxels differ from the
           labels the reference wrote, and how many of those lie in the device's OWN ambiguous(ULP64) -- the parity statement of DESIGN 4
           made without the oracle's BFS.

  python tools/gpu_cut_sets_tol.py [--timing headline:256 headline:512 config3:512] [--counts ct:96 ties:96] [--no-b0] [--repeats 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut, synthetic  # noqa: E402
from medpy_amd.graphcut import ULP64  # noqa: E402

PHASES = ("device_ms", "scale_ms", "open_ms", "forward_ms", "backward_ms", "readout_ms")
COUNTS = ("from_source", "to_sink", "ambiguous", "arcs_closed", "tlinks_closed", "forward_passes", "forward_visits", "forward_seeded", "backward_passes",
          "backward_visits", "backward_seeded", "tiles_skipped")


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def graph(s, reg=None, conn=None, term=None):
    term = term or graphcut.energy_voxel.boundary_difference_exponential
    kw = dict(boundary_term=term, boundary_term_args=(s["image"], s["sigma"], False))
    if reg is not None:
        kw.update(regional_term=graphcut.energy_voxel.regional_probability_map, regional_term_args=(reg["prob"], reg["alpha"]))
    if conn:
        kw["connectivity"] = conn
    return graphcut.graph_from_voxels(s["fg"], s["bg"], **kw)


def note_ms(g):
    return dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))


def forget(g):
    g.__dict__["_cut_sets_cache"] = {}


def timing(case, n, repeats, warmup):
    shape = (n, n, n)
    s = synthetic.sphere(shape)
    reg = synthetic.regional(shape) if case == "config3" else None
    conn = 26 if case == "config3" else None
    g = graph(s, reg, conn)
    flow = g.maxflow()
    st = g.stats()
    ms = {k: [] for k in PHASES}
    plain = []
    for r in range(warmup + repeats):
        forget(g)
        g.cut_is_unique()
        p = note_ms(g).get("device_ms", float("nan"))
        g.cut_is_unique(ULP64)
        note = note_ms(g)
        if r >= warmup:
            plain.append(p)
            for k in PHASES:
                ms[k].append(note.get(k, float("nan")))
    info, info0 = g.cut_sets_info(ULP64), g.cut_sets_info(0.0)
    row = {"kind": "timing", "case": case, "shape": list(shape), "connectivity": conn or 6, "repeats": repeats, "tol": ULP64, "tiles": st["ntiles"],
           "solve_ms": round(st["solve_ms"], 4), "cut_sets_device_ms": summary(plain), "flow": flow, "source_cut": info["source_cut"], "sink_cut": info["sink_cut"],
           "scale_max": info["scale_max"], "device_bytes_before": st["device_bytes"], "device_bytes_after": g.stats()["device_bytes"],
           "counts_at_tol0": [info0["from_source"], info0["to_sink"], info0["ambiguous"]]}
    row.update({"tol_" + k: summary(v) for k, v in ms.items()})
    row.update({k: info[k] for k in COUNTS})
    g.close()
    return row


def counts(case, n):
    shape = (n, n, n)
    s = getattr(synthetic, case)(shape)
    g = graph(s)
    flow = g.maxflow()
    row = {"kind": "counts", "case": case, "image_dtype": str(s["image"].dtype), "shape": list(shape), "flow": flow, "labels_foreground": int(g.labels().sum())}
    plain = g.cut_sets_info()
    row["mgc_cut_sets"] = [plain["from_source"], plain["to_sink"], plain["ambiguous"]]
    for name, tol in (("tol_0", 0.0), ("tol_ulp64", ULP64), ("tol_1e-12", 1e-12)):
        info = g.cut_sets_info(tol)
        row[name] = {k: info[k] for k in ("from_source", "to_sink", "ambiguous", "arcs_closed", "tlinks_closed", "source_cut", "sink_cut")}
    g.close()
    return row


def b0():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_b0.npz"))
    img = z["image"].astype(np.dtype(str(z["image_dtype"])))
    markers = z["markers"]
    sigma = float(z["difference_division/sigma"])
    ref = np.unpackbits(z["difference_division/labels"])[: img.size].reshape(img.shape).astype(bool)
    g = graph({"image": img, "sigma": sigma, "fg": markers == 1, "bg": markers == 2}, term=graphcut.energy_voxel.boundary_difference_division)
    flow = g.maxflow()
    differ = g.labels() != ref
    row = {"kind": "b0", "case": "b0 diff_div", "shape": list(img.shape), "sigma": sigma, "flow": flow, "differ_from_reference_labels": int(differ.sum())}
    for name, tol in (("tol_0", 0.0), ("tol_ulp64", ULP64), ("tol_1e-12", 1e-12)):
        amb, info = g.ambiguous(tol), g.cut_sets_info(tol)
        row[name] = {"from_source": info["from_source"], "to_sink": info["to_sink"], "ambiguous": info["ambiguous"], "arcs_closed": info["arcs_closed"],
                     "tlinks_closed": info["tlinks_closed"], "differing_voxels_in_ambiguous": int((differ & amb).sum())}
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", nargs="*", default=["headline:256", "headline:512", "config3:512"])
    ap.add_argument("--counts", nargs="*", default=["ct:96", "ties:96"])
    ap.add_argument("--no-b0", action="store_true")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_sets_tol.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        def emit(row):
            print(json.dumps(row))
            f.write(json.dumps(row) + "\n")
            f.flush()
        for spec in a.counts:
            case, n = spec.split(":")
            emit(counts(case, int(n)))
        if not a.no_b0:
            emit(b0())
        for spec in a.timing:
            case, n = spec.split(":")
            emit(timing(case, int(n), a.repeats, a.warmup))


if __name__ == "__main__":
    main()
