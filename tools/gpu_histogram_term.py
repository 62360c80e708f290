"""What the histogram regional term costs when it is fitted on the device, next to the path that existed before it (DESIGN 14;
profiles/README).  Nothing is gated on a time: the file is the record.

Two JSON lines per volume and size (part kernels, part round).  Volumes: synthetic.ct (uint16, one bin per value) and
synthetic.sphere (float32, 256 bins), built through the public interface (regional_histogram + boundary_difference_exponential on the same image: no feature image goes up).  Per volume:

  hist     marker_histograms(): host clock around the call (it ends in a stream synchronise), 2 warm-up + 10 timed, median
  update   update_tweights_binned of alternating tables: the library's own split from its note (check, expand, flow constant,
           fold), medians; the bytes the expand moves (image read, t-link plane read, both planes written) as GB/s next to a plain
           device copy of as many bytes in the same run (a process of its own)
  round    the stroke round, binned and dense alternating on one handle, each from the solved state A, 2 warm-up + 10 timed:
             binned: edit_markers(fg=stroke) + marker_histograms() + histogram_tables + update_tweights_binned + maxflow()
                     + labels(out=labels of A)        (what refit_regional_histogram does, with the tables rounded to float32)
             dense:  edit_markers(fg=stroke) + host take of the two tables over the bins (float32 arrays) + update_tweights_dense
                     + maxflow() + labels(out=labels of A)
           both from the same float32-rounded tables, so labels and flow must be identical in every round (asserted).

Every volume runs in a child process under its own time limit; the first failure ends the run.

  python tools/gpu_histogram_term.py [--sizes 256 512] [--volumes ct sphere] [--repeats 10] [--warmup 2] [--out FILE]
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

LAM, EPS = 0.05, 0.5
BINS = {"ct": None, "sphere": 256}


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def note_ms(g):
    return dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))


def rounded_tables(fg_hist, bg_hist):
    """the tables of the term, rounded to float32 and widened again: what both paths of a round are fed"""
    from medpy_amd.graphcut import histogram_tables
    s, k = histogram_tables(fg_hist, bg_hist, LAM, EPS)
    return s.astype(np.float32).astype(np.float64), k.astype(np.float32).astype(np.float64)


def run(volume, n, repeats, warmup, out):
    from gpu_dense_tweights import device_copy_gbs
    from gpu_stroke_edit import stroke
    from medpy_amd import graphcut, synthetic
    from medpy_amd.graphcut import energy_voxel, histogram_bins
    shape = (n, n, n)
    nvox = n ** 3
    s = getattr(synthetic, volume)(shape)
    img = s["image"]
    t0 = time.perf_counter()
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], regional_term=energy_voxel.regional_histogram, regional_term_args=(img, BINS[volume], LAM, EPS),
                                   boundary_term=getattr(energy_voxel, "boundary_" + s["term"]), boundary_term_args=(img, s["sigma"], False))
    build_api_ms = (time.perf_counter() - t0) * 1e3
    nbins, lo, width = g._binning
    rec = {"volume": volume, "size": n, "voxels": nvox, "dtype": img.dtype.name, "nbins": nbins, "lam": LAM, "eps": EPS,
           "graph_from_voxels_api_ms": round(build_api_ms, 3), "info": g.tweight_edit_info()}
    flow_a = g.maxflow()
    st = g.stats()
    rec["first_cut"] = {"flow": flow_a, "build_ms": round(st["build_ms"], 3), "solve_ms": round(st["solve_ms"], 3), "device_bytes": int(st["device_bytes"])}
    labels_a = g.labels().copy()
    # -- hist
    xs = []
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        fg_a, bg_a = g.marker_histograms()
        if rep >= warmup:
            xs.append((time.perf_counter() - t0) * 1e3)
    rec["marker_histograms_ms"] = summary(xs)
    rec["marker_histogram_info"] = g.marker_histogram_info()
    # -- the two states: A (the markers as built) and B (a foreground stroke outside the object)
    ids = np.flatnonzero(stroke(shape, 0.35, 0.45))
    tables_a = rounded_tables(fg_a, bg_a)
    g.edit_markers(fg=ids)
    fg_b, bg_b = g.marker_histograms()
    tables_b = rounded_tables(fg_b, bg_b)
    g.edit_markers(erase=ids)
    # -- update: the library's split, alternating tables
    rows = []
    for rep in range(warmup + repeats):
        g.update_tweights_binned(*(tables_b if rep % 2 == 0 else tables_a))
        if rep >= warmup:
            rows.append(note_ms(g))
    rec["update_tweights_binned_ms"] = {k: summary([r[k] for r in rows]) for k in rows[0]}
    moved = nvox * (img.dtype.itemsize + 8 + 16)   # image read, t-link plane read (for the count of changed voxels), both planes written
    rec["expand_bytes"] = moved
    rec["expand_gbs"] = round(moved / rec["update_tweights_binned_ms"]["expand_ms"]["median"] / 1e6, 1)
    copy = device_copy_gbs(moved)
    if copy:
        rec["device_copy_same_bytes"] = copy
    # -- round: binned and dense alternating, each from the solved state A
    bins = histogram_bins(img, nbins, lo, width)   # (the dense path's per-voxel bins: computed once, as a caller of that path would keep them)

    def to_a():
        g.edit_markers(erase=ids)
        g.update_tweights_binned(*tables_a)
        g.maxflow()
    emit(dict(rec, part="kernels"), out)   # (what is measured so far is on file before the rounds assert anything)
    g.update_tweights_binned(*tables_a)
    g.maxflow()
    labels_a = g.labels().copy()   # (the cut of state A as the rounds reach it)
    rows = []
    for rep in range(warmup + repeats):
        row = {}
        for path in ("binned", "dense"):
            prev = labels_a.copy()
            t0 = time.perf_counter()
            g.edit_markers(fg=ids)
            ta = time.perf_counter()
            if path == "binned":
                g.update_tweights_binned(*rounded_tables(*g.marker_histograms()))
            else:
                src, snk = tables_b[0].astype(np.float32)[bins], tables_b[1].astype(np.float32)[bins]
                row["dense_take_ms"] = 1e3 * (time.perf_counter() - ta)
                g.update_tweights_dense(src, snk)
            tb = time.perf_counter()
            flow = g.maxflow()
            tc = time.perf_counter()
            lab = g.labels(out=prev)
            t1 = time.perf_counter()
            row[path + "_api_ms"] = 1e3 * (t1 - t0)
            row[path + "_edit_markers_ms"], row[path + "_term_ms"] = 1e3 * (ta - t0), 1e3 * (tb - ta)
            row[path + "_maxflow_ms"], row[path + "_labels_ms"] = 1e3 * (tc - tb), 1e3 * (t1 - tc)
            row[path + "_solve_ms"] = g.stats()["solve_ms"]
            row[path + "_sha"], row[path + "_flow"], row["changed"] = sha(lab), flow, int((lab != labels_a).sum())
            to_a()
        assert row["binned_sha"] == row["dense_sha"] and row["binned_flow"] == row["dense_flow"], row   # identical labels and flow in every round
        if rep >= warmup:
            rows.append(row)
    res = {k: summary([r[k] for r in rows]) for k in rows[0] if k.endswith("_ms")}
    res.update(stroke_voxels=int(ids.size), labels_changed=rows[0]["changed"], labels_and_flow_identical=True, label_sha256_16=rows[0]["binned_sha"],
               flow=rows[0]["binned_flow"], repeats=repeats, warmup=warmup)
    res["dense_over_binned_api"] = round(res["dense_api_ms"]["median"] / res["binned_api_ms"]["median"], 3)
    g.close()
    emit({"part": "round", "volume": volume, "size": n, "dtype": img.dtype.name, "nbins": nbins, "round": res}, out)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--volumes", nargs="+", default=["ct", "sphere"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="time limit of one volume's child process, seconds")
    ap.add_argument("--child", nargs=2, metavar=("VOLUME", "SIZE"), help="(internal) run one volume in this process")
    a = ap.parse_args()
    if a.child:
        return run(a.child[0], int(a.child[1]), a.repeats, a.warmup, a.out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in a.sizes:
        for volume in a.volumes:   # a fresh child process per volume, under its own time limit; the first failure ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--child", volume, str(n), "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
            if a.out:
                cmd += ["--out", a.out]
            rc = subprocess.run(cmd, timeout=a.limit).returncode
            if rc != 0:
                sys.exit("gpu_histogram_term: %s %d^3 ended with status %d: stopping" % (volume, n, rc))


if __name__ == "__main__":
    main()
