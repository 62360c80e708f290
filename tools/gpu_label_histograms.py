"""What the histograms over every voxel cost (mgc_label_histograms), next to the only way the parent commit had to the same numbers
on the device, and what a round of the iterated refit costs (profiles/README).  Nothing is gated on a time: the file is
the record.

Two JSON lines per volume and size (part hist, part loop).  Volumes: synthetic.ct (uint16, one bin per value) and synthetic.sphere
(float32, 256 bins), built through the public interface (regional_histogram + boundary_difference_exponential on the same image)
and solved once: the first stroke cut.  Per volume:

  hist   label_histograms() on the solved graph: host clock around the call (it ends in a stream synchronise), 2 warm-up + 10
         timed, median / min / max.  --parent-tree DIR (a checkout of the parent commit with its library built): the baseline is
         marker_histograms() of THAT tree on a handle whose two marker planes are the cut's labels and their complement, in a child
         process of its own that stays open; the timed calls alternate in blocks of five -- new, baseline, new, baseline -- and the
         histograms are asserted equal.  Next to both: a plain device copy of as many bytes as each pass reads.
  loop   iterate_regional_histogram(max_refits=8) from that cut: per refit the time of label_histograms, of histogram_tables, of
         update_tweights_binned with the library's own split from its note (check, expand, flow constant, fold) and of the warm
         maxflow(); the number of refits to the fixed point, and what moved.

Every volume runs in a child process under its own time limit; the first failure ends the run.

  python tools/gpu_label_histograms.py [--sizes 256 512] [--volumes ct sphere] [--repeats 10] [--warmup 2] [--parent-tree DIR] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

LAM, EPS = 0.05, 0.5
BINS = {"ct": None, "sphere": 256}


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(call, count):
    xs, res = [], None
    for _ in range(count):
        t0 = time.perf_counter()
        res = call()
        xs.append((time.perf_counter() - t0) * 1e3)
    return xs, res


def baseline(a):
    """(child of a volume's process, on the parent tree) marker_histograms() under the labels and their complement: warm up, then
    one block of timed calls per line read from the parent process; a JSON line per block"""
    volume, n, labels_path = a.baseline[0], int(a.baseline[1]), a.baseline[2]
    nbins, lo, width = a.baseline[3].split(":")[1:]   # "b:<nbins>:<lo>:<width>", the two floats in hexadecimal (exact)
    nbins, lo, width = int(nbins), float.fromhex(lo), float.fromhex(width)
    from medpy_amd import synthetic
    from medpy_amd.graphcut import VoxelGraph
    shape = (n, n, n)
    img = getattr(synthetic, volume)(shape)["image"]
    labels = np.load(labels_path)
    g = VoxelGraph(shape)
    g._set_feature_image(img)
    g._set_markers(labels, ~labels)
    timed(lambda: g.marker_histograms(nbins, lo, width), a.warmup)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        count = int(line)
        if count <= 0:
            break
        xs, (fg, bg) = timed(lambda: g.marker_histograms(nbins, lo, width), count)
        print(json.dumps({"ms": xs, "fg": fg.tolist(), "bg": bg.tolist(), "info": g.marker_histogram_info()}), flush=True)
    g.close()


def run(volume, n, a):
    from gpu_dense_tweights import device_copy_gbs
    from medpy_amd import graphcut, synthetic
    from medpy_amd.graphcut import energy_voxel
    from medpy_amd.graphcut import graph as graph_module
    shape = (n, n, n)
    nvox = n ** 3
    s = getattr(synthetic, volume)(shape)
    img = s["image"]
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], regional_term=energy_voxel.regional_histogram, regional_term_args=(img, BINS[volume], LAM, EPS),
                                   boundary_term=getattr(energy_voxel, "boundary_" + s["term"]), boundary_term_args=(img, s["sigma"], False))
    nbins, lo, width = g._binning
    flow = g.maxflow()
    st = g.stats()
    labels = g.labels().copy()
    rec = {"part": "hist", "volume": volume, "size": n, "voxels": nvox, "dtype": img.dtype.name, "nbins": nbins, "lam": LAM, "eps": EPS, "repeats": a.repeats,
           "warmup": a.warmup, "first_cut": {"flow": flow, "solve_ms": round(st["solve_ms"], 3), "fg_voxels": int(labels.sum()), "device_bytes": int(st["device_bytes"])}}
    # -- hist: new and baseline alternating in blocks
    half = max(1, a.repeats // 2)
    blocks = [half, a.repeats - half] if a.repeats > half else [half]
    base = None
    tmp = tempfile.mkdtemp()
    if a.parent_tree:
        np.save(os.path.join(tmp, "labels.npy"), labels)
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent_tree))
        env.pop("MEDPY_HIP_LIB", None)
        base = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--warmup", str(a.warmup), "--baseline", volume, str(n), os.path.join(tmp, "labels.npy"),
                                 "b:%d:%s:%s" % (nbins, float(lo).hex(), float(width).hex())], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=os.path.abspath(a.parent_tree))
        assert json.loads(base.stdout.readline())["ready"]
    timed(g.label_histograms, a.warmup)
    new_ms, base_ms = [], []
    for count in blocks:
        xs, (fg_hist, bg_hist) = timed(g.label_histograms, count)
        new_ms += xs
        if base:
            base.stdin.write("%d\n" % count)
            base.stdin.flush()
            got = json.loads(base.stdout.readline())
            base_ms += got["ms"]
            assert got["fg"] == fg_hist.tolist() and got["bg"] == bg_hist.tolist(), "the baseline's histograms differ"   # the same numbers on both paths
    if base:
        base.stdin.write("0\n")
        base.stdin.flush()
        base.wait(timeout=60)
    assert int(fg_hist.sum()) == int(labels.sum()) and int(fg_hist.sum() + bg_hist.sum()) == nvox
    rec["label_histograms_ms"] = summary(new_ms)
    rec["label_histogram_info"] = g.label_histogram_info()
    rec["bytes_read"] = nvox * (1 + img.dtype.itemsize)
    rec["device_copy_same_bytes"] = device_copy_gbs(rec["bytes_read"])
    if base_ms:
        rec["baseline_marker_histograms_ms"] = summary(base_ms)
        rec["baseline_bytes_read"] = nvox * (2 + img.dtype.itemsize)
        rec["baseline_device_copy_same_bytes"] = device_copy_gbs(rec["baseline_bytes_read"])
        rec["histograms_equal"] = True
        rec["new_over_baseline"] = round(rec["label_histograms_ms"]["median"] / rec["baseline_marker_histograms_ms"]["median"], 3)
    emit(rec, a.out)
    # -- loop: every call of the loop timed where the loop makes it
    rows, cur = [], {}

    def wrap(name, call, note=False):
        def inner(*args, **kw):
            t0 = time.perf_counter()
            res = call(*args, **kw)
            cur[name + "_ms"] = (time.perf_counter() - t0) * 1e3
            if note:
                cur.update(("update_" + k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", g.last_note()))
            if name == "maxflow":
                cur["solve_ms"] = g.stats()["solve_ms"]
                rows.append(dict(cur))
                cur.clear()
            return res
        return inner
    tables = graph_module.histogram_tables
    graph_module.histogram_tables = wrap("histogram_tables", tables)
    g.label_histograms = wrap("label_histograms", g.label_histograms)
    g.update_tweights_binned = wrap("update_tweights_binned", g.update_tweights_binned, note=True)
    g.maxflow = wrap("maxflow", g.maxflow)
    t0 = time.perf_counter()
    res = g.iterate_regional_histogram(max_refits=8)
    total_ms = (time.perf_counter() - t0) * 1e3
    graph_module.histogram_tables = tables
    for row, r in zip(rows, res["rounds"]):
        row.update(moved=r["moved"], fg_voxels=r["fg_voxels"], flow=r["flow"])
    keys = [k for k in rows[0] if k.endswith("_ms")]
    emit({"part": "loop", "volume": volume, "size": n, "dtype": img.dtype.name, "nbins": nbins, "refits": len(res["rounds"]), "converged": res["converged"],
          "total_ms": round(total_ms, 3), "last_look_ms": round(cur.get("label_histograms_ms", 0.0), 4), "fg_voxels_final": int(res["fg_hist"].sum()),
          "per_refit_ms": {k: summary([r[k] for r in rows]) for k in keys}, "rounds": [{k: (round(v, 4) if isinstance(v, float) and k.endswith("_ms") else v) for k, v in r.items()} for r in rows]},
         a.out)
    g.close()


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
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the baseline of part hist")
    ap.add_argument("--limit", type=int, default=400, help="time limit of one volume's child process, seconds")
    ap.add_argument("--child", nargs=2, metavar=("VOLUME", "SIZE"), help="(internal) run one volume in this process")
    ap.add_argument("--baseline", nargs=4, metavar=("VOLUME", "SIZE", "LABELS", "BINNING"), help="(internal) the baseline's process, on the parent tree")
    a = ap.parse_args()
    if a.baseline:
        return baseline(a)   # (medpy_amd comes from PYTHONPATH: the parent tree)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    if a.child:
        return run(a.child[0], int(a.child[1]), a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in a.sizes:
        for volume in a.volumes:   # a fresh child process per volume, under its own time limit; the first failure ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--child", volume, str(n), "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
            if a.out:
                cmd += ["--out", a.out]
            if a.parent_tree:
                cmd += ["--parent-tree", a.parent_tree]
            rc = subprocess.run(cmd, timeout=a.limit).returncode
            if rc != 0:
                sys.exit("gpu_label_histograms: %s %d^3 ended with status %d: stopping" % (volume, n, rc))


if __name__ == "__main__":
    main()
