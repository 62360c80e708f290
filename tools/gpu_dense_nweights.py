"""What a boundary term of the caller's own costs when it reaches the tile solver as whole arrays (profiles/README).

For every size the headline volume (synthetic.sphere, 6-neighbourhood, markers only: bench.py's flagship) is built and solved
with the built-in exponential term; its three per-axis weight arrays are read back (nweights(axis), the layout of the reference's
__skeleton_base), padded to the full shape on the host, and handed to a FRESH handle without a boundary term as dense weights,
one mgc_add_nweights call per axis (symmetric: back = NULL).  That handle holds the same graph, so labels and flow must agree.
Recorded per size, one JSON line: per call the host-API time and the library's own split of it (upload, check, accumulate: a
host clock around stretches that end in a stream synchronise), the bytes the accumulate kernel moves and its bytes/s next to
a plain device-to-device copy of as many bytes (torch, HIP events), then build_ms, solve_ms, device_bytes, radial_cycles,
wall_tiles, launch counts, label SHA-256 and flow of both handles.  At sizes up to --edges-max the same graph is also put
together edge by edge through GCGraph.set_nweight, Python time included.  Nothing is gated on a time: the file is the record.

  python tools/gpu_dense_nweights.py [--sizes 64 256 512] [--edges-max 64] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medpy_amd import graphcut, synthetic  # noqa: E402
from medpy_amd.graphcut.graph import VoxelGraph, pad_skeleton_weights  # noqa: E402


def sha(labels):
    return hashlib.sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()[:16]


def device_copy_child(nbytes_moved):
    """(child process, torch alone on the device) one JSON line: GB/s and ms of the best of five device-to-device copies that move
    `nbytes_moved` bytes in all -- half read, half written"""
    import torch
    half = nbytes_moved // 2
    a = torch.zeros(half, dtype=torch.uint8, device="cuda")
    b = torch.empty(half, dtype=torch.uint8, device="cuda")
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    print(json.dumps({"gbs": round(2 * half / best / 1e6, 1), "ms": round(best, 3), "bytes": 2 * half}))


def device_copy_gbs(nbytes_moved):
    """the copy in a process of its own (the library and torch each bring a HIP runtime), or None where it cannot be had"""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--copy-bytes", str(nbytes_moved)], capture_output=True, text=True, timeout=120)
        return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    except Exception:  # noqa: BLE001
        return None


def solved(g):
    t0 = time.perf_counter()
    flow = g.maxflow()
    api_ms = (time.perf_counter() - t0) * 1e3
    st = g.stats()
    return {"flow": flow, "labels_sha256": sha(g.labels()), "maxflow_api_ms": round(api_ms, 3), "build_ms": round(st["build_ms"], 3),
            "solve_ms": round(st["solve_ms"], 3), "device_bytes": int(st["device_bytes"]), "radial_cycles": int(st["radial_cycles"]),
            "wall_tiles": int(st["wall_tiles"]), "global_relabels": int(st["global_relabels"]),
            "launches": {k: v for k, v in g.launch_counts().items() if v}}


def run(n, edges_max, out):
    shape = (n, n, n)
    s = synthetic.sphere(shape)
    rec = {"size": n, "voxels": n ** 3}
    g = graphcut.graph_from_voxels(s["fg"], s["bg"], boundary_term=graphcut.energy_voxel.boundary_difference_exponential,
                                   boundary_term_args=(s["image"], s["sigma"], False))
    rec["built_in"] = solved(g)
    t0 = time.perf_counter()
    ws = [g.nweights(axis) for axis in range(3)]
    rec["readback_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    g.close()
    t0 = time.perf_counter()
    full = [pad_skeleton_weights(shape, axis, w) for axis, w in enumerate(ws)]
    rec["pad_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    h = VoxelGraph(shape)
    h._set_markers(s["fg"], s["bg"])
    ntiles = ((n + 7) // 8) ** 3
    # per call: `there` is read twice (the arc and, shifted by the offset, its reverse), two planes of the store are read and written
    moved = 2 * n ** 3 * 8 + 4 * ntiles * 512 * 8
    calls = []
    for axis in range(3):
        off = tuple(1 if k == axis else 0 for k in range(3))
        t0 = time.perf_counter()
        h._add_nweights(off, full[axis])
        api_ms = (time.perf_counter() - t0) * 1e3
        note = dict((k, float(v)) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", h.last_note()))
        note["api_ms"] = round(api_ms, 3)
        note["accumulate_bytes"] = moved
        if note.get("accumulate_ms"):
            note["accumulate_gbs"] = round(moved / note["accumulate_ms"] / 1e6, 1)   # (the first call's time includes clearing the store)
        calls.append(note)
    rec["add_nweights_calls"] = calls
    t0 = time.perf_counter()
    h._build()
    rec["dense_build_api_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    rec["dense"] = solved(h)
    h.close()
    copy = device_copy_gbs(moved)
    if copy:
        rec["device_copy_same_bytes"] = copy
    rec["labels_equal"] = rec["dense"]["labels_sha256"] == rec["built_in"]["labels_sha256"]
    rec["flow_rel_diff"] = abs(rec["dense"]["flow"] - rec["built_in"]["flow"]) / max(abs(rec["built_in"]["flow"]), 1e-300)
    if n <= edges_max:
        ids = np.arange(n ** 3, dtype=np.int64).reshape(shape)
        t0 = time.perf_counter()
        gc = graphcut.GCGraph(n ** 3, 3 * n ** 3, shape=shape)
        gc.record_markers(s["fg"], s["bg"])
        for axis, w in enumerate(ws):
            lo = tuple(slice(0, n - 1) if k == axis else slice(None) for k in range(3))
            hi = tuple(slice(1, n) if k == axis else slice(None) for k in range(3))
            for i, j, v in zip(ids[lo].ravel().tolist(), ids[hi].ravel().tolist(), w.ravel().tolist()):
                gc.set_nweight(i, j, v, v)
        t1 = time.perf_counter()
        e = gc.get_graph()
        t2 = time.perf_counter()
        rec["edge_by_edge"] = dict(solved(e), set_nweight_calls=3 * n * n * (n - 1), python_calls_ms=round((t1 - t0) * 1e3, 1),
                                   get_graph_ms=round((t2 - t1) * 1e3, 1))
        e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--edges-max", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--copy-bytes", type=int, default=0, help="(internal) time a device copy of this many bytes and leave")
    a = ap.parse_args()
    if a.copy_bytes:
        return device_copy_child(a.copy_bytes)
    for n in a.sizes:
        run(n, a.edges_max, a.out)


if __name__ == "__main__":
    main()
