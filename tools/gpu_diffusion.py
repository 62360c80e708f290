"""What the anisotropic diffusion costs on the device (mgc_diffuse_image, mgc_diffuse; profiles/README).

For every size, input dtype (uint16, float32) and option (1, 2, 3):
  iteration:  ms per iteration of k_diffuse from HIP events around the launches (the iterate_ms of the note mgc_diffuse leaves in
              mgc_last_error): 3 warm-up calls, then the median, minimum and maximum of 7 calls of one iteration each on a handle
              that holds the image; the same for calls of 5 iterations (float32 to float32 from the second on); the achieved
              bytes/s by the model of 8 B per voxel and iteration (one float32 read, one written), next to a plain device copy of
              as many bytes in the same run (a process of its own)
  call:       niter = 5 through the C ABI without a handle (mgc_diffuse_image) and through Python
              (medpy_amd.filter.anisotropic_diffusion): host-clock ms of the whole call, with the upload_ms, iterate_ms and
              download_ms of the note stated apart
  e1:         (--e1, once, in a child process) option 1 on the device against tests/golden/diffusion.npz: for every option-1 case of
              tests/diffusion_cases.py a row `e1_device_vs_golden` with e = max|a - golden| / ptp(golden) and whether the device
              equalled the NumPy statement bit for bit, then `e1_device_vs_golden_max` with the largest e next to the bound
  host:       (--host N, once) the NumPy statement of tests/diffusion_cases.py on this machine's host at N^3 for one iteration,
              option 2 -- ours, not the reference's, which is not needed here
Nothing is gated on a time: the file is the record.  Every size runs in a child process of its own under a time limit; the first
that fails or runs out of time ends the run.

  python tools/gpu_diffusion.py [--sizes 256 512] [--limit 300] [--e1] [--host 256] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WARMUP, REPEATS = 3, 7


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def note_ms(note):
    return {k: float(v) for k, v in re.findall(r"(\w+_ms)=([0-9.]+)", note)}


def image_of(n, dtype):
    import numpy as np
    rng = np.random.default_rng(5)
    if dtype == "uint16":
        return rng.integers(0, 4096, (n, n, n)).astype(np.uint16)
    return rng.normal(100.0, 40.0, (n, n, n)).astype(np.float32)


def run(n):
    import numpy as np
    from gpu_dense_tweights import device_copy_gbs
    from medpy_amd import _lib
    from medpy_amd import filter as flt
    from medpy_amd.graphcut import VoxelGraph
    lib = _lib.load()
    nvox = n ** 3
    rows = []
    copy = device_copy_gbs(8 * nvox)
    out = np.empty((n, n, n), np.float32)
    shp = (C.c_int64 * 3)(n, n, n)
    for dtype in ("uint16", "float32"):
        img = image_of(n, dtype)
        g = VoxelGraph((n, n, n))
        g._set_feature_image(img)
        for option in (1, 2, 3):
            row = {"kind": "gpu", "shape": [n, n, n], "dtype": dtype, "option": option, "kappa": 50.0, "gamma": 0.1, "warmup": WARMUP, "repeats": REPEATS}
            for niter, key in ((1, "iteration_ms"), (5, "five_iterations_ms")):
                ms = []
                for r in range(WARMUP + REPEATS):
                    _lib.check(g._h, lib.mgc_diffuse(g._h, niter, 50.0, 0.1, None, option, 0, _lib.ptr(out), None))
                    if r >= WARMUP:
                        ms.append(note_ms(lib.mgc_last_error(g._h).decode())["iterate_ms"] / niter)
                row[key] = summary(ms)
            row["model_bytes_per_voxel_iteration"] = 8
            row["achieved_gbs_first_iteration"] = round(8 * nvox / (row["iteration_ms"]["median"] * 1e-3) / 1e9, 1)
            row["achieved_gbs_five_iterations"] = round(8 * nvox / (row["five_iterations_ms"]["median"] * 1e-3) / 1e9, 1)
            if copy:
                row["device_copy_same_bytes"] = copy
            # the whole call, niter = 5
            t0 = time.perf_counter()
            _lib.check(None, lib.mgc_diffuse_image(0, 3, shp, _lib.ptr(img), _lib.DTYPE_IDS[img.dtype], 5, 50.0, 0.1, None, option, _lib.ptr(out), None))
            first = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            _lib.check(None, lib.mgc_diffuse_image(0, 3, shp, _lib.ptr(img), _lib.DTYPE_IDS[img.dtype], 5, 50.0, 0.1, None, option, _lib.ptr(out), None))
            row["c_abi_niter5"] = dict(note_ms(lib.mgc_last_error(None).decode()), first_call_ms=round(first, 3), call_ms=round((time.perf_counter() - t0) * 1e3, 3))
            t0 = time.perf_counter()
            flt.anisotropic_diffusion(img, 5, 50.0, 0.1, None, option)
            row["python_niter5"] = dict(note_ms(lib.mgc_last_error(None).decode()), call_ms=round((time.perf_counter() - t0) * 1e3, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        g.close()
    return rows


def e1_device():
    """option 1 on the device against the golden file, case by case"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import diffusion_cases as dc
    from medpy_amd import filter as flt
    rows = []
    for c in dc.CASES:
        if c.option == 1:
            got = flt.anisotropic_diffusion(dc.image(c), c.niter, c.kappa, c.gamma, c.spacing, 1)
            same = bool(np.array_equal(got, dc.statement(dc.image(c), c.niter, c.kappa, c.gamma, c.spacing, 1)))
            rows.append({"kind": "e1_device_vs_golden", "case": c.name, "e": dc.error_measure(got, dc.golden(c.name)), "equals_statement": same})
    rows.append({"kind": "e1_device_vs_golden_max", "e": max(r["e"] for r in rows), "bound": dc.E1_BOUND, "cases": len(rows),
                 "equal_to_statement": sum(r["equals_statement"] for r in rows)})
    for r in rows:
        print(json.dumps(r), flush=True)


def host(n):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import diffusion_cases as dc
    img = image_of(n, "float32")
    t0 = time.perf_counter()
    dc.statement(img, 1, 50.0, 0.1, None, 2)
    return {"kind": "host_numpy_statement", "what": "tests/diffusion_cases.py:statement (ours, not the reference's), one iteration, option 2, float32", "shape": [n, n, n],
            "ms": round((time.perf_counter() - t0) * 1e3, 1), "numpy": np.__version__}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--limit", type=int, default=300, help="seconds per size")
    ap.add_argument("--e1", action="store_true", help="also option 1 on the device against the golden file, case by case")
    ap.add_argument("--host", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        e1_device() if args.child == "e1" else run(int(args.child))
        return 0
    lines, rc = [], 0
    for n in (["e1"] if args.e1 else []) + list(args.sizes):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n)], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("part %s ran out of time: the run ends here" % n, file=sys.stderr)
            rc = 1
            break
        if r.returncode != 0:
            print("part %s failed (%d): the run ends here\n%s" % (n, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            rc = 1
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.host and not rc:
        lines.append(json.dumps(host(args.host)))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    print(text, end="")
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
