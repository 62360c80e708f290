#!/usr/bin/env python
"""Writes tests/golden/diffusion.npz: the output of the reference's medpy.filter.smoothing.anisotropic_diffusion for every case of
tests/diffusion_cases.py.  Results only; nothing of the reference is copied.

    python tools/gen_diffusion_golden.py --reference /path/to/medpy-checkout [--out FILE] [--measure]

The reference's smoothing.py is loaded from its source file.  Its ``from .utilities import xminus1d`` would drag in medpy.io (and
SimpleITK); the loader gives it a stub parent package with a dummy ``xminus1d`` instead.  --measure also computes, for every
option-1 case, e = max|statement - golden| / ptp(golden) of the statement of diffusion_cases.py (f64 exp, rounded once), writes the
values to profiles/diffusion.jsonl (rows of kind "e1_statement_vs_golden") and prints the largest: E1_MEASURED of diffusion_cases.py.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_reference(path):
    """the reference's anisotropic_diffusion, from <path>/medpy/filter/smoothing.py"""
    src = os.path.join(path, "medpy", "filter", "smoothing.py")
    pkg = types.ModuleType("_refmedpy_filter")
    pkg.__path__ = []
    util = types.ModuleType("_refmedpy_filter.utilities")
    util.xminus1d = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("stub"))
    sys.modules["_refmedpy_filter"] = pkg
    sys.modules["_refmedpy_filter.utilities"] = util
    try:
        import scipy.ndimage  # noqa: F401
    except Exception:  # the module imports gaussian_filter at its top; the diffusion does not use it
        nd = types.ModuleType("scipy.ndimage")
        nd.gaussian_filter = None
        sys.modules.setdefault("scipy", types.ModuleType("scipy"))
        sys.modules["scipy.ndimage"] = nd
    spec = importlib.util.spec_from_file_location("_refmedpy_filter.smoothing", src)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.anisotropic_diffusion


def generate(reference):
    import diffusion_cases as dc
    fn = load_reference(reference)
    out = {}
    with np.errstate(all="ignore"):
        for c in dc.CASES:
            res = fn(dc.image(c), niter=c.niter, kappa=c.kappa, gamma=c.gamma, voxelspacing=c.spacing, option=c.option)
            assert res.dtype == np.float32 and res.shape == c.shape, c.name
            out[c.name] = res
    return out


def measure(gold):
    """rows of e for every option-1 case, and the largest"""
    import diffusion_cases as dc
    rows = []
    for c in dc.CASES:
        if c.option == 1:
            e = dc.error_measure(dc.statement(dc.image(c), c.niter, c.kappa, c.gamma, c.spacing, 1), gold[c.name])
            rows.append({"kind": "e1_statement_vs_golden", "case": c.name, "e": e, "numpy": np.__version__})
    return rows, max(r["e"] for r in rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds medpy/filter/smoothing.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "diffusion.npz"))
    ap.add_argument("--measure", action="store_true", help="also measure option 1's statement against the golden file")
    args = ap.parse_args()
    gold = generate(args.reference)
    np.savez_compressed(args.out, **gold)
    print("%d cases, %d voxels, %d bytes -> %s" % (len(gold), sum(a.size for a in gold.values()), os.path.getsize(args.out), args.out))
    if args.measure:
        rows, top = measure(gold)
        path = os.path.join(ROOT, "profiles", "diffusion.jsonl")
        keep = [ln for ln in open(path).read().splitlines() if ln.strip() and json.loads(ln).get("kind") != "e1_statement_vs_golden"] if os.path.exists(path) else []
        with open(path, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps({"kind": "e1_statement_vs_golden_max", "E1_MEASURED": top, "cases": len(rows), "numpy": np.__version__}) + "\n")
            for ln in keep:
                if json.loads(ln).get("kind") != "e1_statement_vs_golden_max":
                    f.write(ln + "\n")
        print("E1_MEASURED = %r over %d option-1 cases" % (top, len(rows)))


if __name__ == "__main__":
    main()
