"""Writes tests/golden/metric_binary.json: the surface and count measures of the cases of tests/metric_cases.py as the reference's own
medpy/metric/binary.py computes them.  The file stores results only -- the cases are (pattern, shape, seed) in
metric_cases.py, the planes are rebuilt from them.

    python tools/gen_metric_golden.py --reference /path/to/medpy-checkout

The reference is loaded from its source file, on the machine that has it; nothing of it is copied."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metric_cases as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds medpy/metric/binary.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "metric_binary.json"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_metric_binary", os.path.join(args.reference, "medpy", "metric", "binary.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    gold = {"cases": [[name, list(shape), mc.PATTERNS[name][1]] for name, shape in mc.golden_cases()], "surface": {}, "counts": {}}
    for case in mc.golden_cases():
        a, b = mc.plane_of(case) != 0, mc.partner(case[1]) != 0
        gold["counts"][mc.case_id(case)] = {name: float(getattr(ref, name)(a, b)) for name in mc.COUNT_METRICS}
        for conn in mc.connectivities(case[1]):
            for spacing in mc.SPACINGS:
                sp = mc.spacing_for(spacing, a.ndim)
                gold["surface"][mc.golden_key(case, sp, conn)] = {name: float(getattr(ref, name)(a, b, sp, conn)) for name in mc.SURFACE_METRICS}
    with open(args.out, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d surface entries, %d count entries, %d bytes" % (args.out, len(gold["surface"]), len(gold["counts"]), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
