#!/usr/bin/env python
"""Writes tests/golden/watershed.npz: what the reference's medpy.filter.image.local_minima returns for every minimum-filter case of
tests/watershed_cases.py (MIN_CASES): ``<case>/indices`` and ``<case>/values``.  Results only; nothing of the reference is copied.

    python tools/gen_watershed_golden.py --reference /path/to/medpy-checkout [--out FILE]

The reference's image.py is loaded from its source file.  Its ``from ..io import header`` and ``from .utilities import ...`` would
drag in medpy.io (and SimpleITK); the loader gives it stub parent packages instead: local_minima uses neither.  The order of equal
values in the pair is that of the reference's (unstable) ``argsort()`` on the machine that wrote the file: tests compare the values
and, per value, the sets of indices.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_reference(path):
    """the reference's local_minima, from <path>/medpy/filter/image.py"""
    src = os.path.join(path, "medpy", "filter", "image.py")
    top = types.ModuleType("_refmedpy")
    top.__path__ = []
    io = types.ModuleType("_refmedpy.io")
    io.header = None
    pkg = types.ModuleType("_refmedpy.filter")
    pkg.__path__ = []
    util = types.ModuleType("_refmedpy.filter.utilities")
    stub = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("stub"))
    setattr(util, "__make_footprint", stub)
    util.pad = stub
    for m in (top, io, pkg, util):
        sys.modules[m.__name__] = m
    spec = importlib.util.spec_from_file_location("_refmedpy.filter.image", src)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.local_minima


def generate(reference):
    import watershed_cases as wc
    fn = load_reference(reference)
    out = {}
    for c in wc.MIN_CASES:
        idx, val = fn(c.image, c.size)
        assert idx.shape == (val.size, c.image.ndim) and val.dtype == c.image.dtype, c.name
        out[c.name + "/indices"] = idx.astype(np.int32)
        out[c.name + "/values"] = val
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds medpy/filter/image.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "watershed.npz"))
    args = ap.parse_args()
    gold = generate(args.reference)
    np.savez_compressed(args.out, **gold)
    print("%d cases, %d bytes -> %s" % (len(gold) // 2, os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
