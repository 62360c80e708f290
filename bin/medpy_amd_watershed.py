#!/usr/bin/env python3
"""MI355X drop-in for MedPy's bin/medpy_watershed.py (see medpy_amd/cli/watershed.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medpy_amd.cli.watershed import main  # noqa: E402

if __name__ == "__main__":
    raise SystemExit(main())
