#!/usr/bin/env python3
"""MI355X drop-in for MedPy's bin/medpy_anisotropic_diffusion.py (see medpy_amd/cli/anisotropic_diffusion.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medpy_amd.cli.anisotropic_diffusion import main  # noqa: E402

if __name__ == "__main__":
    raise SystemExit(main())
