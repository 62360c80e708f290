"""The command line of the anisotropic diffusion: the surface of the reference's bin/medpy_anisotropic_diffusion.py,
and a small NIfTI volume through it and back against the reference's recorded output (on the GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import diffusion_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "2x9x66-uint8-noise-n2-k50-g0.1-o1-sp1.5_0.7_2.2"   # what the script can express: an integer kappa, option 1, the header's spacing


def test_parser_matches_the_reference_surface():
    from medpy_amd.cli.anisotropic_diffusion import getParser
    a = getParser().parse_args(["in.nii", "out.nii", "-i", "7", "-k", "30", "-g", "0.2", "-v", "-f"])
    assert (a.input, a.output, a.iterations, a.kappa, a.gamma, a.verbose, a.debug, a.force) == ("in.nii", "out.nii", 7, 30, 0.2, True, False, True)
    d = getParser().parse_args(["a", "b"])
    assert (d.iterations, d.kappa, d.gamma, d.verbose, d.debug, d.force) == (1, 50, 0.1, False, False, False)   # the reference's defaults
    assert getParser().parse_args(["a", "b", "--iterations", "3", "--kappa", "9", "--gamma", "1"]).iterations == 3
    with pytest.raises(SystemExit):
        getParser().parse_args(["a", "b", "-k", "2.5"])   # kappa is an integer on the command line, as in the reference
    assert os.access(os.path.join(ROOT, "bin", "medpy_amd_anisotropic_diffusion.py"), os.X_OK)
    case = dc.BY_NAME[CASE]
    assert case.option == 1 and case.kappa == int(case.kappa) and case.spacing is not None and case.niter == 2


@pytest.mark.gpu
def test_a_small_nifti_round_trips_against_the_reference(tmp_path):
    from medpy_amd import io
    case = dc.BY_NAME[CASE]
    src, dst = str(tmp_path / "in.nii.gz"), str(tmp_path / "out.nii")
    io.save(dc.image(case), src, io.Header(case.spacing), force=True)
    script = os.path.join(ROOT, "bin", "medpy_amd_anisotropic_diffusion.py")
    cmd = [sys.executable, script, src, dst, "-i", str(case.niter), "-k", str(int(case.kappa)), "-g", repr(case.gamma)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got, hdr = io.load(dst)
    assert io.get_pixel_spacing(hdr) == tuple(float(np.float32(s)) for s in case.spacing)
    dc.check(np.ascontiguousarray(got), case, "command line")
    # an existing output is refused without -f and overwritten with it
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode != 0 and "is there already" in out.stderr
    assert subprocess.run(cmd + ["-f"], capture_output=True, text=True).returncode == 0
