"""The command line of the watershed: the surface of the reference's bin/medpy_watershed.py, and a small NIfTI volume
through it and back against the statement (on the GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

import watershed_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_matches_the_reference_surface():
    from medpy_amd.cli.watershed import getParser
    a = getParser().parse_args(["in.nii", "out.nii", "--mindist", "7", "--mask", "m.nii", "-v", "-f"])
    assert (a.input, a.output, a.mindist, a.mask, a.verbose, a.debug, a.force) == ("in.nii", "out.nii", 7, "m.nii", True, False, True)
    d = getParser().parse_args(["a", "b"])
    assert (d.mindist, d.mask, d.verbose, d.debug, d.force) == (2, None, False, False, False)   # the reference's defaults
    with pytest.raises(SystemExit):
        getParser().parse_args(["a", "b", "--mindist", "2.5"])
    assert os.access(os.path.join(ROOT, "bin", "medpy_amd_watershed.py"), os.X_OK)


@pytest.mark.gpu
def test_a_small_nifti_round_trips_against_the_statement(tmp_path):
    from medpy_amd import io
    rng = np.random.default_rng(21)
    image = rng.integers(0, 6, (9, 17, 12)).astype(np.int16)
    mask = rng.random(image.shape) < 0.85
    src, msk, dst = str(tmp_path / "in.nii.gz"), str(tmp_path / "mask.nii"), str(tmp_path / "out.nii")
    io.save(image, src, io.Header((1.5, 0.7, 2.2)), force=True)
    io.save(mask.astype(np.uint8), msk, io.Header((1.5, 0.7, 2.2)), force=True)
    script = os.path.join(ROOT, "bin", "medpy_amd_watershed.py")
    for extra, m in (([], None), (["--mask", msk], mask)):
        cmd = [sys.executable, script, src, dst, "--mindist", "3", "-f"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        got, hdr = io.load(dst)
        plane = wc.minima_statement(image, 3) if m is None else wc.minima_statement(image, 3) & m
        markers = ndi.label(plane)[0].astype(np.int32)
        assert io.get_pixel_spacing(hdr) == tuple(float(np.float32(s)) for s in (1.5, 0.7, 2.2))
        assert np.array_equal(got, wc.statement(image, markers, m)[2])         # the mask IS applied (the reference raises on it under NumPy 2)
    # an existing output is refused without -f
    out = subprocess.run([sys.executable, script, src, dst], capture_output=True, text=True)
    assert out.returncode != 0 and "is there already" in out.stderr
