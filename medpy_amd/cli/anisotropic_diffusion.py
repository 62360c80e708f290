"""Anisotropic diffusion command line: the reference's ``bin/medpy_anisotropic_diffusion.py`` on MI355X.

It takes what the reference's script takes -- ``input output [-i ITERATIONS] [-k KAPPA] [-g GAMMA] [-v] [-d] [-f]``, with its
defaults, kappa an integer, the filter's default conduction function (option 1) -- so that a pipeline can swap one for the other; the
text and the code are this package's own.  The voxel spacing is taken from the input's header; files go through ``medpy_amd.io``
(.npy / NIfTI-1).
"""
import argparse
import logging
import os

from ..filter.smoothing import anisotropic_diffusion
from ..io import get_pixel_spacing, load, save

__description__ = """
Smooth an image on an AMD MI355X without blurring its edges (anisotropic diffusion after Perona and Malik).  Takes the arguments of
MedPy's medpy_anisotropic_diffusion.py.  The spacing of the voxels is read from the input's header; intensities scaled to [0, 1] and a
matching kappa work best.
"""


def build_parser():
    """the command line: two positionals and the options -i -k -g -v -d -f"""
    p = argparse.ArgumentParser(description=__description__)
    p.add_argument("input", help="image to smooth (.nii, .nii.gz or .npy)")
    p.add_argument("output", help="where the smoothed float32 image goes")
    p.add_argument("-i", "--iterations", type=int, default=1, help="how many diffusion steps to take (default 1)")
    p.add_argument("-k", "--kappa", type=int, default=50, help="conduction coefficient: intensity steps well above it stop the diffusion (default 50)")
    p.add_argument("-g", "--gamma", type=float, default=0.1, help="step size of one iteration; stable up to 0.25 (default 0.1)")
    p.add_argument("-v", dest="verbose", action="store_true", help="report progress")
    p.add_argument("-d", dest="debug", action="store_true", help="report progress and details")
    p.add_argument("-f", dest="force", action="store_true", help="overwrite the output if it exists")
    return p


getParser = build_parser   # the name the other command lines of this package use


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    log = logging.getLogger("medpy_amd")
    logging.basicConfig(format="%(levelname)s: %(message)s")
    log.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)
    if os.path.exists(args.output) and not args.force:   # before the work, not after it
        parser.error("{} is there already; -f overwrites it".format(args.output))
    image, header = load(args.input)
    spacing = get_pixel_spacing(header)
    log.info("%d iteration(s), kappa %s, gamma %s, spacing %s", args.iterations, args.kappa, args.gamma, spacing)
    smoothed = anisotropic_diffusion(image, args.iterations, args.kappa, args.gamma, spacing)
    save(smoothed, args.output, header, args.force)
    log.info("wrote %s", args.output)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
