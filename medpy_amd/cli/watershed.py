"""Watershed command line: the reference's ``bin/medpy_watershed.py`` on MI355X.

It takes what the reference's script takes -- ``input output [--mindist N] [--mask FILE] [-v] [-d] [-f]``, with its defaults -- so
that a pipeline can swap one for the other; the text and the code are this package's own.  The local minima of the input (usually a
gradient image) at least ``--mindist`` voxels apart become the markers, touching ones joined and numbered as
``scipy.ndimage.label`` numbers them, and the seeded watershed grows the regions from them: the region image
``medpy_amd_graphcut_label.py`` takes.  Files go through ``medpy_amd.io`` (.npy / NIfTI-1).

One deliberate difference: the reference tests its mask with ``if not None == mask``, which raises on an array under NumPy 2; here a
mask that is given is applied -- minima outside it are no markers, and voxels outside it keep the label 0.
"""
import argparse
import logging
import os

import numpy

from ..filter.image import minima_markers, watershed, watershed_info
from ..io import load, save

__description__ = """
Segment an image into catchment basins on an AMD MI355X (seeded watershed from the local minima).  Takes the arguments of MedPy's
medpy_watershed.py.  The voxel spacing is not taken into account.
"""


def build_parser():
    """the command line: two positionals and the options --mindist --mask -v -d -f"""
    p = argparse.ArgumentParser(description=__description__)
    p.add_argument("input", help="image to segment, usually a gradient image (.nii, .nii.gz or .npy)")
    p.add_argument("output", help="where the int32 region image goes")
    p.add_argument("--mindist", type=int, default=2, help="smallest distance between two local minima, in voxels (default 2)")
    p.add_argument("--mask", help="binary image: the watershed runs where it is not zero")
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
    mask = None
    if args.mask:
        mask = load(args.mask)[0].astype(numpy.bool_)
        if mask.shape != image.shape:
            parser.error("the mask has shape {}, the image {}".format(mask.shape, image.shape))
    log.info("local minima at least %d voxel(s) apart", args.mindist)
    markers = minima_markers(image, args.mindist, mask)
    log.info("%d markers; flooding", int(markers.max()) if markers.size else 0)
    regions = watershed(image, markers, mask)
    log.debug("device work: %s", watershed_info())
    save(regions, args.output, header, args.force)
    log.info("wrote %s", args.output)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
