"""Where the drivers that bring kernels of their own come into the library ("Headline check"): a kernel lies in
the code object where the host code first names it, so the six driver files are included at the very end of mgc_kernels.hip, behind
its last function, one behind the other in the order they were added -- and nowhere else.  Shared by the host tests of those drivers."""
import os
import re

DRIVERS = ["mgc_reach_driver.inl", "mgc_binned_driver.inl", "mgc_label_hist_driver.inl", "mgc_cc_driver.inl", "mgc_edt_driver.inl", "mgc_geo_driver.inl"]


def assert_behind_everything_before_it(own, prefix):
    """``own`` (a driver file) stands in its place of the list at the end of mgc_kernels.hip; nothing else of the kernel file or of the
    drivers in front of it includes a file whose name begins with ``prefix``, and no driver includes another"""
    from medpy_amd import build
    text = open(os.path.join(build.CSRC, "mgc_kernels.hip")).read()
    tail = [ln for ln in text.splitlines() if ln.strip()][-len(DRIVERS):]
    for ln, d in zip(tail, DRIVERS):   # the last lines of the file, each the include and at most a comment
        assert re.fullmatch(r'#include "%s"\s*(/\*.*\*/)?' % re.escape(d), ln), ln
    assert text.index('#include "%s"' % DRIVERS[0]) > text.index("int mgc_get_stats(")   # (the last function of the file)
    includes = lambda s: [ln for ln in s.splitlines() if ln.lstrip().startswith("#include")]
    assert [ln for ln in includes(text) if '"%s' % prefix in ln] == [tail[DRIVERS.index(own)]]
    for d in DRIVERS:
        theirs = includes(open(os.path.join(build.CSRC, d)).read())
        assert not [ln for ln in theirs if "_driver.inl" in ln], d
        if DRIVERS.index(d) < DRIVERS.index(own):
            assert not [ln for ln in theirs if '"%s' % prefix in ln], d
