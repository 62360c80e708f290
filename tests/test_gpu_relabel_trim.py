"""-m gpu: the three economies of the incremental global relabel against the BK oracle -- labels equal, flow to 1e-9, mgc_validate
all zero -- each case as shipped and with the thresholds that route a small volume through the kernel forms of a large one
(conftest.LARGE_VOLUME_FORMS, set on the handle).

 seeds     k_reset_suspect queues only the reset tiles a label can come from (mgc_reset_seeds_tile: a sink link, or a face
           neighbour that keeps labels).  The suspect region has to be at least three tiles thick, or every reset tile is on its
           rim: the ball of the sphere volume after a flood on radial labels (also with partial tiles), the weak-contrast volume
           (everything is suspect, the seeds are the tiles with a sink link), and a ball behind a wall that seals at once, so that
           a relabel ends with most of the tiles it reset still at INF.
 closure   the suspect closure stops after the first stretch of passes whose LAST pass changed nothing.  A bar of 40 x 2 x 2 tiles,
           markers on its end faces: a chain of supports crosses five bricks of 8 tiles, one brick per pass, so a stretch of four
           passes can end on a pass that still changed something.  Along each axis.
 looks     the schedule reads the counters from a buffer the device writes, guarded by a sequence number.  Two handles built and
           solved in turn, thirty times each: a stale snapshot, or the other handle's, shows as a solve that differs from the
           handle's first."""
import functools

import numpy as np
import pytest

from oracle import pipeline

pytestmark = pytest.mark.gpu

FORMS = ["as_shipped", "large_volume_forms"]


def _apply_forms(g, forms):
    if forms == "large_volume_forms":
        from conftest import LARGE_VOLUME_FORMS
        for kv in LARGE_VOLUME_FORMS.split(","):
            k, v = kv.split("=")
            g.set_param(k, int(v))


def _sealed(shape):
    """the sphere volume with an edge no flow crosses (exp(-(300 / 15)^2) underflows to the smallest weight): the wall seals with
    the first pushes, and every relabel after that resets a ball that stays at INF"""
    from medpy_amd import synthetic
    return synthetic.sphere(shape, step=300.0, noise=2.0)


def _bar(axis):
    """320 x 16 x 16 voxels along `axis`, foreground marker on one end face, background on the other; quiet noise, and a weaker
    plane inside the last brick before the background end (where the cut falls)"""
    shape = [16, 16, 16]
    shape[axis] = 320
    shape = tuple(shape)
    pos = np.arange(320).reshape([320 if a == axis else 1 for a in range(3)])
    img = np.random.default_rng(7).normal(0.0, 3.0, shape) + 25.0 * (pos >= 296)
    fg = np.zeros(shape, bool)
    bg = np.zeros(shape, bool)
    first = [slice(None)] * 3
    last = [slice(None)] * 3
    first[axis], last[axis] = 0, -1
    fg[tuple(first)] = True
    bg[tuple(last)] = True
    return {"image": img.astype(np.float32), "fg": fg, "bg": bg, "sigma": 15.0, "term": "difference_exponential"}


@functools.lru_cache(maxsize=None)
def _case(name, shape):
    """(inputs, oracle result): computed once, shared by the forms and parameter sets of a case"""
    from medpy_amd import synthetic
    if name == "sealed":
        s = _sealed(shape)
    elif name == "bar":
        s = _bar(shape)
    else:
        s = getattr(synthetic, name)(shape)
    ref = pipeline.graphcut_voxel(s["fg"], s["bg"], term=s["term"], image=s["image"], sigma=s["sigma"])
    return s, ref


def _solve(s, forms, **params):
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph(s["image"].shape)
    g._set_boundary(s["term"], s["image"], s["sigma"], False)
    g._set_markers(s["fg"], s["bg"])
    _apply_forms(g, forms)
    for k, v in params.items():
        g.set_param(k, v)
    g._build()
    flow = g.maxflow()
    return g, flow


def _assert_oracle(g, flow, ref):
    from medpy_amd import _lib
    st = g.stats()
    print({k: st[k] for k in ("global_relabels", "phases", "discharge_tiles", "relabel_tiles", "radial_cycles")},
          "flow %r (BK %r), %d voxels differ" % (flow, ref.flow, int((g.labels() != ref.labels).sum())))
    np.testing.assert_array_equal(g.labels(), ref.labels)
    assert flow == pytest.approx(ref.flow, rel=1e-9)
    v = g.validate()
    assert not any(v[k] for k in _lib.VIOLATION_KEYS), v
    return st


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("shape", [(64, 64, 64), (52, 44, 68)])
def test_seeds_after_a_flood_on_radial_labels(shape, forms):
    s, ref = _case("sphere", shape)
    g, flow = _solve(s, forms, radial=1, radial_min_c=4, radial_min_walls=0)
    st = _assert_oracle(g, flow, ref)
    assert st["radial_cycles"] >= 1, st
    assert st["global_relabels"] >= 2, st  # (at least one incremental relabel ran)
    g.close()


@pytest.mark.parametrize("forms", FORMS)
def test_seeds_are_the_sink_tiles_where_everything_is_suspect(forms):
    s, ref = _case("hard", (48, 48, 48))
    g, flow = _solve(s, forms)
    st = _assert_oracle(g, flow, ref)
    assert st["global_relabels"] >= 2, st
    g.close()


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("radial", [0, 1])
def test_seeds_of_a_sealed_ball_that_stays_at_inf(radial, forms):
    from medpy_amd import _lib
    s, ref = _case("sealed", (64, 64, 64))
    g, flow = _solve(s, forms, radial=radial, radial_min_c=4, radial_min_walls=0)
    st = _assert_oracle(g, flow, ref)
    assert st["global_relabels"] >= 2, st
    # the source side is what the last relabel reset and could not reach from the sink: a ball five tiles across, all INF
    h = g.heights()
    assert (h[ref.labels] == _lib.HINF).all()
    g.close()


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_closure_along_a_bar_of_five_bricks(axis, forms):
    s, ref = _case("bar", axis)
    assert 0 < ref.labels.sum() < ref.labels.size
    g, flow = _solve(s, forms)
    st = _assert_oracle(g, flow, ref)
    assert st["global_relabels"] >= 2, st
    g.close()


def test_looks_of_two_handles_solved_in_turn():
    from medpy_amd import synthetic
    from medpy_amd.graphcut import VoxelGraph
    handles = []
    for n in (32, 40):
        s = synthetic.sphere((n, n, n))
        g = VoxelGraph((n, n, n))
        g._set_boundary(s["term"], s["image"], s["sigma"], False)
        g._set_markers(s["fg"], s["bg"])
        handles.append([g, None, None])
    for turn in range(30):
        for h in handles:
            g = h[0]
            g._build()
            flow = g.maxflow()
            labels = g.labels().copy()
            if turn == 0:
                h[1], h[2] = flow, labels
                assert 0 < labels.sum() < labels.size
            else:
                assert flow == h[1], (turn, flow, h[1])
                np.testing.assert_array_equal(labels, h[2])
    for h in handles:
        h[0].close()
