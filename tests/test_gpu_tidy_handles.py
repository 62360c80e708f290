"""-m gpu: a handle nobody closed goes back to the device's pool when the garbage collector frees it, not before and not never.

``VoxelGraph.__del__`` closes the handle, so a graph that falls out of scope gives its device memory back at once -- unless it sits
in a reference cycle, which is what a test leaves behind that catches an error of the graph with ``pytest.raises(...) as ei`` and does
not close it (the traceback holds the frame, the frame holds the graph and ``ei``).  Such a handle lives until the collector runs,
and the pool's idle bytes move at that moment, whatever test is running then.  This module states the behaviour and, placed by its
name behind the modules that leave such handles and in front of those that compare the pool's idle bytes with ``==``
(test_gpu_tweight_paths.py), hands them a pool that has settled: every unreachable handle is released here."""
import gc
import weakref

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_a_handle_in_a_cycle_goes_back_to_the_pool_when_collected():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    gc.collect()   # what earlier tests left unreachable is released first
    was_enabled = gc.isenabled()
    gc.disable()   # between the two looks below nothing but this test decides when the collector runs
    try:
        g = VoxelGraph((64, 64, 64))
        g._set_feature_image(np.zeros((64, 64, 64), np.float32))   # a block of its own, above the pool's threshold of 1 MiB
        held = g.stats()["device_bytes"]
        assert held > 64 ** 3 * 4
        alive = weakref.ref(g)
        cycle = [g]
        cycle.append(cycle)
        idle_held = _lib.pool_info()["idle_bytes"]
        del g, cycle
        assert alive() is not None                                  # unreachable, and not freed: only the collector can
        assert _lib.pool_info()["idle_bytes"] == idle_held
        gc.collect()
        assert alive() is None
        idle_freed = _lib.pool_info()["idle_bytes"]
        assert idle_held <= idle_freed <= idle_held + held          # its blocks went to the pool (or, past the pool's budget, to the driver)
        gc.collect()
        assert _lib.pool_info()["idle_bytes"] == idle_freed         # settled: nothing is left for a later collection to move
    finally:
        if was_enabled:
            gc.enable()


def test_a_closed_handle_has_nothing_left_for_the_collector():
    from medpy_amd import _lib
    from medpy_amd.graphcut import VoxelGraph
    g = VoxelGraph((64, 64, 64))
    with pytest.raises(_lib.MedpyHipError) as ei:   # the cycle a test leaves: traceback -> frame -> g, ei
        g.edit_markers(fg=[5])                      # nothing was built
    assert ei.value.code == _lib.ERR_STATE
    g.close()
    idle = _lib.pool_info()["idle_bytes"]
    del g, ei
    gc.collect()
    assert _lib.pool_info()["idle_bytes"] == idle
