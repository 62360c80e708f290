"""CPU tier of the edits by list: the pure merge of the fg / bg / erase lists into the (ids, ops) list that
mgc_edit_markers takes, and the agreement of header, symbol table and library on the three new calls."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _merge(*a, **kw):
    from medpy_amd.graphcut.graph import merge_marker_edits
    return merge_marker_edits(*a, **kw)


def _apply_ops(fg, bg, ids, ops):
    """what the scatter kernel does to the mask planes"""
    fg, bg = fg.copy().ravel(), bg.copy().ravel()
    fg[ids[(ops & 4) != 0]] = False
    bg[ids[(ops & 8) != 0]] = False
    fg[ids[(ops & 1) != 0]] = True
    bg[ids[(ops & 2) != 0]] = True
    return fg, bg


def test_flat_ids_and_index_tuples_give_the_same_list():
    shape = (5, 6, 7)
    rng = np.random.default_rng(3)
    fg, bg, er = (rng.random(shape) < 0.1 for _ in range(3))
    a = _merge(shape, np.flatnonzero(fg), np.flatnonzero(bg), np.flatnonzero(er))
    b = _merge(shape, np.nonzero(fg), np.nonzero(bg), np.nonzero(er))
    c = _merge(shape, np.flatnonzero(fg).astype(np.int32), np.flatnonzero(bg).astype(np.uint16), list(np.flatnonzero(er)))
    for ids, ops in (a, b, c):
        assert ids.dtype == np.int64 and ops.dtype == np.uint8 and ids.shape == ops.shape
        assert np.array_equal(ids, a[0]) and np.array_equal(ops, a[1])
    assert np.all(np.diff(a[0]) > 0)
    assert np.array_equal(a[0], np.flatnonzero(fg | bg | er))
    # 2-D and 1-D volumes
    assert np.array_equal(_merge((4, 5), fg=([1, 3], [2, 4]))[0], [7, 19])
    assert np.array_equal(_merge((9,), bg=(np.array([8, 2]),))[0], [2, 8])


def test_merged_ops_of_ids_in_several_lists():
    ids, ops = _merge((100,), fg=[1, 4, 5, 7], bg=[2, 4, 6, 7], erase=[3, 5, 6, 7])
    assert ids.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert ops.tolist() == [1, 2, 4 | 8, 1 | 2, 1 | 8, 2 | 4, 1 | 2]
    assert all(0 < o <= 15 and (o & 5) != 5 and (o & 10) != 10 for o in ops.tolist())  # what the library accepts


def test_repeats_inside_a_list_count_once():
    ids, ops = _merge((10,), fg=[3, 3, 1, 3], bg=[1, 1], erase=[9, 9, 3])
    assert ids.tolist() == [1, 3, 9] and ops.tolist() == [3, 9, 12]


def test_nothing_to_do():
    for kw in ({}, dict(fg=[], bg=np.empty(0, dtype=np.int64), erase=None), dict(fg=(np.empty(0, int), np.empty(0, int)))):
        ids, ops = _merge((3, 4), **kw)
        assert ids.size == 0 and ops.size == 0 and ids.dtype == np.int64 and ops.dtype == np.uint8


@pytest.mark.parametrize("kw", [dict(fg=[12]), dict(bg=[-1]), dict(erase=np.array([2 ** 63], dtype=np.uint64)),
                                dict(fg=np.array([1.0, 2.0])), dict(bg=np.array([True, False])), dict(erase=["a"]),
                                dict(fg=([1], [1], [1])), dict(fg=([1],)), dict(bg=([3], [0])), dict(bg=([0], [4])),
                                dict(erase=([0.5], [1])), dict(fg=([0, 1], [1])), dict(fg=np.zeros((2, 2), dtype=int))])
def test_value_errors(kw):
    with pytest.raises(ValueError):
        _merge((3, 4), **kw)


@pytest.mark.parametrize("shape", [(50,), (7, 9), (4, 5, 6)])
def test_list_applied_to_masks_is_the_mask_formula(shape):
    rng = np.random.default_rng(len(shape))
    for _ in range(20):
        fg, bg = rng.random(shape) < 0.3, rng.random(shape) < 0.3
        f, b, e = (rng.integers(0, fg.size, rng.integers(0, 30)) for _ in range(3))  # repeats and overlaps included
        ids, ops = _merge(shape, f, b, e)
        mf, mb, me = (np.isin(np.arange(fg.size), x) for x in (f, b, e))
        got_fg, got_bg = _apply_ops(fg, bg, ids, ops)
        assert np.array_equal(got_fg, (fg.ravel() & ~me) | mf)
        assert np.array_equal(got_bg, (bg.ravel() & ~me) | mb)


def test_header_table_and_library_agree_on_the_new_calls():
    from medpy_amd import _lib, build
    build.build_library()
    header = open(os.path.join(ROOT, "include", "medpy_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    want = {"mgc_edit_markers": r"int mgc_edit_markers\(mgc_handle h, int64_t n, const int64_t\* ids, const uint8_t\* ops\);",
            "mgc_get_markers": r"int mgc_get_markers\(mgc_handle h, uint8_t\* fg, uint8_t\* bg\);",
            "mgc_labels_delta": r"int mgc_labels_delta\(mgc_handle h, int64_t cap, int64_t\* ids, int64_t\* n\);"}
    for name, decl in want.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == decl.count(",") + 1
    # mgc_stats grew by one double at its end, in the header and in the ctypes mirror alike
    body = re.search(r"typedef struct mgc_stats \{(.*?)\} mgc_stats;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:double|int64_t)\s+(\w+)", body, re.M)
    assert fields[-2:] == ["update_ms", "delta_ms"]
    assert [k for k, _ in _lib.Stats._fields_] == fields
    assert ctypes.sizeof(_lib.Stats) == 8 * (len(fields) + 2)  # (reserved[3] is one field of three words)
