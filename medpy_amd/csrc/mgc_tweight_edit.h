/*
 * mgc_tweight_edit.h -- host preparation of an edit of explicit t-links by voxel list (mgc_edit_tweights): the list is
 * checked entry by entry before the first write, so that a refused call leaves the handle as it was (the approach of
 * msg_list_check.h), a list that does not ascend strictly is sorted in a copy, and the SEGMENTS of the store's share plane that
 * the list touches are named, so that only their partials of the flow constant are summed again.  Plain C++, no HIP:
 * mgc_kernels.hip includes it, and a stand-alone host program can (tests/hostsim/tweight_edit_main.cpp).
 */
#ifndef MGC_TWEIGHT_EDIT_H
#define MGC_TWEIGHT_EDIT_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

/* voxels per segment of the share plane: a wave sums one segment in a fixed order (k_tw_partials, mgc_tweight_ops.inl) */
#define MGC_TW_SEG 4096

#define MGC_TW_LIST_OK 0
#define MGC_TW_LIST_INVALID 1 /* an id outside the volume, a weight that is not finite, an id given twice */

/* what the kernels read: ids ascending and distinct, the two weights of ids[k] next to it */
struct MgcTweightList {
    std::vector<int64_t> ids;
    std::vector<double> source, sink;
    bool sorted_copy = false; /* the caller's arrays did not ascend strictly: ids / source / sink hold the sorted copy (else they are empty) */
};

static inline int64_t mgc_tw_segments(int64_t nvox) { return (nvox + MGC_TW_SEG - 1) / MGC_TW_SEG; }

/* The checks of mgc_edit_tweights: ids in [0, nvox), weights finite (negative values are allowed, as in Graph::add_tweights), no
 * id twice.  Returns MGC_TW_LIST_OK, or MGC_TW_LIST_INVALID with *bad = the index of the FIRST offending entry (of two entries
 * with one id the later one offends) and a sentence about it in msg.  Reads only.  A list in strictly ascending order, what the
 * Python layer sends, is accepted without a copy; any other comes back sorted by id in *out. */
static inline int mgc_tweight_list_check(int64_t nvox, int64_t n, const int64_t* ids, const double* source, const double* sink, MgcTweightList* out,
                                         int64_t* bad, char* msg, size_t msg_len)
{
    out->ids.clear(); out->source.clear(); out->sink.clear();
    out->sorted_copy = false;
    int64_t k1 = n;
    int code = MGC_TW_LIST_OK;
    bool ascending = true;
    for (int64_t k = 0; k < n && code == MGC_TW_LIST_OK; ++k) {
        if (ids[k] < 0 || ids[k] >= nvox) {
            code = MGC_TW_LIST_INVALID;
            snprintf(msg, msg_len, "entry %lld: id %lld outside [0, %lld)", (long long)k, (long long)ids[k], (long long)nvox);
        } else if (!isfinite(source[k]) || !isfinite(sink[k])) {
            code = MGC_TW_LIST_INVALID;
            snprintf(msg, msg_len, "entry %lld (id %lld): weights %g / %g must be finite", (long long)k, (long long)ids[k], source[k], sink[k]);
        }
        if (code != MGC_TW_LIST_OK) k1 = k;
        else if (k > 0 && !(ids[k - 1] < ids[k])) ascending = false;
    }
    if (ascending && code == MGC_TW_LIST_OK) return MGC_TW_LIST_OK;
    /* an id given twice among the entries in front of the first offender so far: the later of the two offends */
    std::vector<std::pair<int64_t, int64_t>> byid((size_t)k1);
    for (int64_t k = 0; k < k1; ++k) byid[(size_t)k] = {ids[k], k};
    std::sort(byid.begin(), byid.end());
    int64_t twice = -1;
    for (size_t k = 1; k < byid.size(); ++k)
        if (byid[k].first == byid[k - 1].first && (twice < 0 || byid[k].second < twice)) twice = byid[k].second;
    if (twice >= 0) {
        code = MGC_TW_LIST_INVALID;
        k1 = twice;
        snprintf(msg, msg_len, "entry %lld: id %lld is in the list twice", (long long)twice, (long long)ids[twice]);
    }
    if (code != MGC_TW_LIST_OK) {
        if (bad) *bad = k1;
        return code;
    }
    out->sorted_copy = true;
    out->ids.resize((size_t)n); out->source.resize((size_t)n); out->sink.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        out->ids[(size_t)k] = byid[(size_t)k].first;
        out->source[(size_t)k] = source[byid[(size_t)k].second];
        out->sink[(size_t)k] = sink[byid[(size_t)k].second];
    }
    return MGC_TW_LIST_OK;
}

/* the segments an ASCENDING list of ids touches, ascending and distinct */
static inline void mgc_tweight_list_segments(int64_t n, const int64_t* ids, std::vector<int64_t>* segs)
{
    segs->clear();
    for (int64_t k = 0; k < n; ++k) {
        const int64_t s = ids[k] / MGC_TW_SEG;
        if (segs->empty() || segs->back() != s) segs->push_back(s);
    }
}

#endif /* MGC_TWEIGHT_EDIT_H */
