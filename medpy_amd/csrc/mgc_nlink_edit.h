/*
 * mgc_nlink_edit.h -- host preparation of an edit of n-links by arc list (mgc_edit_nweights; DESIGN 10, "Edits of n-links by
 * list"): the list is checked, every pair becomes two HALF-ARCS -- the arc as its tail sees it, and the reverse arc as the head
 * sees it -- and the half-arcs are sorted by (tile, voxel, direction), so that the arcs of one voxel lie next to each other and the
 * arcs of one tile form one range.  Plain C++, no HIP: mgc_kernels.hip includes it, and a stand-alone host program can
 * (tests/hostsim/nlink_edit_main.cpp).
 */
#ifndef MGC_NLINK_EDIT_H
#define MGC_NLINK_EDIT_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "mgc_common.h"

#define MGC_EDIT_OK 0
#define MGC_EDIT_INVALID 1        /* an id outside the volume, a capacity that is not finite and >= 0, a pair given twice */
#define MGC_EDIT_NOT_NEIGHBOURS 2 /* (i, j) do not join neighbours of the lattice */

/* what k_edit_gather / k_edit_nlinks read (mgc_nlink_edit_ops.inl); half-arc k of the sorted order:
 *   slot[k]     index of the arc in rcap / cap0: (tile * ndir + direction) * 512 + voxel of the tile
 *   partner[k]  position of the reverse arc's half-arc
 *   c_out1[k], c_in1[k]  new capacity of the arc and of its reverse
 * and the touched tiles, ascending: the half-arcs of tile[m] are [begin[m], begin[m + 1]). */
struct MgcEditPlan {
    std::vector<int64_t> slot;
    std::vector<int32_t> partner;
    std::vector<double> c_out1, c_in1;
    std::vector<int32_t> tile, begin;
};

static inline int mgc_edit_reverse(int ndir, int d) { return ndir == 6 ? (d ^ 1) : (25 - d); }

/* The checks of mgc_edit_nweights, entry by entry: ids in [0, nvox), (i, j) neighbours of the lattice, capacities finite and >= 0
 * (rev NULL: rev = cap), no unordered pair twice.  Returns MGC_EDIT_OK, or the code of the FIRST offending entry with *bad = its
 * index and a sentence about it in msg.  Reads only; L needs its extents, tile grid and ndir. */
static inline int mgc_edit_check(const MgcLattice& L, int64_t n, const int64_t* i, const int64_t* j, const double* cap, const double* rev, int64_t* bad,
                                 char* msg, size_t msg_len)
{
    int64_t k1 = n;
    int code = MGC_EDIT_OK;
    for (int64_t k = 0; k < n && code == MGC_EDIT_OK; ++k) {
        const double a = cap[k], b = rev ? rev[k] : cap[k];
        if (i[k] < 0 || j[k] < 0 || i[k] >= L.nvox || j[k] >= L.nvox) {
            code = MGC_EDIT_INVALID;
            snprintf(msg, msg_len, "entry %lld joins nodes %lld and %lld outside [0, %lld)", (long long)k, (long long)i[k], (long long)j[k], (long long)L.nvox);
        } else if (mgc_arc_direction(L, i[k], j[k]) < 0) {
            code = MGC_EDIT_NOT_NEIGHBOURS;
            snprintf(msg, msg_len, "entry %lld (%lld, %lld) does not join neighbours of the %d-neighbourhood lattice", (long long)k, (long long)i[k], (long long)j[k], L.ndir);
        } else if (!(a >= 0.0 && a <= 1.7976931348623157e308) || !(b >= 0.0 && b <= 1.7976931348623157e308)) {
            code = MGC_EDIT_INVALID;
            snprintf(msg, msg_len, "entry %lld (%lld, %lld): capacities %g / %g must be finite and >= 0", (long long)k, (long long)i[k], (long long)j[k], a, b);
        }
        if (code != MGC_EDIT_OK) k1 = k;
    }
    /* a pair given twice, in either orientation, among the entries in front of that one: the later of the two offends */
    std::vector<std::pair<std::pair<int64_t, int64_t>, int64_t>> pairs((size_t)k1);
    for (int64_t k = 0; k < k1; ++k) pairs[(size_t)k] = {{std::min(i[k], j[k]), std::max(i[k], j[k])}, k};
    std::sort(pairs.begin(), pairs.end());
    int64_t twice = -1;
    for (size_t k = 1; k < pairs.size(); ++k)
        if (pairs[k].first == pairs[k - 1].first && (twice < 0 || pairs[k].second < twice)) twice = pairs[k].second;
    if (twice >= 0) {
        code = MGC_EDIT_INVALID;
        k1 = twice;
        snprintf(msg, msg_len, "entry %lld: the pair (%lld, %lld) is in the list twice", (long long)twice, (long long)i[twice], (long long)j[twice]);
    }
    if (code != MGC_EDIT_OK && bad) *bad = k1;
    return code;
}

/* the plan of a list that mgc_edit_check let through (n < 2^30) */
static inline void mgc_edit_plan(const MgcLattice& L, int64_t n, const int64_t* i, const int64_t* j, const double* cap, const double* rev, MgcEditPlan* P)
{
    struct Half { int64_t key; int64_t slot; double c_out1, c_in1; };
    std::vector<Half> hs((size_t)(2 * n));
    for (int64_t k = 0; k < n; ++k) {
        const int d = mgc_arc_direction(L, i[k], j[k]), dr = mgc_edit_reverse(L.ndir, d);
        const double a = cap[k], b = rev ? rev[k] : cap[k];
        int ti, li, tj, lj;
        mgc_node_to_tile(L, i[k], ti, li);
        mgc_node_to_tile(L, j[k], tj, lj);
        hs[(size_t)(2 * k)] = {((int64_t)ti * MGC_TV + li) * 32 + d, ((int64_t)ti * L.ndir + d) * MGC_TV + li, a, b};
        hs[(size_t)(2 * k + 1)] = {((int64_t)tj * MGC_TV + lj) * 32 + dr, ((int64_t)tj * L.ndir + dr) * MGC_TV + lj, b, a};
    }
    std::vector<int32_t> order(hs.size()), where(hs.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int32_t)k;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hs[(size_t)a].key < hs[(size_t)b].key; }); /* (no key twice: no pair twice) */
    for (size_t k = 0; k < order.size(); ++k) where[(size_t)order[k]] = (int32_t)k;
    const size_t m = hs.size();
    P->slot.resize(m); P->partner.resize(m); P->c_out1.resize(m); P->c_in1.resize(m);
    P->tile.clear(); P->begin.clear();
    for (size_t k = 0; k < m; ++k) {
        const Half& h = hs[(size_t)order[k]];
        P->slot[k] = h.slot;
        P->partner[k] = where[(size_t)order[k] ^ 1u];
        P->c_out1[k] = h.c_out1;
        P->c_in1[k] = h.c_in1;
        const int32_t tile = (int32_t)(h.key / (32 * MGC_TV));
        if (P->tile.empty() || P->tile.back() != tile) { P->tile.push_back(tile); P->begin.push_back((int32_t)k); }
    }
    P->begin.push_back((int32_t)m);
}

#endif /* MGC_NLINK_EDIT_H */
