/*
 * msg_list_check.h -- the host-side check of a msg_update_tweights call (include/medpy_hip.h), done before the first write so
 * that a refused call leaves the handle as it was: the rule mgc_edit_markers follows.  Plain C++, no HIP: msg_sparse.hip
 * includes it, and a stand-alone host program can (tests/hostsim/msg_list_check_main.cpp).
 */
#ifndef MSG_LIST_CHECK_H
#define MSG_LIST_CHECK_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

/* 0 = accepted, 1 = refused (`err` says why).  ids == NULL: the whole vector, n == nodes (or n == 0: nothing).  A list that does not
 * ascend strictly comes back sorted by id in sorted_ids / sorted_tr (left empty when the caller's own arrays are in order). */
static inline int msg_check_tweight_list_impl(int64_t nodes, int64_t n, const int64_t* ids, const double* tr, double flow_const,
                                              std::vector<int64_t>* sorted_ids, std::vector<double>* sorted_tr, std::string& err)
{
    char buf[256];
    sorted_ids->clear();
    sorted_tr->clear();
    if (n < 0 || (n > 0 && !tr) || (!ids && n != 0 && n != nodes)) {
        snprintf(buf, sizeof(buf), "msg_update_tweights: n = %lld (ids NULL: the whole vector of %lld nodes), tr NULL", (long long)n, (long long)nodes);
        err = buf;
        return 1;
    }
    if (!isfinite(flow_const)) { err = "msg_update_tweights: the flow constant is not finite"; return 1; }
    bool ascending = true;
    for (int64_t k = 0; k < n; ++k) {
        if (ids && (ids[k] < 0 || ids[k] >= nodes)) {
            snprintf(buf, sizeof(buf), "msg_update_tweights: entry %lld: id %lld outside [0, %lld)", (long long)k, (long long)ids[k], (long long)nodes);
            err = buf;
            return 1;
        }
        if (!isfinite(tr[k])) {
            snprintf(buf, sizeof(buf), "msg_update_tweights: entry %lld: the t-link is not finite", (long long)k);
            err = buf;
            return 1;
        }
        if (ids && k > 0 && !(ids[k - 1] < ids[k])) ascending = false;
    }
    if (ascending) return 0;
    std::vector<std::pair<int64_t, int64_t>> byid((size_t)n);
    for (int64_t k = 0; k < n; ++k) byid[(size_t)k] = {ids[k], k};
    std::sort(byid.begin(), byid.end());
    for (int64_t k = 1; k < n; ++k)
        if (byid[(size_t)k].first == byid[(size_t)k - 1].first) {
            snprintf(buf, sizeof(buf), "msg_update_tweights: entry %lld: id %lld is in the list twice", (long long)byid[(size_t)k].second, (long long)byid[(size_t)k].first);
            err = buf;
            return 1;
        }
    sorted_ids->resize((size_t)n);
    sorted_tr->resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        (*sorted_ids)[(size_t)k] = byid[(size_t)k].first;
        (*sorted_tr)[(size_t)k] = tr[byid[(size_t)k].second];
    }
    return 0;
}

#endif /* MSG_LIST_CHECK_H */
