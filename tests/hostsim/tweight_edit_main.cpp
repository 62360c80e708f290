/*
 * tweight_edit_main.cpp -- TEST ONLY.  The host preparation of an edit of explicit t-links by voxel list
 * (medpy_amd/csrc/mgc_tweight_edit.h) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run
 * on the CPU.  Exit status 0 = every property held; else the failed ones are printed.
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../medpy_amd/csrc/mgc_tweight_edit.h"

static int failures = 0;

static void expect(bool ok, const char* what, long long a = 0, long long b = 0)
{
    if (ok) return;
    if (++failures <= 30) printf("FAILED: %s (%lld, %lld)\n", what, a, b);
}

struct Result {
    int code;
    int64_t bad;
    std::string msg;
    MgcTweightList list;
};

static Result check(int64_t nvox, const std::vector<int64_t>& ids, const std::vector<double>& s, const std::vector<double>& k)
{
    Result r;
    char msg[256] = "";
    r.bad = -1;
    r.code = mgc_tweight_list_check(nvox, (int64_t)ids.size(), ids.data(), s.data(), k.data(), &r.list, &r.bad, msg, sizeof(msg));
    r.msg = msg;
    return r;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t nvox = 17 * 9 * 10;
    /* n = 0: accepted, nothing to sort (NULL arrays are never read) */
    {
        MgcTweightList L;
        int64_t bad = -1;
        char msg[64] = "";
        expect(mgc_tweight_list_check(nvox, 0, nullptr, nullptr, nullptr, &L, &bad, msg, sizeof(msg)) == MGC_TW_LIST_OK, "n = 0 is accepted");
        expect(!L.sorted_copy && L.ids.empty() && bad == -1, "n = 0 leaves nothing behind");
        std::vector<int64_t> segs(3, 7);
        mgc_tweight_list_segments(0, nullptr, &segs);
        expect(segs.empty(), "n = 0 touches no segment");
    }
    /* an ascending list goes through without a copy; negative weights are allowed */
    {
        const Result r = check(nvox, {0, 5, 6, nvox - 1}, {1.0, -2.0, 0.0, 3.5}, {0.0, 4.0, -1.0, 3.5});
        expect(r.code == MGC_TW_LIST_OK && !r.list.sorted_copy && r.list.ids.empty(), "ascending list accepted as it is");
    }
    /* out of range: the first offender is named */
    {
        Result r = check(nvox, {3, nvox, -1}, {1, 1, 1}, {1, 1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 1, "id == nvox refused at entry 1", r.code, r.bad);
        expect(r.msg.find("entry 1") != std::string::npos && r.msg.find(std::to_string((long long)nvox)) != std::string::npos, "the message names entry and id");
        r = check(nvox, {-1, 4}, {1, 1}, {1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 0 && r.msg.find("entry 0") != std::string::npos, "negative id refused at entry 0", r.code, r.bad);
    }
    /* not finite, either array */
    {
        Result r = check(nvox, {1, 2, 3}, {1, 1, nan}, {1, 1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 2 && r.msg.find("entry 2") != std::string::npos, "NaN source refused at entry 2", r.code, r.bad);
        r = check(nvox, {1, 2, 3}, {1, 1, 1}, {1, -inf, inf});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 1 && r.msg.find("entry 1") != std::string::npos, "-inf sink refused at entry 1", r.code, r.bad);
        expect(r.list.ids.empty() && !r.list.sorted_copy, "a refused list leaves no copy");
    }
    /* an id twice: the later of the two offends; it is found in ascending and unsorted lists, and in front of another offender */
    {
        Result r = check(nvox, {9, 4, 9, 4}, {1, 1, 1, 1}, {1, 1, 1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 2 && r.msg.find("entry 2") != std::string::npos && r.msg.find("twice") != std::string::npos,
               "duplicate refused at the first later entry", r.code, r.bad);
        r = check(nvox, {4, 4}, {1, 1}, {1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 1, "adjacent duplicate", r.code, r.bad);
        r = check(nvox, {7, 2, 7, nvox + 5}, {1, 1, 1, 1}, {1, 1, 1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 2, "a duplicate in front of a bad id is the first offender", r.code, r.bad);
        r = check(nvox, {7, nvox + 5, 2, 7}, {1, 1, 1, 1}, {1, 1, 1, 1});
        expect(r.code == MGC_TW_LIST_INVALID && r.bad == 1, "a bad id in front of a duplicate is the first offender", r.code, r.bad);
    }
    /* an unsorted list comes back sorted in a copy, the weights with their ids; the caller's arrays are not written */
    {
        std::mt19937_64 rng(20251019);
        std::vector<int64_t> ids;
        for (int64_t v = 0; v < nvox; v += 1 + (int64_t)(rng() % 7)) ids.push_back(v);
        std::shuffle(ids.begin(), ids.end(), rng);
        std::vector<double> s(ids.size()), k(ids.size());
        for (size_t i = 0; i < ids.size(); ++i) { s[i] = (double)ids[i] + 0.25; k[i] = -(double)ids[i]; }
        const std::vector<int64_t> ids0 = ids;
        const Result r = check(nvox, ids, s, k);
        expect(r.code == MGC_TW_LIST_OK && r.list.sorted_copy && r.list.ids.size() == ids.size(), "unsorted list accepted as a copy");
        bool ok = ids == ids0;
        for (size_t i = 0; ok && i < r.list.ids.size(); ++i) {
            if (i && !(r.list.ids[i - 1] < r.list.ids[i])) ok = false;
            if (r.list.source[i] != (double)r.list.ids[i] + 0.25 || r.list.sink[i] != -(double)r.list.ids[i]) ok = false;
        }
        expect(ok, "the copy ascends strictly and keeps the weights with their ids");
        /* the segments of the sorted ids: ascending, distinct, exactly those that hold an id */
        std::vector<int64_t> segs;
        mgc_tweight_list_segments((int64_t)r.list.ids.size(), r.list.ids.data(), &segs);
        std::vector<char> want((size_t)mgc_tw_segments(nvox), 0);
        for (int64_t v : ids) want[(size_t)(v / MGC_TW_SEG)] = 1;
        size_t nwant = 0;
        for (char c : want) nwant += c ? 1 : 0;
        ok = segs.size() == nwant;
        for (size_t i = 0; ok && i < segs.size(); ++i) ok = want[(size_t)segs[i]] && (i == 0 || segs[i - 1] < segs[i]);
        expect(ok, "touched segments");
    }
    /* segments at the borders of a volume that is no multiple of a segment */
    {
        const int64_t n2 = 3 * MGC_TW_SEG + 5;
        expect(mgc_tw_segments(n2) == 4 && mgc_tw_segments(MGC_TW_SEG) == 1 && mgc_tw_segments(1) == 1, "segment count");
        const std::vector<int64_t> ids = {0, MGC_TW_SEG - 1, MGC_TW_SEG, 3 * MGC_TW_SEG, n2 - 1};
        std::vector<int64_t> segs;
        mgc_tweight_list_segments((int64_t)ids.size(), ids.data(), &segs);
        expect(segs == std::vector<int64_t>({0, 1, 3}), "segments of ids at segment borders");
    }
    if (failures) printf("%d properties failed\n", failures);
    else printf("tweight_edit: all properties held\n");
    return failures ? 1 : 0;
}
