/*
 * msg_list_check_main.cpp -- TEST ONLY.  The host-side check of a msg_update_tweights list (medpy_amd/csrc/msg_list_check.h: ids in
 * range, values finite, sorted in a copy, no id twice) as a stand-alone program, so that it can also be built with
 * -fsanitize=address,undefined and run on the CPU.  Exit status 0 = every case behaved; else the failed cases are printed.
 */
#include <limits>
#include <random>

#include "../../medpy_amd/csrc/msg_list_check.h"

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) { printf("FAILED: %s\n", what); ++failures; }
}

static int run(int64_t nodes, const std::vector<int64_t>& ids, const std::vector<double>& tr, double fc, std::vector<int64_t>* si, std::vector<double>* st,
               bool whole = false)
{
    std::string err;
    const int rc = msg_check_tweight_list_impl(nodes, (int64_t)tr.size(), whole ? nullptr : ids.data(), tr.data(), fc, si, st, err);
    if (rc && err.empty()) { printf("FAILED: refused without a message\n"); ++failures; }
    return rc;
}

int main()
{
    std::vector<int64_t> si;
    std::vector<double> st;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    expect(run(10, {}, {}, 0.0, &si, &st) == 0 && si.empty(), "an empty list is accepted");
    expect(run(10, {1, 4, 9}, {1.0, -2.0, 0.0}, 0.5, &si, &st) == 0 && si.empty() && st.empty(), "an ascending list is used as it is");
    expect(run(10, {9, 1, 4}, {9.0, 1.0, 4.0}, 0.5, &si, &st) == 0 && si == std::vector<int64_t>({1, 4, 9}) && st == std::vector<double>({1.0, 4.0, 9.0}),
           "a list out of order is sorted in a copy, values with their ids");
    expect(run(10, {1, 10}, {1.0, 1.0}, 0.0, &si, &st) == 1 && si.empty(), "id == nodes is refused");
    expect(run(10, {-1, 2}, {1.0, 1.0}, 0.0, &si, &st) == 1, "a negative id is refused");
    expect(run(10, {3, 3}, {1.0, 1.0}, 0.0, &si, &st) == 1, "an id twice in a row is refused");
    expect(run(10, {3, 5, 3}, {1.0, 1.0, 2.0}, 0.0, &si, &st) == 1 && si.empty(), "an id twice, apart, is refused");
    expect(run(10, {3, 5}, {1.0, nan}, 0.0, &si, &st) == 1, "NaN is refused");
    expect(run(10, {3, 5}, {-inf, 1.0}, 0.0, &si, &st) == 1, "an infinite t-link is refused");
    expect(run(10, {3, 5}, {1.0, 1.0}, nan, &si, &st) == 1, "a flow constant that is not finite is refused");
    expect(run(3, {}, {1.0, 2.0, 3.0}, 0.0, &si, &st, true) == 0 && si.empty(), "the whole vector, ids NULL");
    expect(run(4, {}, {1.0, 2.0, 3.0}, 0.0, &si, &st, true) == 1, "ids NULL with n != nodes is refused");
    expect(run(3, {}, {1.0, nan, 3.0}, 0.0, &si, &st, true) == 1, "the whole vector with NaN is refused");
    {
        std::string err;
        const int64_t one = 1;
        expect(msg_check_tweight_list_impl(10, 1, &one, nullptr, 0.0, &si, &st, err) == 1, "tr NULL is refused");
        expect(msg_check_tweight_list_impl(10, -1, &one, nullptr, 0.0, &si, &st, err) == 1, "n < 0 is refused");
    }
    /* a long shuffled list: sorted, every value still with its id; one id doubled: refused */
    std::mt19937_64 rng(7);
    const int64_t nodes = 100000;
    std::vector<int64_t> ids;
    for (int64_t u = 0; u < nodes; u += 3) ids.push_back(u);
    std::shuffle(ids.begin(), ids.end(), rng);
    std::vector<double> tr(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) tr[k] = 0.25 * (double)ids[k] - 7.0;
    bool ok = run(nodes, ids, tr, 1.0, &si, &st) == 0 && si.size() == ids.size();
    for (size_t k = 0; ok && k < si.size(); ++k) ok = (k == 0 || si[k - 1] < si[k]) && st[k] == 0.25 * (double)si[k] - 7.0;
    expect(ok, "100000 / 3 shuffled ids come back ascending with their values");
    ids.back() = ids.front();
    expect(run(nodes, ids, tr, 1.0, &si, &st) == 1 && si.empty(), "one id doubled in the long list is refused");
    if (!failures) printf("msg_list_check: all cases passed\n");
    return failures ? 1 : 0;
}
