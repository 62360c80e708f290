/*
 * sparse_reach_main.cpp -- TEST ONLY, stand-alone (its own main, no library, no GPU; also built with -fsanitize=address,undefined).
 * The node operations of medpy_amd/csrc/msg_reach_ops.inl on random DIRECTED residual graphs: residuals, capacities as built and t-link
 * residuals drawn independently per direction from zeros, dust (2^-80), whole numbers and fractions; rows without arcs, isolated
 * nodes, no node pair twice.  Per case and tolerance:
 *   - the scale, the open bytes and the seeds against the rule written out here a second time, arc by arc;
 *   - bit 1 of an arc's byte is bit 0 of its reverse arc's;
 *   - the flood with the nodes visited ascending, descending and in random permutations, to the fixpoint: identical marks each way,
 *     equal to a plain breadth-first search, forward and backward;
 *   - the backward flood equals the forward flood run on the transposed bits;
 *   - the read-out planes and their counts.
 * Prints "<cases> cases, <k> floods of more than one pass, <failed> failed"; exit status 1 when something failed.
 */
#include <algorithm>
#include <math.h>
#include <queue>
#include <random>
#include <set>
#include <stdint.h>
#include <stdio.h>
#include <utility>
#include <vector>

#include "../../medpy_amd/csrc/msg_reach_ops.inl"

namespace {

const double DUST = 1.0 / 1208925819614629174706176.0; /* 2^-80 */
const double ULP64 = 64.0 / 4503599627370496.0;        /* 64 * 2^-52 */

struct Case {
    int64_t n = 0, arcs = 0;
    std::vector<int64_t> row, rev;
    std::vector<int32_t> head, tail, height;
    std::vector<double> rcap, cap0, excess, sink, tr;
    bool has_tr = true;
};

double draw(std::mt19937_64& rng)
{
    switch (rng() % 6) {
    case 0: return 0.0;
    case 1: return DUST;
    case 2: return (double)(1 + rng() % 4);
    case 3: return (double)(rng() % 1000) / 64.0;
    case 4: return ldexp((double)(1 + rng() % 7), -60);
    default: return 0.0;
    }
}

Case make_case(std::mt19937_64& rng)
{
    Case c;
    c.n = 1 + (int64_t)(rng() % 60);
    const int64_t live = 1 + (int64_t)(rng() % c.n); /* nodes >= live stay isolated */
    std::set<std::pair<int32_t, int32_t>> pairs;
    const int64_t want = live < 2 ? 0 : (int64_t)(rng() % (3 * live));
    for (int64_t k = 0; k < want; ++k) {
        const int32_t a = (int32_t)(rng() % live), b = (int32_t)(rng() % live);
        if (a != b && !(rng() % 7 == 0 && a % 5 == 0)) pairs.insert({std::min(a, b), std::max(a, b)}); /* some nodes get fewer arcs: empty rows among filled ones */
    }
    std::vector<std::pair<int32_t, int32_t>> arcs;
    for (const auto& p : pairs) { arcs.push_back(p); arcs.push_back({p.second, p.first}); }
    std::sort(arcs.begin(), arcs.end());
    c.arcs = (int64_t)arcs.size();
    c.row.assign((size_t)c.n + 1, 0);
    for (const auto& a : arcs) { c.tail.push_back(a.first); c.head.push_back(a.second); c.row[(size_t)a.first + 1]++; }
    for (int64_t u = 0; u < c.n; ++u) c.row[u + 1] += c.row[u];
    c.rev.assign((size_t)c.arcs, 0);
    for (int64_t a = 0; a < c.arcs; ++a)
        c.rev[a] = std::lower_bound(arcs.begin(), arcs.end(), std::make_pair(c.head[a], c.tail[a])) - arcs.begin();
    for (int64_t a = 0; a < c.arcs; ++a) { c.rcap.push_back(draw(rng)); c.cap0.push_back(draw(rng)); }
    c.has_tr = rng() % 4 != 0;
    for (int64_t u = 0; u < c.n; ++u) {
        c.excess.push_back(rng() % 3 == 0 ? draw(rng) : 0.0);
        c.sink.push_back(rng() % 3 == 0 ? draw(rng) : 0.0);
        c.tr.push_back(draw(rng) * (rng() % 2 ? 1.0 : -1.0));
        c.height.push_back(rng() % 2 ? MSG_HINF : (int32_t)(1 + rng() % 9));
    }
    return c;
}

struct Planes {
    std::vector<double> scale;
    std::vector<uint8_t> open, mark0, mark1, to, amb, nts;
    int32_t count[4] = {0, 0, 0, 0};
};

MsgReach bind(const Case& c, Planes& p, bool use_tol, double tol)
{
    p.scale.assign((size_t)c.n, -1.0);
    p.open.assign((size_t)(c.arcs ? c.arcs : 1), 0xff);
    p.mark0.assign((size_t)c.n, 0xff); p.mark1.assign((size_t)c.n, 0xff);
    p.to.assign((size_t)c.n, 0xff); p.amb.assign((size_t)c.n, 0xff); p.nts.assign((size_t)c.n, 0xff);
    MsgReach R;
    R.nodes = c.n; R.arcs = c.arcs; R.row = c.row.data(); R.head = c.head.data(); R.rev = c.rev.data(); R.rcap = c.rcap.data(); R.cap0 = c.cap0.data();
    R.excess = c.excess.data(); R.sink = c.sink.data(); R.tr = c.has_tr ? c.tr.data() : nullptr; R.height = c.height.data();
    R.use_tol = use_tol ? 1 : 0; R.tol = tol;
    R.scale = p.scale.data(); R.open = p.open.data(); R.mark[0] = p.mark0.data(); R.mark[1] = p.mark1.data();
    R.to_sink = p.to.data(); R.ambiguous = p.amb.data(); R.not_to_sink = p.nts.data(); R.count = p.count;
    return R;
}

/* the rule a second time, without the node operations */
double ref_scale(const Case& c, int64_t v)
{
    double s = 0.0;
    for (int64_t a = c.row[v]; a < c.row[v + 1]; ++a) s = std::max(s, c.cap0[a] + c.cap0[c.rev[a]]);
    return s;
}

bool ref_open(const Case& c, int64_t a, bool use_tol, double tol)
{
    if (!(c.rcap[a] > 0.0)) return false;
    if (!use_tol || tol == 0.0) return true;
    return c.rcap[a] > tol * std::max(ref_scale(c, c.tail[a]), ref_scale(c, c.head[a]));
}

bool ref_seed(const Case& c, int64_t v, bool back, bool use_tol, double tol)
{
    const double x = back ? c.sink[v] : c.excess[v];
    if (!(x > 0.0)) return false;
    if (!use_tol || tol == 0.0) return true;
    return x > tol * std::max(c.has_tr ? fabs(c.tr[v]) : 0.0, ref_scale(c, v));
}

std::vector<uint8_t> ref_bfs(const Case& c, bool back, bool use_tol, double tol)
{
    std::vector<uint8_t> m((size_t)c.n, 0);
    std::queue<int64_t> q;
    for (int64_t v = 0; v < c.n; ++v)
        if (ref_seed(c, v, back, use_tol, tol)) { m[v] = 1; q.push(v); }
    while (!q.empty()) {
        const int64_t u = q.front();
        q.pop();
        for (int64_t a = c.row[u]; a < c.row[u + 1]; ++a) {
            const int64_t w = c.head[a];
            /* forward: along u -> w; backward: w joins when ITS arc w -> u is open */
            if (!m[w] && ref_open(c, back ? c.rev[a] : a, use_tol, tol)) { m[w] = 1; q.push(w); }
        }
    }
    return m;
}

/* passes over the nodes in `order` until one marks nothing; returns the passes that marked something */
template <bool BACK>
int flood(const MsgReach& R, const std::vector<int64_t>& order)
{
    int productive = 0;
    for (;;) {
        bool ch = false;
        for (int64_t v : order) ch |= msg_reach_pass_node<BACK>(R, v);
        if (!ch) return productive;
        productive++;
    }
}

int failed = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            failed++;                     \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

} // namespace

int main()
{
    std::mt19937_64 rng(20240613);
    const double tols[4] = {-1.0, 0.0, ULP64, 1e-6};
    int cases = 0, long_floods = 0;
    for (int t = 0; t < 400; ++t) {
        const Case c = make_case(rng);
        for (int ti = 0; ti < 4; ++ti) {
            const bool use_tol = tols[ti] >= 0.0;
            const double tol = use_tol ? tols[ti] : 0.0;
            cases++;
            Planes p;
            const MsgReach R = bind(c, p, use_tol, tol);
            if (use_tol)
                for (int64_t v = 0; v < c.n; ++v) {
                    const double s = msg_reach_scale_node(R, v);
                    CHECK(s == ref_scale(c, v) && p.scale[v] == s, "case %d tol %g: scale of node %lld", t, tols[ti], (long long)v);
                }
            int64_t closed = 0, ref_closed = 0;
            for (int64_t v = c.n - 1; v >= 0; --v) closed += msg_reach_open_node(R, v);
            for (int64_t a = 0; a < c.arcs; ++a) {
                const bool o = ref_open(c, a, use_tol, tol);
                ref_closed += c.rcap[a] > 0.0 && !o;
                CHECK((p.open[a] & 1) == (o ? 1 : 0) && p.open[a] < 4, "case %d tol %g: open bit of arc %lld", t, tols[ti], (long long)a);
                CHECK(((p.open[a] >> 1) & 1) == (p.open[c.rev[a]] & 1), "case %d tol %g: bit 1 of arc %lld is not bit 0 of its reverse", t, tols[ti], (long long)a);
            }
            CHECK(closed == ref_closed, "case %d tol %g: %lld arcs closed, expected %lld", t, tols[ti], (long long)closed, (long long)ref_closed);
            const std::vector<uint8_t> want_f = ref_bfs(c, false, use_tol, tol), want_b = ref_bfs(c, true, use_tol, tol);
            std::vector<int64_t> order((size_t)c.n);
            for (int64_t v = 0; v < c.n; ++v) order[v] = v;
            for (int variant = 0; variant < 5; ++variant) {
                if (variant == 1) std::reverse(order.begin(), order.end());
                if (variant >= 2) std::shuffle(order.begin(), order.end(), rng);
                for (int64_t v : order) {
                    const int kf = msg_reach_seed_node<false>(R, v), kb = msg_reach_seed_node<true>(R, v);
                    CHECK((kf == 1) == ref_seed(c, v, false, use_tol, tol) && (kf == 0) == !(c.excess[v] > 0.0), "case %d tol %g: source seed of node %lld", t, tols[ti], (long long)v);
                    CHECK((kb == 1) == ref_seed(c, v, true, use_tol, tol) && (kb == 0) == !(c.sink[v] > 0.0), "case %d tol %g: sink seed of node %lld", t, tols[ti], (long long)v);
                }
                const int pf = flood<false>(R, order), pb = flood<true>(R, order);
                if (variant == 0) long_floods += (pf > 1) + (pb > 1);
                CHECK(p.mark0 == want_f, "case %d tol %g order %d: the forward flood is not the breadth-first search", t, tols[ti], variant);
                CHECK(p.mark1 == want_b, "case %d tol %g order %d: the backward flood is not the breadth-first search", t, tols[ti], variant);
            }
            /* the backward flood is the forward flood on the transposed bits */
            {
                Planes q;
                MsgReach T = bind(c, q, use_tol, tol);
                for (int64_t a = 0; a < c.arcs; ++a) q.open[a] = (uint8_t)(((p.open[a] & 1) << 1) | ((p.open[a] >> 1) & 1));
                for (int64_t v = 0; v < c.n; ++v) q.mark0[v] = ref_seed(c, v, true, use_tol, tol) ? 1 : 0;
                flood<false>(T, order);
                CHECK(q.mark0 == p.mark1, "case %d tol %g: backward flood != forward flood on the transposed bits", t, tols[ti]);
            }
            int64_t nf = 0, nt = 0, na = 0;
            for (int64_t v = 0; v < c.n; ++v) {
                const int k = msg_reach_readout_node(R, v);
                const int f = want_f[v], to = use_tol ? want_b[v] : (c.height[v] < MSG_HINF ? 1 : 0);
                nf += k & 1; nt += (k >> 1) & 1; na += (k >> 2) & 1;
                CHECK(k == (f | (to << 1) | ((f | to) ? 0 : 4)) && p.to[v] == to && p.nts[v] == 1 - to && p.amb[v] == ((f | to) ? 0 : 1),
                      "case %d tol %g: read-out of node %lld", t, tols[ti], (long long)v);
            }
            CHECK(nf + na + nt - (int64_t)std::count_if(order.begin(), order.end(), [&](int64_t v) { return p.mark0[v] && p.to[v]; }) == c.n,
                  "case %d tol %g: the counts do not add up", t, tols[ti]);
        }
    }
    printf("%d cases, %d floods of more than one pass, %d failed\n", cases, long_floods, failed);
    return failed ? 1 : 0;
}
