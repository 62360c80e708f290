/*
 * nlink_edit_main.cpp -- TEST ONLY.  The directed per-arc rule of an edit of n-links by arc list (medpy_amd/csrc/mgc_nlink_fold.h,
 * mgc_nlink_fold_directed) and the host preparation of such an edit (medpy_amd/csrc/mgc_nlink_edit.h) as a stand-alone program, so
 * that both can be built with -fsanitize=address,undefined and run on the CPU.  Exit status 0 = every property held; else the failed
 * ones are printed (the first few cases each).
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../medpy_amd/csrc/mgc_nlink_fold.h"
#include "../../medpy_amd/csrc/mgc_nlink_edit.h"

static int failures = 0;

static void expect(bool ok, const char* what, double a = 0.0, double b = 0.0, double c = 0.0, double d = 0.0)
{
    if (ok) return;
    if (++failures <= 30) printf("FAILED: %s (%.17g, %.17g, %.17g, %.17g)\n", what, a, b, c, d);
}

/* ---- the rule ---- */

/* capacities from the floor sys.float_info.min up to the marker weight, log-uniform, the two ends included; `zero`: 0 among them */
static double capacity(std::mt19937_64& rng, bool zero)
{
    const double lo = log(1e-308), hi = log(65535.0);
    const int pick = (int)(rng() % 16);
    if (pick == 0) return 1e-308;
    if (pick == 1) return 65535.0;
    if (pick == 2) return 1.0;
    if (pick == 3 && zero) return 0.0;
    return exp(lo + (hi - lo) * std::uniform_real_distribution<double>(0.0, 1.0)(rng));
}

/* a flow the pair (c_out, c_in) can carry: saturated either way, none, anything between */
static double flow_on(std::mt19937_64& rng, double c_out, double c_in)
{
    switch (rng() % 6) {
    case 0: return c_out;
    case 1: return -c_in;
    case 2: return 0.0;
    default: {
        const double u = std::uniform_real_distribution<double>(-1.0, 1.0)(rng);
        return u >= 0.0 ? u * c_out : u * c_in;
    }
    }
}

static void rule_cases()
{
    std::mt19937_64 rng(20250917);
    for (int k = 0; k < 400000; ++k) {
        const double co = capacity(rng, true), ci = capacity(rng, true), phi = flow_on(rng, co, ci);
        const double r0 = co - phi; /* what the solver holds: in [0, c_out + c_in] */
        bool clamped = true;
        { /* both capacities unchanged: the residual keeps its bits, nothing comes back */
            double r = r0;
            const double back = mgc_nlink_fold_directed(co, ci, co, ci, &r, &clamped);
            expect(mgc_same_bits(r, r0) && back == 0.0 && !clamped, "unchanged capacities touch nothing", co, ci, phi);
        }
        /* new capacities: independent, or near the old ones, or 0 (a barrier, a one-way arc): the flow ends up inside, at and beyond both bounds */
        double co1 = (k & 1) ? capacity(rng, true) : co * exp(std::uniform_real_distribution<double>(-3.0, 3.0)(rng));
        double ci1 = (k & 2) ? capacity(rng, true) : ci * exp(std::uniform_real_distribution<double>(-3.0, 3.0)(rng));
        if (!std::isfinite(co1) || !std::isfinite(ci1)) continue;
        if (mgc_same_bits(co, co1) && mgc_same_bits(ci, ci1)) continue;
        double r = r0;
        const double back = mgc_nlink_fold_directed(co, ci, co1, ci1, &r, &clamped);
        const double seen = co - r0; /* the flow as the rule sees it */
        expect(r >= 0.0 && r <= co1 + ci1, "0 <= r' <= c_out' + c_in'", co, ci, co1, ci1);
        if (seen >= -ci1 && seen <= co1) {
            expect(back == 0.0 && !clamped, "a flow inside the new bounds gives back exactly 0", co, ci, co1, ci1);
            expect(r == co1 - seen, "r' = c_out' - phi", co, ci, co1, ci1);
        } else {
            expect(clamped && back != 0.0 && (back > 0.0) == (seen > 0.0), "a flow outside the new bounds comes back with its sign", co, ci, co1, ci1);
            expect(r == (seen > 0.0 ? 0.0 : co1 + ci1), "a clamped arc is saturated one way or the other", co, ci, co1, ci1);
            expect(back == seen - (seen > 0.0 ? co1 : -ci1), "what comes back is phi - phi'", co, ci, co1, ci1);
        }
    }
    /* symmetric inputs: bit for bit the symmetric rule, flows beyond both bounds and the unchanged capacity included */
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 400000; ++k) {
        double c = capacity(rng, false), c1 = (k & 1) ? capacity(rng, false) : c * exp(std::uniform_real_distribution<double>(-3.0, 3.0)(rng));
        if (k % 7 == 0) c1 = c;
        if (k % 1001 == 0) c = nan;
        if (k % 1003 == 0) c1 = nan;
        const double phi = (c == c ? c : 1.0) * std::uniform_real_distribution<double>(-1.5, 1.5)(rng);
        double ra = c - phi, rb = ra;
        if (k % 1001 == 0 && (k & 4)) ra = rb = phi; /* (a residual that is a number under a capacity that is not) */
        bool ca, cb;
        const double back_a = mgc_nlink_fold(c, c1, &ra, &ca), back_b = mgc_nlink_fold_directed(c, c, c1, c1, &rb, &cb);
        expect(mgc_same_bits(ra, rb) && mgc_same_bits(back_a, back_b) && ca == cb, "symmetric inputs: the result of mgc_nlink_fold, bit for bit", c, c1, phi);
    }
    /* dyadic inputs: every operation of the rule is exact, so the two ends of a pair -- each from its own residual -- hand back equal and
     * opposite amounts and the pair keeps r'_ab + r'_ba == c'_ab + c'_ba */
    for (int k = 0; k < 400000; ++k) {
        auto dy = [&](bool zero) { const uint64_t v = rng() % 4097; return (double)(zero ? v : 1 + v % 4096) / 64.0; };
        const double cab = dy(false), cba = dy(false), cab1 = dy(true), cba1 = dy(true);
        const int64_t up = (int64_t)(cab * 64.0), down = (int64_t)(cba * 64.0);
        double phi = (double)((int64_t)(rng() % (uint64_t)(up + down + 1)) - down) / 64.0; /* in [-c_ba, c_ab] */
        if (rng() % 5 == 0) phi = (rng() & 1) ? cab : -cba;
        double rab = cab - phi, rba = cba + phi;
        expect(rab + rba == cab + cba, "(the case conserves the pair exactly)", cab, cba, phi);
        bool ca, cb;
        const double back_a = mgc_nlink_fold_directed(cab, cba, cab1, cba1, &rab, &ca), back_b = mgc_nlink_fold_directed(cba, cab, cba1, cab1, &rba, &cb);
        expect(back_a == -back_b && ca == cb, "the two ends hand back equal and opposite amounts", cab, cba, cab1, cba1);
        expect((cab == cab1 && cba == cba1) || rab + rba == cab1 + cba1, "r'_ab + r'_ba == c'_ab + c'_ba", cab, cba, cab1, cba1);
        expect(rab >= 0.0 && rba >= 0.0, "no negative residual", cab, cba, cab1, cba1);
    }
}

/* ---- the host preparation ---- */

static MgcLattice lattice(int ndim, const int64_t* shape, int connectivity)
{
    MgcLattice L;
    memset(&L, 0, sizeof(L));
    int64_t s[3] = {1, 1, 1};
    for (int k = 0; k < ndim; ++k) s[3 - ndim + k] = shape[k];
    L.dz = s[0]; L.dy = s[1]; L.dx = s[2];
    L.nvox = s[0] * s[1] * s[2];
    L.gz = (int)((s[0] + 7) / 8); L.gy = (int)((s[1] + 7) / 8); L.gx = (int)((s[2] + 7) / 8);
    L.ntiles = L.gz * L.gy * L.gx;
    L.tz_own_hi = L.gz;
    L.ndir = connectivity == 2 * ndim ? 6 : 26;
    return L;
}

static int64_t node(const MgcLattice& L, int64_t z, int64_t y, int64_t x) { return (z * L.dy + y) * L.dx + x; }

/* offset (z, y, x) -> direction index, as mgc_add_nweights encodes it */
static int direction_of(int ndir, int oz, int oy, int ox)
{
    if (ndir == 6) return ox ? (ox > 0 ? 1 : 0) : (oy ? (oy > 0 ? 3 : 2) : (oz > 0 ? 5 : 4));
    const int c = (oz + 1) * 9 + (oy + 1) * 3 + (ox + 1);
    return c < 13 ? c : c - 1;
}

struct Call {
    std::vector<int64_t> i, j;
    std::vector<double> cap, rev;
    void add(int64_t a, int64_t b, double c, double r) { i.push_back(a); j.push_back(b); cap.push_back(c); rev.push_back(r); }
};

static int check(const MgcLattice& L, const Call& c, bool with_rev, int64_t* bad, std::string* msg)
{
    char buf[256] = "";
    *bad = -1;
    const int code = mgc_edit_check(L, (int64_t)c.i.size(), c.i.data(), c.j.data(), c.cap.data(), with_rev ? c.rev.data() : nullptr, bad, buf, sizeof(buf));
    *msg = buf;
    return code;
}

static void expect_refused(const MgcLattice& L, const Call& c, bool with_rev, int code, int64_t entry, const char* what)
{
    int64_t bad;
    std::string msg;
    const int got = check(L, c, with_rev, &bad, &msg);
    char name[32];
    snprintf(name, sizeof(name), "entry %lld", (long long)entry);
    if (!(got == code && bad == entry && msg.find(name) != std::string::npos)) {
        if (++failures <= 30) printf("FAILED: %s: code %d (want %d), entry %lld (want %lld), message '%s'\n", what, got, code, (long long)bad, (long long)entry, msg.c_str());
    }
}

/* the plan of a call: the invariants every plan keeps, whatever the list */
static void expect_plan(const MgcLattice& L, const Call& c, const MgcEditPlan& P, const char* what)
{
    const size_t m = 2 * c.i.size();
    bool ok = P.slot.size() == m && P.partner.size() == m && P.c_out1.size() == m && P.c_in1.size() == m && P.begin.size() == P.tile.size() + 1;
    if (ok) {
        /* the tile ranges cover the half-arcs exactly once: begin ascends strictly from 0 to m, tiles ascend strictly */
        ok = ok && P.begin.front() == 0 && P.begin.back() == (int32_t)m;
        for (size_t t = 0; t < P.tile.size() && ok; ++t) {
            ok = P.begin[t] < P.begin[t + 1] && (t == 0 || P.tile[t - 1] < P.tile[t]) && P.tile[t] >= 0 && P.tile[t] < L.ntiles;
            int64_t prev = -1;
            for (int32_t k = P.begin[t]; k < P.begin[t + 1] && ok; ++k) {
                const int64_t o = P.slot[(size_t)k];
                const int64_t tile = o / ((int64_t)L.ndir * MGC_TV), d = (o / MGC_TV) % L.ndir, loc = o % MGC_TV;
                ok = tile == P.tile[t] && loc * 32 + d > prev; /* sorted by (voxel, direction) inside the tile */
                prev = loc * 32 + d;
            }
        }
        /* partners: an involution that swaps the two capacities and points along the reverse direction */
        for (size_t k = 0; k < m && ok; ++k) {
            const size_t p = (size_t)P.partner[k];
            ok = p < m && p != k && (size_t)P.partner[p] == k && mgc_same_bits(P.c_out1[k], P.c_in1[p]) && mgc_same_bits(P.c_in1[k], P.c_out1[p]) &&
                 (int)((P.slot[p] / MGC_TV) % L.ndir) == mgc_edit_reverse(L.ndir, (int)((P.slot[k] / MGC_TV) % L.ndir));
        }
        /* every entry of the call is there, as the arc slot of its tail with the two capacities */
        for (size_t e = 0; e < c.i.size() && ok; ++e) {
            int tile, loc;
            mgc_node_to_tile(L, c.i[e], tile, loc);
            const int64_t zi = c.i[e] / (L.dy * L.dx), yi = (c.i[e] / L.dx) % L.dy, xi = c.i[e] % L.dx;
            const int64_t zj = c.j[e] / (L.dy * L.dx), yj = (c.j[e] / L.dx) % L.dy, xj = c.j[e] % L.dx;
            const int64_t want = ((int64_t)tile * L.ndir + direction_of(L.ndir, (int)(zj - zi), (int)(yj - yi), (int)(xj - xi))) * MGC_TV + loc;
            bool found = false;
            for (size_t k = 0; k < m; ++k)
                if (P.slot[k] == want) found = mgc_same_bits(P.c_out1[k], c.cap[e]) && mgc_same_bits(P.c_in1[k], c.rev[e]);
            ok = found;
        }
    }
    if (!ok && ++failures <= 30) printf("FAILED: plan invariants: %s\n", what);
}

static void prep_cases(int ndim, const int64_t* shape, int connectivity)
{
    const MgcLattice L = lattice(ndim, shape, connectivity);
    char what[128];
    snprintf(what, sizeof(what), "shape (%lld, %lld, %lld) / %d", (long long)L.dz, (long long)L.dy, (long long)L.dx, connectivity);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    /* a list of every arc pair of the lattice that leaves a few voxels: the baseline that must pass */
    std::vector<int> offs;
    for (int oz = -1; oz <= 1; ++oz)
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const int nz = (oz != 0) + (oy != 0) + (ox != 0);
                if (nz == 0 || (L.ndir == 6 && nz != 1)) continue;
                offs.push_back((oz + 1) * 9 + (oy + 1) * 3 + (ox + 1));
            }
    auto inside = [&](int64_t z, int64_t y, int64_t x) { return z >= 0 && z < L.dz && y >= 0 && y < L.dy && x >= 0 && x < L.dx; };
    /* a voxel as far inside as the shape allows, and one in the corner of the first tile where the volume goes on behind it */
    const int64_t cz = std::min<int64_t>(L.dz - 1, L.dz > 8 ? 7 : L.dz / 2), cy = std::min<int64_t>(L.dy - 1, L.dy > 8 ? 7 : L.dy / 2), cx = std::min<int64_t>(L.dx - 1, L.dx > 8 ? 7 : L.dx / 2);
    Call good;
    std::set<int> seen_dirs;
    double w = 1.0;
    for (int c : offs) {
        const int oz = c / 9 - 1, oy = (c / 3) % 3 - 1, ox = c % 3 - 1;
        if (!inside(cz + oz, cy + oy, cx + ox)) continue;
        good.add(node(L, cz, cy, cx), node(L, cz + oz, cy + oy, cx + ox), w, w + 0.5);
        w += 1.0;
        /* direction indices against the encoding of mgc_add_nweights */
        const int d = mgc_arc_direction(L, node(L, cz, cy, cx), node(L, cz + oz, cy + oy, cx + ox));
        expect(d == direction_of(L.ndir, oz, oy, ox), "direction index of an offset", oz, oy, ox, d);
        seen_dirs.insert(d);
    }
    if (ndim == 3 && L.dz > 8 && L.dy > 8 && L.dx > 8) expect((int)seen_dirs.size() == L.ndir, "every direction of the neighbourhood was looked at", (double)seen_dirs.size(), L.ndir);
    expect(!good.i.empty(), "(the shape has arcs)");
    int64_t bad;
    std::string msg;
    expect(check(L, good, true, &bad, &msg) == MGC_EDIT_OK && bad == -1, "a good list passes");
    expect(check(L, good, false, &bad, &msg) == MGC_EDIT_OK, "a good list passes without rev");
    MgcEditPlan P;
    mgc_edit_plan(L, (int64_t)good.i.size(), good.i.data(), good.j.data(), good.cap.data(), good.rev.data(), &P);
    expect_plan(L, good, P, what);
    /* all arcs of the one voxel are adjacent after the sort (three of them, where the shape has that many) */
    {
        int tile, loc, run = 0, best = 0;
        mgc_node_to_tile(L, good.i[0], tile, loc);
        for (size_t k = 0; k < P.slot.size(); ++k) {
            const bool mine = P.slot[k] / ((int64_t)L.ndir * MGC_TV) == tile && P.slot[k] % MGC_TV == loc;
            run = mine ? run + 1 : 0;
            best = std::max(best, run);
        }
        expect(best == (int)good.i.size(), "the arcs of one voxel are adjacent after the sort", best, (double)good.i.size());
        expect(good.i.size() >= 3 || L.nvox / std::max(L.dz, std::max(L.dy, L.dx)) == 1, "(three arcs of one voxel)", (double)good.i.size());
    }
    /* pairs across a tile face, an edge and a corner give two tiles */
    for (int c : offs) {
        const int oz = c / 9 - 1, oy = (c / 3) % 3 - 1, ox = c % 3 - 1;
        if (oz < 0 || oy < 0 || ox < 0) continue;
        const int64_t z = oz ? 7 : 0, y = oy ? 7 : 0, x = ox ? 7 : 0; /* steps from coordinate 7 to 8 along every axis of the offset */
        if (!inside(z + oz, y + oy, x + ox)) continue;
        Call one;
        one.add(node(L, z, y, x), node(L, z + oz, y + oy, x + ox), 2.0, 3.0);
        MgcEditPlan Q;
        mgc_edit_plan(L, 1, one.i.data(), one.j.data(), one.cap.data(), one.rev.data(), &Q);
        expect_plan(L, one, Q, what);
        expect(Q.tile.size() == 2 && Q.begin.size() == 3 && Q.begin[1] == 1, "a pair across a tile face / edge / corner gives two tiles", oz, oy, ox, (double)Q.tile.size());
    }
    /* a pair inside a tile gives one */
    if (L.dx > 1) {
        Call one;
        one.add(node(L, 0, 0, 0), node(L, 0, 0, 1), 0.0, 0.0);
        MgcEditPlan Q;
        mgc_edit_plan(L, 1, one.i.data(), one.j.data(), one.cap.data(), nullptr, &Q);
        expect(Q.tile.size() == 1 && Q.begin[1] == 2 && Q.c_in1[0] == 0.0, "a pair inside a tile gives one tile");
    }
    /* every refusal, with the entry it names; the bad entry sits behind the good ones */
    const int64_t at = (int64_t)good.i.size();
    { Call c = good; c.add(L.nvox, 0, 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "an id == nvox"); }
    { Call c = good; c.add(0, -1, 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a negative id"); }
    { Call c = good; c.add(0, 0, 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_NOT_NEIGHBOURS, at, "i == j"); }
    if (L.dx > 2) { Call c = good; c.add(0, 2, 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_NOT_NEIGHBOURS, at, "two steps along x"); }
    if (L.ndir == 6 && L.dy > 1 && L.dx > 1) { Call c = good; c.add(0, node(L, 0, 1, 1), 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_NOT_NEIGHBOURS, at, "a diagonal in the 6-neighbourhood"); }
    if (L.dx > 1 && L.dy > 1) { Call c = good; c.add(node(L, 0, 0, L.dx - 1), node(L, 0, 1, 0), 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_NOT_NEIGHBOURS, at, "consecutive ids across the end of a row"); }
    const double bads[4] = {-1.0, inf, nan, -1e-300};
    for (double b : bads) {
        const int64_t u = 0, v = 1; /* a pair along x that the good list, which sits around coordinate 7, does not hold */
        { Call c = good; c.add(u, v, b, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a bad capacity"); expect_refused(L, c, false, MGC_EDIT_INVALID, at, "a bad capacity, rev NULL"); }
        { Call c = good; c.add(u, v, 1.0, b); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a bad reverse capacity"); }
    }
    { Call c = good; c.add(good.i[0], good.j[0], 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a pair twice"); }
    { Call c = good; c.add(good.j[0], good.i[0], 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a pair twice, the other way round"); }
    /* the FIRST offending entry: a repeated pair in front of a bad id, and a bad id in front of a repeated pair */
    { Call c = good; c.add(good.j[0], good.i[0], 1.0, 1.0); c.add(L.nvox, 0, 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "twice, then a bad id"); }
    { Call c = good; c.add(L.nvox, 0, 1.0, 1.0); c.add(good.j[0], good.i[0], 1.0, 1.0); expect_refused(L, c, true, MGC_EDIT_INVALID, at, "a bad id, then twice"); }
}

int main()
{
    rule_cases();
    const int64_t s0[3] = {17, 9, 10}, s1[3] = {9, 10, 11}, s2[2] = {9, 10}, s3[3] = {1, 1, 17};
    prep_cases(3, s0, 6);
    prep_cases(3, s1, 26);
    prep_cases(2, s2, 4);
    prep_cases(2, s2, 8);
    prep_cases(3, s3, 6);
    if (failures) printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
