/*
 * reach_tol_main.cpp -- stand-alone host program of the CPU test tier for mgc_cut_sets_tol: the scale step and the open
 * step of medpy_amd/csrc/mgc_reach_tol_ops.inl and both directions of the tile step of mgc_reach_ops.inl, compiled for the host and run with one thread, against a plain
 * per-voxel restatement of the rule over the C-order volume and a voxel BFS.
 *
 * The residual planes are as hostile as the tile-major layout allows: directed (rcap of u -> v says nothing about v -> u), a mixture
 * of zeros, dust (2^-80 .. 2^-70) and weights of order 1, and GARBAGE -- large positive numbers -- on the padding voxels of partial
 * tiles and on every direction that leaves the volume.  Neither may raise a scale, open an arc, count as closed or carry a mark.
 * The floods run tile by tile the way the device runs them: a work list visited in RANDOM order, every visit queues neighbour tiles
 * (stamp de-duplicated) for the next pass, until a pass queues nobody.  Both floods are the tile step of mgc_reach_ops.inl on the
 * thresholded plane, with the arcs and against them.  6 and 26 directions, partial tiles, single-voxel axes.
 *
 * Built and run by tests/test_cut_sets_tol_host.py, plainly and with -fsanitize=address,undefined.  Exit code 0 = all passed.
 */
#include <cmath>
#include <cstdlib>
#include <queue>

#include "../../medpy_amd/csrc/mgc_reach_tol_ops.inl"
#include "reach_host.h"

struct Result {
    int passes_fwd = 0, passes_back = 0;
    long closed = 0;
};

template <int NDIR, class Mask>
static int run_case(int64_t dz, int64_t dy, int64_t dx, double p_zero, double p_dust, double p_seed, double tol, uint32_t seed, Result& res)
{
    const MgcLattice L = lattice(dz, dy, dx, NDIR);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const size_t ntv = (size_t)L.ntiles * MGC_TV;
    /* every word of the planes garbage first, then the arcs inside the volume */
    std::vector<double> rcap(ntv * NDIR);
    for (double& r : rcap) r = 1e3 + 1e6 * uni(rng);
    std::vector<uint8_t> inside(ntv, 0);
    auto plane = [&](int64_t id, int d) -> double& {
        int tile, loc;
        mgc_node_to_tile(L, id, tile, loc);
        return rcap[((size_t)tile * NDIR + d) * MGC_TV + loc];
    };
    for (int64_t id = 0; id < L.nvox; ++id) {
        int tile, loc;
        mgc_node_to_tile(L, id, tile, loc);
        inside[(size_t)tile * MGC_TV + loc] = 1;
        for (int d = 0; d < NDIR; ++d) {
            if (neighbour<NDIR>(L, id, d) < 0) continue;
            const double u = uni(rng);
            plane(id, d) = u < p_zero ? 0.0 : (u < p_zero + p_dust ? ldexp(1.0 + 1000.0 * uni(rng), -80) : 1.0 + 7.0 * uni(rng));
        }
    }
    /* the rule, voxel by voxel over the C-order volume */
    std::vector<double> scale_ref(L.nvox, 0.0);
    double most_ref = 0.0;
    for (int64_t id = 0; id < L.nvox; ++id) {
        for (int d = 0; d < NDIR; ++d) {
            const int64_t n = neighbour<NDIR>(L, id, d);
            if (n < 0) continue;
            if (mgc_arc_direction(L, id, n) != d) { printf("direction table: arc %lld -> %lld is not direction %d\n", (long long)id, (long long)n, d); return 1; }
            scale_ref[id] = std::max(scale_ref[id], plane(id, d) + plane(n, mgc_reach_opposite<NDIR>(d)));
        }
        most_ref = std::max(most_ref, scale_ref[id]);
    }
    std::vector<uint32_t> open_ref(L.nvox, 0);
    long closed_ref = 0;
    for (int64_t id = 0; id < L.nvox; ++id)
        for (int d = 0; d < NDIR; ++d) {
            const int64_t n = neighbour<NDIR>(L, id, d);
            if (n < 0) continue;
            const double r = plane(id, d);
            if (r > 0.0 && r > tol * std::max(scale_ref[id], scale_ref[n])) open_ref[id] |= 1u << d;
            else if (r > 0.0) closed_ref++;
        }
    /* the two steps, tiles in random order */
    std::vector<int> order(L.ntiles);
    for (int t = 0; t < L.ntiles; ++t) order[t] = t;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<double> scale(ntv, -1.0);
    double most = 0.0;
    for (int tile : order) most = std::max(most, mgc_reach_scale_tile<NDIR>(L, rcap.data(), scale.data(), tile, 0, 1));
    std::vector<Mask> masks(ntv, (Mask)~(Mask)0);
    long closed = 0;
    std::shuffle(order.begin(), order.end(), rng);
    for (int tile : order) closed += mgc_reach_open_tile<NDIR, Mask>(L, rcap.data(), scale.data(), tol, masks.data(), tile, 0, 1);
    long bad_scale = 0, bad_mask = 0, bad_pad = 0;
    for (size_t i = 0; i < ntv; ++i)
        if (!inside[i] && (scale[i] != 0.0 || masks[i] != 0)) bad_pad++;
    for (int64_t id = 0; id < L.nvox; ++id) {
        int tile, loc;
        mgc_node_to_tile(L, id, tile, loc);
        if (scale[(size_t)tile * MGC_TV + loc] != scale_ref[id]) bad_scale++;
        if ((uint32_t)masks[(size_t)tile * MGC_TV + loc] != open_ref[id]) bad_mask++;
    }
    if (bad_scale || bad_mask || bad_pad || closed != closed_ref || most != most_ref) {
        printf("%d directions, %lld x %lld x %lld, tol %g, seed %u: %ld scales and %ld masks differ from the restatement, %ld padding voxels not 0, closed %ld (expected %ld), largest %g (expected %g)\n",
               NDIR, (long long)dz, (long long)dy, (long long)dx, tol, seed, bad_scale, bad_mask, bad_pad, closed, closed_ref, most, most_ref);
        return 1;
    }
    res.closed += closed;
    /* seeds, then both closures by BFS over the voxels and by the tile steps */
    std::vector<uint8_t> seeds(L.nvox, 0);
    for (int64_t id = 0; id < L.nvox; ++id) seeds[id] = uni(rng) < p_seed;
    for (int back = 0; back < 2; ++back) {
        std::vector<uint8_t> ref(L.nvox, 0), marks(ntv, 0);
        std::queue<int64_t> q;
        for (int64_t id = 0; id < L.nvox; ++id)
            if (seeds[id]) {
                int tile, loc;
                mgc_node_to_tile(L, id, tile, loc);
                marks[(size_t)tile * MGC_TV + loc] = 1;
                ref[id] = 1;
                q.push(id);
            }
        while (!q.empty()) {
            const int64_t v = q.front();
            q.pop();
            for (int d = 0; d < NDIR; ++d) {
                const int64_t n = neighbour<NDIR>(L, v, d);
                if (n < 0 || ref[n]) continue;
                /* forward: the arc v -> n, v's bit d; backward: the arc n -> v, n's bit for the direction back */
                const bool open = back ? ((open_ref[n] >> mgc_reach_opposite<NDIR>(d)) & 1u) != 0 : ((open_ref[v] >> d) & 1u) != 0;
                if (open) { ref[n] = 1; q.push(n); }
            }
        }
        long visits = 0;
        if (flood<NDIR, Mask>(L, marks, masks, back != 0, rng, back ? res.passes_back : res.passes_fwd, visits)) return 1;
        long bad = 0, padding = 0, count = 0;
        for (size_t i = 0; i < ntv; ++i)
            if (marks[i] && !inside[i]) padding++;
        for (int64_t id = 0; id < L.nvox; ++id) {
            int tile, loc;
            mgc_node_to_tile(L, id, tile, loc);
            const uint8_t got = marks[(size_t)tile * MGC_TV + loc];
            if (got > 1 || (got != 0) != (ref[id] != 0)) bad++;
            count += ref[id];
        }
        if (bad || padding) {
            printf("%d directions, %lld x %lld x %lld, tol %g, seed %u, %s flood: %ld voxels differ from the BFS, %ld padding voxels marked (BFS marks %ld)\n",
                   NDIR, (long long)dz, (long long)dy, (long long)dx, tol, seed, back ? "backward" : "forward", bad, padding, count);
            return 1;
        }
    }
    return 0;
}

static int rule_cases()
{
    int failed = 0;
    const double dust = ldexp(1.0, -80), ulp64 = 64.0 * ldexp(1.0, -52);
    failed += !mgc_tol_arc_open(dust, 0.0, 4.0, 8.0);          /* tol 0: open iff > 0 */
    failed += mgc_tol_arc_open(0.0, 0.0, 4.0, 8.0);
    failed += mgc_tol_arc_open(0.0, 0.0, 0.0, 0.0);            /* never "0 > 0 * 0" */
    failed += mgc_tol_arc_open(dust, ulp64, 4.0, 0.0);         /* the larger of the two scales decides, whichever end it is */
    failed += mgc_tol_arc_open(dust, ulp64, 0.0, 4.0);
    failed += !mgc_tol_arc_open(dust, ulp64, dust, 2.0 * dust); /* dust among dust is a weight */
    failed += !mgc_tol_arc_open(1.0, ulp64, 4.0, 8.0);
    failed += mgc_tol_tlink_open(dust, ulp64, dust, 4.0);       /* a dust t-link next to arcs of order 1 */
    failed += mgc_tol_tlink_open(dust, ulp64, -1000.0, 0.0);    /* what is left of a large t-link */
    failed += !mgc_tol_tlink_open(dust, ulp64, dust, 0.0);
    failed += !mgc_tol_tlink_open(3.0, ulp64, 0.0, 8.0);        /* stranded excess at a voxel without a t-link */
    failed += mgc_tol_tlink_open(0.0, 0.0, 0.0, 0.0);
    failed += !mgc_tol_tlink_open(dust, 0.0, 5.0, 8.0);
    if (failed) printf("%d cases of the rule itself failed\n", failed);
    return failed;
}

int main()
{
    const int64_t shapes[][3] = {{1, 1, 41}, {1, 19, 26}, {8, 8, 8}, {9, 10, 33}, {20, 13, 27}, {17, 17, 17}, {3, 34, 37}, {16, 8, 24}};
    const double tols[3] = {0.0, 64.0 * ldexp(1.0, -52), 1e-6};
    int failed = rule_cases(), cases = 0, multi_fwd = 0, multi_back = 0;
    long closed = 0;
    for (const auto& s : shapes)
        for (int k = 0; k < 3; ++k) {
            /* zero / dust fractions that leave the open arcs around the threshold at which a closure goes from pockets to most of the volume */
            const double z6[3] = {0.45, 0.3, 0.2}, d6[3] = {0.25, 0.3, 0.3}, z26[3] = {0.8, 0.7, 0.5}, d26[3] = {0.12, 0.2, 0.3};
            Result a, b;
            failed += run_case<6, uint8_t>(s[0], s[1], s[2], z6[k], d6[k], 0.01, tols[k], 1000u * (uint32_t)cases + 1u, a);
            failed += run_case<26, uint32_t>(s[0], s[1], s[2], z26[k], d26[k], 0.01, tols[(k + 1) % 3], 1000u * (uint32_t)cases + 2u, b);
            multi_fwd += (a.passes_fwd > 1) + (b.passes_fwd > 1);
            multi_back += (a.passes_back > 1) + (b.passes_back > 1);
            closed += a.closed + b.closed;
            cases += 2;
        }
    if (multi_fwd < cases / 4 || multi_back < cases / 4) { printf("only %d forward and %d backward floods of %d crossed a tile face: the cases do not test the lists\n", multi_fwd, multi_back, cases); failed++; }
    if (closed == 0) { printf("no arc was closed by a threshold: the cases do not test it\n"); failed++; }
    printf("%d cases, %d forward and %d backward floods of more than one pass, %ld arcs closed by the threshold, %d failed\n", cases, multi_fwd, multi_back, closed, failed);
    return failed ? 1 : 0;
}
