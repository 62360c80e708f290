/*
 * reach_main.cpp -- stand-alone host program of the CPU test tier for the forward reachability flood of mgc_cut_sets.
 *
 * Compiles the tile step of medpy_amd/csrc/mgc_reach_ops.inl for the host (one worker, no barrier) and floods randomly masked
 * lattices with it tile by tile, the way the device does: a work list of tiles, visited in RANDOM order, every visit queues the
 * neighbour tiles an open arc leads into (stamp de-duplicated) for the next pass, until a pass queues nobody.  The result must be
 * the set a plain voxel BFS over the C-order volume finds.  6 and 26 directions, volumes with partial tiles and single-voxel axes.
 *
 * The masks are as hostile as the tile-major planes allow: directed (bit d of u says nothing about the way back), random bits on
 * the padding voxels of partial tiles and on directions that leave the volume.  Neither may ever carry a mark.
 *
 * The same body runs the backward flood of mgc_cut_sets_tol (BACK): on every case the backward flood must mark what the forward flood
 * marks on the transposed masks.
 *
 * Built and run by tests/test_cut_sets_host.py, plainly and with -fsanitize=address,undefined.  Prints what failed; exit code 0 = all passed.
 */
#include <cstdlib>
#include <queue>

#include "../../medpy_amd/csrc/mgc_reach_ops.inl"
#include "reach_host.h"

struct Result {
    int passes = 0;
    long visits = 0;
};

template <int NDIR, class Mask>
static int run_case(int64_t dz, int64_t dy, int64_t dx, double p_open, double p_seed, uint32_t seed, Result& res)
{
    const MgcLattice L = lattice(dz, dy, dx, NDIR);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const size_t ntv = (size_t)L.ntiles * MGC_TV;
    std::vector<Mask> masks(ntv);
    std::vector<uint8_t> marks(ntv, 0), inside(ntv, 0);
    for (size_t i = 0; i < ntv; ++i) {
        uint32_t m = 0;
        for (int d = 0; d < NDIR; ++d)
            if (uni(rng) < p_open) m |= 1u << d;
        if (uni(rng) < 0.3) m |= 1u << NDIR; /* the sink bit: not an arc */
        masks[i] = (Mask)m;
    }
    /* seeds: voxels of the volume only, as k_reach_seed marks them */
    for (int64_t id = 0; id < L.nvox; ++id) {
        int tile, loc;
        mgc_node_to_tile(L, id, tile, loc);
        inside[(size_t)tile * MGC_TV + loc] = 1;
        if (uni(rng) < p_seed) marks[(size_t)tile * MGC_TV + loc] = 1;
    }
    /* the reference: BFS over the voxels, the arc u -> v open iff bit d of u's mask is set */
    std::vector<uint8_t> ref(L.nvox, 0);
    {
        std::queue<int64_t> q;
        for (int64_t id = 0; id < L.nvox; ++id) {
            int tile, loc;
            mgc_node_to_tile(L, id, tile, loc);
            if (marks[(size_t)tile * MGC_TV + loc]) { ref[id] = 1; q.push(id); }
        }
        while (!q.empty()) {
            const int64_t u = q.front();
            q.pop();
            int tile, loc;
            mgc_node_to_tile(L, u, tile, loc);
            const uint32_t m = (uint32_t)masks[(size_t)tile * MGC_TV + loc];
            const int64_t ux = u % dx, uy = (u / dx) % dy, uz = u / (dx * dy);
            for (int d = 0; d < NDIR; ++d) {
                if (!((m >> d) & 1u)) continue;
                int oz, oy, ox;
                mgc_reach_offset<NDIR>(d, oz, oy, ox);
                const int64_t vz = uz + oz, vy = uy + oy, vx = ux + ox;
                if (vz < 0 || vz >= dz || vy < 0 || vy >= dy || vx < 0 || vx >= dx) continue;
                const int64_t v = (vz * dy + vy) * dx + vx;
                if (mgc_arc_direction(L, u, v) != d) { printf("direction table: arc %lld -> %lld is not direction %d\n", (long long)u, (long long)v, d); return 1; }
                if (!ref[v]) { ref[v] = 1; q.push(v); }
            }
        }
    }
    /* the flood, tile by tile */
    const std::vector<uint8_t> seeds = marks;
    if (flood<NDIR, Mask>(L, marks, masks, false, rng, res.passes, res.visits)) return 1;
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
        printf("%d directions, %lld x %lld x %lld, p %.2f, seed %u: %ld voxels differ from the BFS, %ld padding voxels marked (BFS marks %ld)\n",
               NDIR, (long long)dz, (long long)dy, (long long)dx, p_open, seed, bad, padding, count);
        return 1;
    }
    /* One body serves both directions: the backward flood from the seeds on these masks marks exactly what the forward flood from the
     * same seeds marks on the TRANSPOSED masks -- bit d of v = bit opposite(d) of v + offset(d), 0 where that voxel lies outside the
     * volume; padding voxels keep their random bits. */
    std::vector<Mask> transposed = masks;
    for (int64_t id = 0; id < L.nvox; ++id) {
        uint32_t m = 0;
        for (int d = 0; d < NDIR; ++d) {
            const int64_t n = neighbour<NDIR>(L, id, d);
            if (n < 0) continue;
            int tile, loc;
            mgc_node_to_tile(L, n, tile, loc);
            m |= (((uint32_t)masks[(size_t)tile * MGC_TV + loc] >> mgc_reach_opposite<NDIR>(d)) & 1u) << d;
        }
        int tile, loc;
        mgc_node_to_tile(L, id, tile, loc);
        transposed[(size_t)tile * MGC_TV + loc] = (Mask)m;
    }
    std::vector<uint8_t> back = seeds, fwd_t = seeds;
    int passes = 0;
    long visits = 0;
    if (flood<NDIR, Mask>(L, back, masks, true, rng, passes, visits) || flood<NDIR, Mask>(L, fwd_t, transposed, false, rng, passes, visits)) return 1;
    if (back != fwd_t) {
        long differ = 0;
        for (size_t i = 0; i < ntv; ++i) differ += back[i] != fwd_t[i];
        printf("%d directions, %lld x %lld x %lld, p %.2f, seed %u: the backward flood and the forward flood on the transposed masks differ in %ld cells\n",
               NDIR, (long long)dz, (long long)dy, (long long)dx, p_open, seed, differ);
        return 1;
    }
    return 0;
}

int main()
{
    const int64_t shapes[][3] = {{1, 1, 41}, {1, 19, 26}, {8, 8, 8}, {9, 10, 33}, {20, 13, 27}, {17, 17, 17}, {3, 34, 37}, {16, 8, 24}};
    int failed = 0, cases = 0, multi_pass = 0;
    for (const auto& s : shapes)
        for (int k = 0; k < 4; ++k) {
            /* open fractions around the thresholds at which the reachable set goes from pockets to most of the volume */
            const double p6[4] = {0.15, 0.3, 0.4, 0.6}, p26[4] = {0.03, 0.06, 0.1, 0.3};
            Result a, b;
            failed += run_case<6, uint8_t>(s[0], s[1], s[2], p6[k], 0.01, 1000u * (uint32_t)cases + 1u, a);
            failed += run_case<26, uint32_t>(s[0], s[1], s[2], p26[k], 0.01, 1000u * (uint32_t)cases + 2u, b);
            multi_pass += (a.passes > 1) + (b.passes > 1);
            cases += 2;
        }
    /* no seed at all: nothing marked, no visit */
    {
        Result r;
        failed += run_case<6, uint8_t>(9, 10, 33, 0.5, 0.0, 7u, r);
        if (r.passes != 0 || r.visits != 0) { printf("a flood without seeds visited %ld tiles\n", r.visits); failed++; }
        cases++;
    }
    if (multi_pass < cases / 4) { printf("only %d of %d floods crossed a tile face: the cases do not test the lists\n", multi_pass, cases); failed++; }
    printf("%d cases, %d floods of more than one pass, %d failed\n", cases, multi_pass, failed);
    return failed ? 1 : 0;
}
