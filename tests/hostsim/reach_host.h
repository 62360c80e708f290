/*
 * reach_host.h -- what the stand-alone host programs of the flood (reach_main.cpp, reach_tol_main.cpp) share: a lattice without a
 * device, the neighbour of a voxel, and one flood to its fixpoint the way the device runs it -- a work list of tiles visited in
 * RANDOM order, every visit queues neighbour tiles (stamp de-duplicated) for the next pass, until a pass queues nobody.
 * Include behind medpy_amd/csrc/mgc_reach_ops.inl (or mgc_reach_tol_ops.inl).
 */
#ifndef REACH_HOST_H
#define REACH_HOST_H

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

struct NoBarrier {
    int operator()(int v) const { return v; }
};

static MgcLattice lattice(int64_t dz, int64_t dy, int64_t dx, int ndir)
{
    MgcLattice L;
    memset(&L, 0, sizeof(L));
    L.dz = dz; L.dy = dy; L.dx = dx;
    L.nvox = dz * dy * dx;
    L.gz = (int)((dz + 7) / 8); L.gy = (int)((dy + 7) / 8); L.gx = (int)((dx + 7) / 8);
    L.ntiles = L.gz * L.gy * L.gx;
    L.tz_own_hi = L.gz;
    L.ndir = ndir;
    L.nshard = 1;
    return L;
}

/* the neighbour of voxel id in direction d, or -1 */
template <int NDIR>
static int64_t neighbour(const MgcLattice& L, int64_t id, int d)
{
    int oz, oy, ox;
    mgc_reach_offset<NDIR>(d, oz, oy, ox);
    const int64_t x = id % L.dx + ox, y = (id / L.dx) % L.dy + oy, z = id / (L.dx * L.dy) + oz;
    if (z < 0 || z >= L.dz || y < 0 || y >= L.dy || x < 0 || x >= L.dx) return -1;
    return (z * L.dy + y) * L.dx + x;
}

/* one flood from the marked voxels to its fixpoint, tile by tile, with the arcs (back = false) or against them; counts passes and visits */
template <int NDIR, class Mask>
static int flood(const MgcLattice& L, std::vector<uint8_t>& marks, const std::vector<Mask>& masks, bool back, std::mt19937& rng, int& passes, long& visits)
{
    std::vector<int> cur, nxt;
    std::vector<uint32_t> stamp(L.ntiles, 0);
    for (int tile = 0; tile < L.ntiles; ++tile)
        for (int v = 0; v < MGC_TV; ++v)
            if (marks[(size_t)tile * MGC_TV + v]) { cur.push_back(tile); break; }
    std::vector<uint8_t> mk(MGC_REACH_BLOCK);
    std::vector<uint32_t> ms(MGC_REACH_BLOCK);
    NoBarrier sync;
    uint32_t epoch = 0;
    while (!cur.empty()) {
        ++epoch;
        visits += (long)cur.size();
        if (++passes > 100000) { printf("the flood does not end\n"); return 1; }
        std::shuffle(cur.begin(), cur.end(), rng);
        for (int tile : cur) {
            const uint32_t wake = back ? mgc_reach_tile_step<NDIR, true>(L, marks.data(), masks.data(), tile, mk.data(), ms.data(), 0, 1, sync)
                                       : mgc_reach_tile_step<NDIR, false>(L, marks.data(), masks.data(), tile, mk.data(), ms.data(), 0, 1, sync);
            for (int c = 0; c < 27; ++c) {
                if (!((wake >> c) & 1u)) continue;
                const int nt = mgc_reach_wake_tile(L, tile, c);
                if (nt < 0) { printf("tile %d wakes a tile outside the grid (bit %d)\n", tile, c); return 1; }
                if (stamp[nt] != epoch) { stamp[nt] = epoch; nxt.push_back(nt); }
            }
        }
        cur.swap(nxt);
        nxt.clear();
    }
    return 0;
}

#endif /* REACH_HOST_H */
