/*
 * mgc_nlink_edit_ops.inl -- edits of n-links by arc list (mgc_edit_nweights; DESIGN 10, "Edits of n-links by list"): the listed
 * arcs get new capacities (REPLACE), the flow the last solve left on them is clamped to the new pair of capacities and what no
 * longer fits goes back to the arcs' ends as signed excess (mgc_nlink_fold_directed).  The host has checked and sorted the list
 * (mgc_nlink_edit.h).  Included by mgc_kernels.hip behind mgc_built_capacity.
 *
 *   k_materialise_cap0  the capacities as built of an image-determined graph, written out once: from then on the handle is a cap0 handle
 *   k_edit_gather       the capacities as built of the listed arcs, before anybody writes one
 *   k_edit_nlinks       the fold: one wave per touched tile, no barriers, no atomics
 */
#ifndef MGC_NLINK_EDIT_OPS_INL
#define MGC_NLINK_EDIT_OPS_INL

#include "mgc_nlink_fold.h"

#define MGC_EDIT_MAX_WAVES 1024 /* persistent grid of k_edit_nlinks: a wave per touched tile up to here, then tiles in turns */

/* per wave of k_edit_nlinks (summed on the host: what mgc_get_nweight_edit_info reports) */
struct MgcEditCounts {
    unsigned pairs_changed;  /* pairs with a capacity that changed bitwise (counted at the pair's first half-arc) */
    unsigned arcs_clamped;   /* arcs whose flow no longer fitted */
    unsigned voxels_changed; /* voxels whose excess or residual sink link changed */
    unsigned pad;
};

/* L.cap0 is NULL here: mgc_built_capacity evaluates the boundary term from the resident image, with the operations of k_build.  One
 * workgroup per tile as k_build is laid out; arcs that leave the volume and padding voxels get 0, what k_build writes there. */
template <bool FULL>
__global__ __launch_bounds__(MGC_TV) void k_materialise_cap0(MgcLattice L, MgcBuildArgs A, double* cap0)
{
    constexpr int NDIR = FULL ? MGC26_NDIR : MGC_NDIR;
    const int t = threadIdx.x;
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        const int64_t gz = (int64_t)tz * 8 + (t >> 6), gy = (int64_t)ty * 8 + ((t >> 3) & 7), gx = (int64_t)tx * 8 + (t & 7);
        const bool valid = gz < L.dz && gy < L.dy && gx < L.dx;
#pragma unroll
        for (int d = 0; d < NDIR; ++d) {
            int dz, dy, dx;
            if (FULL) mgc26_offset(d, dz, dy, dx);
            else {
                dz = (d >> 1) == 2 ? ((d & 1) ? 1 : -1) : 0;
                dy = (d >> 1) == 1 ? ((d & 1) ? 1 : -1) : 0;
                dx = (d >> 1) == 0 ? ((d & 1) ? 1 : -1) : 0;
            }
            const bool has = valid && gz + dz >= 0 && gz + dz < L.dz && gy + dy >= 0 && gy + dy < L.dy && gx + dx >= 0 && gx + dx < L.dx;
            const double c = has ? mgc_built_capacity(L, A, tile, t, gz, gy, gx, d) : 0.0;
            MGC_STORE_STREAM(&cap0[((int64_t)tile * NDIR + d) * MGC_TV + t], c);
        }
    }
}

/* old[k] = capacity as built of half-arc k's arc.  A launch of its own in front of the fold: a wave of k_edit_nlinks needs the old
 * capacity of the REVERSE arc too, which lives in a tile that another wave is writing. */
__global__ __launch_bounds__(256) void k_edit_gather(int64_t m, const int64_t* __restrict__ slot, const double* __restrict__ cap0, double* __restrict__ old)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) old[k] = cap0[slot[k]];
}

/* One wave per touched tile (64 lanes x 8 voxels = the tile), tiles in turns over a persistent grid; ntouched tiles, the half-arcs of
 * tile[m] are [begin[m], begin[m + 1]), sorted by (voxel, direction).  A lane takes a voxel's whole run of half-arcs -- the lane that
 * holds the run's first half-arc walks it -- so the voxel's signed excess x = excess - sink collects what its arcs give back
 * sequentially, in direction order, and every word of the tile's state has one writer.  A pair across a tile face, edge or corner is
 * two half-arcs in two tiles; the two waves share nothing (the old capacities come from k_edit_gather).
 *
 * FLAGS (k_update_tlinks): the 6-neighbourhood reads the planes tr0 and sink as zeros where the tile's flags do not vouch for them
 * (tflags == 0; no MGC_ST_SINK).  The wave writes such a plane in full -- zeros, 8 voxels a lane -- BEFORE it folds, so a voxel that
 * ends with sink > 0 stores into a valid plane, and the tile then gets tflags bit 1, MGC_ST_SINK and the voxel's mask bit.  A tile
 * that gains nothing keeps its flags: its planes then hold zeros where they held garbage, which nobody reads either.
 * The status word only gains bits here (SINK, EXCESS); the whole-volume refresh behind the launch (mgc_update_tlinks) rewrites every
 * status word, the stamps and the count of sink tiles from the planes. */
template <bool FULL>
__global__ __launch_bounds__(64) void k_edit_nlinks(MgcLattice L, double* tr0, uint8_t* tflags, int ntouched, const int32_t* __restrict__ tiles,
                                                    const int32_t* __restrict__ begin, const int64_t* __restrict__ slot, const int32_t* __restrict__ partner,
                                                    const double* __restrict__ c_out1, const double* __restrict__ c_in1, const double* __restrict__ old,
                                                    MgcEditCounts* counts)
{
    constexpr int NDIR = FULL ? MGC26_NDIR : MGC_NDIR;
    const int lane = threadIdx.x;
    unsigned n_pairs = 0, n_clamped = 0, n_voxels = 0;
    for (int ti = blockIdx.x; ti < ntouched; ti += gridDim.x) {
        const int tile = tiles[ti];
        const int b = begin[ti], e = begin[ti + 1];
        const uint32_t st = L.status[tile];
        const uint32_t tf_old = tflags[tile];
        const bool tr0_ok = FULL || tf_old != 0u, sink_ok = FULL || (st & MGC_ST_SINK) != 0u;
        const int64_t v0 = (int64_t)tile * MGC_TV;
        if (!sink_ok) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                L.sink[v0 + q * 64 + lane] = 0.0;
                if (!tr0_ok) tr0[v0 + q * 64 + lane] = 0.0;
            }
            /* the zeros are out before a lane stores another lane's voxel: two stores of one wave to one address, from different lanes */
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        bool any_sink = false, any_excess = false;
        for (int a0 = b; a0 < e; a0 += 64) { /* (uniform) */
            const int a = a0 + lane;
            if (a >= e) continue;
            const int loc = (int)(slot[a] & (MGC_TV - 1));
            if (a > b && (int)(slot[a - 1] & (MGC_TV - 1)) == loc) continue; /* inside a run: its first lane walks it */
            const int64_t v = v0 + loc;
            const double sk_old = sink_ok ? L.sink[v] : 0.0;
            const double e_old = L.excess[v];
            double x = e_old - sk_old;
            bool gave = false, touched = false;
            uint32_t m = FULL ? L.rmask32[v] : (uint32_t)L.rmask[v];
            for (int k = a; k < e; ++k) {
                const int64_t o = slot[k];
                if ((int)(o & (MGC_TV - 1)) != loc) break;
                const int d = (int)(o >> 9) - tile * NDIR;
                const int pk = partner[k];
                const double co = old[k], ci = old[pk], co1 = c_out1[k], ci1 = c_in1[k];
                if (mgc_same_bits(co, co1) && mgc_same_bits(ci, ci1)) continue;
                double r = L.rcap[o];
                bool clamped;
                const double back = mgc_nlink_fold_directed(co, ci, co1, ci1, &r, &clamped);
                L.rcap[o] = r;
                if (!mgc_same_bits(co, co1)) L.cap0[o] = co1;
                m = (m & ~(1u << d)) | (r > 0.0 ? 1u << d : 0u);
                if (back != 0.0) { x += back; gave = true; }
                touched = true;
                n_pairs += pk > k ? 1u : 0u;
                n_clamped += clamped ? 1u : 0u;
            }
            double ex = e_old, sk = sk_old;
            if (gave) {
                ex = x > 0.0 ? x : 0.0;
                sk = x < 0.0 ? -x : 0.0;
            }
            if (ex != e_old) L.excess[v] = ex;
            if (sk != sk_old) L.sink[v] = sk;
            if (touched || (sk > 0.0) != (sk_old > 0.0)) {
                if (FULL) L.rmask32[v] = (m & ~MGC26_MASK_SINK) | (sk > 0.0 ? MGC26_MASK_SINK : 0u);
                else L.rmask[v] = (uint8_t)((m & ~(uint32_t)MGC_MASK_SINK) | (sk > 0.0 ? MGC_MASK_SINK : 0));
            }
            n_voxels += (ex != e_old || sk != sk_old) ? 1u : 0u;
            any_sink |= sk > 0.0;
            any_excess |= ex > 0.0;
        }
        const bool tile_sink = __ballot(any_sink) != 0ull, tile_excess = __ballot(any_excess) != 0ull;
        if (lane == 0 && (tile_sink || tile_excess)) {
            L.status[tile] = st | (tile_sink ? MGC_ST_SINK : 0u) | (tile_excess ? MGC_ST_EXCESS : 0u);
            if (tile_sink) tflags[tile] = (uint8_t)(tf_old | 2u);
        }
    }
    /* the counters: summed over the wave, one slot per wave */
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_pairs += (unsigned)__shfl_xor((int)n_pairs, d, 64);
        n_clamped += (unsigned)__shfl_xor((int)n_clamped, d, 64);
        n_voxels += (unsigned)__shfl_xor((int)n_voxels, d, 64);
    }
    if (lane == 0) {
        counts[blockIdx.x].pairs_changed = n_pairs;
        counts[blockIdx.x].arcs_clamped = n_clamped;
        counts[blockIdx.x].voxels_changed = n_voxels;
        counts[blockIdx.x].pad = 0u;
    }
}

#endif /* MGC_NLINK_EDIT_OPS_INL */
