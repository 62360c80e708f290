/*
 * mgc_reach_tol_ops.inl -- the three sets of mgc_cut_sets at a rounding tolerance (mgc_cut_sets_tol); DESIGN 13.
 *
 * from_source(tol) = what the source seeds reach along arcs open at tol, to_sink(tol) = what reaches the sink seeds along such arcs,
 * ambiguous(tol) = neither; "open at tol" and the seeds: mgc_reach_tol.h.  Nothing here looks at the labels: the sink side comes from
 * a flood of its own, against the arcs, so that at tol = 0 it has to find the labels' set by another way.
 *
 *   k_reach_scale       one workgroup per tile: the tile-major f64 plane scale(v), from the tile's own residual planes and the
 *                       reverse residuals of the neighbour voxels (own tile and the one-voxel halo of the neighbour tiles)
 *   k_reach_open        one workgroup per tile: the thresholded mask plane, bit d of v = the arc v -> v + offset(d) is open at tol, in
 *                       the bit layout of rmask / rmask32 (bits towards the outside of the volume and padding voxels: 0); counts the
 *                       arcs with rcap > 0 that the threshold closed
 *   k_reach_seed_tol    one wave per tile: marks the source seeds (or the sink seeds) and lists their tiles
 *   (both floods)       k_reach_flood<NDIR, false | true> of mgc_reach_ops.inl, on the thresholded plane
 *   k_reach_readout_tol the two mark planes -> C order: from_source, to_sink, ambiguous, and the plane "not to_sink" the cut value
 *                       kernel reads; three counts per tile for k_reach_sum
 *
 * The scale and open steps of ONE tile are plain C++ over (first index, stride) as the flood step of mgc_reach_ops.inl: the kernels
 * run them with 512 threads, tests/hostsim/reach_tol_main.cpp with one.
 */
#ifndef MGC_REACH_TOL_OPS_INL
#define MGC_REACH_TOL_OPS_INL

#include "mgc_reach_ops.inl"
#include "mgc_reach_tol.h"

/* slots of the info block (mgc_get_cut_sets_tol_info): 0 .. 2 the counts as in mgc_reach_ops.inl, 3 .. 5 passes / visits / seeded tiles
 * of the forward flood, then: */
#define MGC_REACHT_BACK 6          /* .. 8: passes, visits, seeded tiles of the backward flood */
#define MGC_REACHT_ARCS_CLOSED 9   /* arcs with rcap > 0 that are not open at tol */
#define MGC_REACHT_TLINKS_CLOSED 10 /* voxels with excess > 0, plus voxels with sink > 0, that are no seeds at tol */
#define MGC_REACHT_SKIPPED 11      /* tiles the forward seeding skipped on their label summary */
#define MGC_REACHT_SCALE_MAX 12    /* bit pattern of the largest scale(v) (a non-negative double: ordered as an integer) */

/* the voxel next to local voxel v of tile (tz, ty, tx) in direction d: false outside the volume, else its tile and local index */
template <int NDIR>
MGC_HD bool mgc_reach_neighbour(const MgcLattice& L, int tz, int ty, int tx, int v, int d, int& ntile, int& nloc)
{
    int dz, dy, dx;
    mgc_reach_offset<NDIR>(d, dz, dy, dx);
    const int64_t z = (int64_t)tz * 8 + (v >> 6) + dz, y = (int64_t)ty * 8 + ((v >> 3) & 7) + dy, x = (int64_t)tx * 8 + (v & 7) + dx;
    if (z < 0 || z >= L.dz || y < 0 || y >= L.dy || x < 0 || x >= L.dx) return false;
    ntile = mgc_tile_id(L, (int)(z >> 3), (int)(y >> 3), (int)(x >> 3));
    nloc = mgc_local((int)(z & 7), (int)(y & 7), (int)(x & 7));
    return true;
}

MGC_HD bool mgc_reach_inside(const MgcLattice& L, int tz, int ty, int tx, int v)
{
    return (int64_t)tz * 8 + (v >> 6) < L.dz && (int64_t)ty * 8 + ((v >> 3) & 7) < L.dy && (int64_t)tx * 8 + (v & 7) < L.dx;
}

/* scale(v) of every voxel of one tile by workers t0, t0 + nt, ...: the largest pair capacity among the arc pairs whose two ends are
 * voxels of the volume; padding voxels get 0.  rcap: [ntiles][NDIR][512].  Returns the largest value this worker wrote. */
template <int NDIR>
MGC_HD double mgc_reach_scale_tile(const MgcLattice& L, const double* rcap, double* scale, int tile, int t0, int nt)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    double most = 0.0;
    for (int v = t0; v < MGC_TV; v += nt) {
        double s = 0.0;
        if (mgc_reach_inside(L, tz, ty, tx, v)) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int d = 0; d < NDIR; ++d) {
                int ntile, nloc;
                if (!mgc_reach_neighbour<NDIR>(L, tz, ty, tx, v, d, ntile, nloc)) continue;
                const double pair = mgc_tol_pair(rcap[((int64_t)tile * NDIR + d) * MGC_TV + v],
                                                 rcap[((int64_t)ntile * NDIR + mgc_reach_opposite<NDIR>(d)) * MGC_TV + nloc]);
                if (pair > s) s = pair;
            }
        }
        scale[(int64_t)tile * MGC_TV + v] = s;
        if (s > most) most = s;
    }
    return most;
}

/* the thresholded masks of one tile: bit d of voxel v = the arc v -> v + offset(d) leads to a voxel of the volume and is open at tol.
 * Returns the number of this worker's arcs with rcap > 0 that are not. */
template <int NDIR, class Mask>
MGC_HD int mgc_reach_open_tile(const MgcLattice& L, const double* rcap, const double* scale, double tol, Mask* omask, int tile, int t0, int nt)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    int closed = 0;
    for (int v = t0; v < MGC_TV; v += nt) {
        uint32_t m = 0;
        if (mgc_reach_inside(L, tz, ty, tx, v)) {
            const double su = scale[(int64_t)tile * MGC_TV + v];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int d = 0; d < NDIR; ++d) {
                int ntile, nloc;
                if (!mgc_reach_neighbour<NDIR>(L, tz, ty, tx, v, d, ntile, nloc)) continue;
                const double r = rcap[((int64_t)tile * NDIR + d) * MGC_TV + v];
                if (!(r > 0.0)) continue;
                if (mgc_tol_arc_open(r, tol, su, scale[(int64_t)ntile * MGC_TV + nloc])) m |= 1u << d;
                else closed++;
            }
        }
        omask[(int64_t)tile * MGC_TV + v] = (Mask)m;
    }
    return closed;
}

#if defined(__HIPCC__)

template <int NDIR>
__global__ __launch_bounds__(MGC_TV) void k_reach_scale(MgcLattice L, double* scale, unsigned long long* info)
{
    double most = 0.0;
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        const double m = mgc_reach_scale_tile<NDIR>(L, L.rcap, scale, tile, (int)threadIdx.x, MGC_TV);
        if (m > most) most = m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(most, off, 64);
        if (o > most) most = o;
    }
    if ((threadIdx.x & 63) == 0 && most > 0.0) atomicMax(info + MGC_REACHT_SCALE_MAX, (unsigned long long)__double_as_longlong(most));
}

template <int NDIR>
__global__ __launch_bounds__(MGC_TV) void k_reach_open(MgcLattice L, const double* scale, double tol, void* omask, unsigned long long* info)
{
    int closed = 0;
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        if (NDIR == 6) closed += mgc_reach_open_tile<6>(L, L.rcap, scale, tol, (uint8_t*)omask, tile, (int)threadIdx.x, MGC_TV);
        else closed += mgc_reach_open_tile<26>(L, L.rcap, scale, tol, (uint32_t*)omask, tile, (int)threadIdx.x, MGC_TV);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) closed += __shfl_down(closed, off, 64);
    if ((threadIdx.x & 63) == 0 && closed) atomicAdd(info + MGC_REACHT_ARCS_CLOSED, (unsigned long long)closed);
}

/* One wave per tile, lane = row (z, y) of eight voxels, as k_reach_seed.  BACK = false: the source seeds, excess open at tol; tsum as
 * in k_reach_seed (from_source(tol) is a part of from_source(0), so a tile wholly on the sink side still holds none) or NULL.
 * BACK = true: the sink seeds, the residual sink link open at tol; no label, no summary.  tr0 and sink are read under the flag rule of
 * DESIGN 10 (tflags; status MGC_ST_SINK) and count as 0 elsewhere; the full neighbourhood writes both planes everywhere.  The mark plane
 * arrives zeroed; padding voxels are never marked.  seeded / skipped / closed: the info slots to count into. */
template <bool BACK>
__global__ __launch_bounds__(256) void k_reach_seed_tol(MgcLattice L, const uint8_t* tflags, const double* tr0, const double* scale, double tol, const uint8_t* tsum,
                                                        uint8_t* marks, int list, int cnt, unsigned long long* seeded_out, unsigned long long* skipped_out,
                                                        unsigned long long* closed_out)
{
    const int lane = threadIdx.x & 63;
    unsigned long long seeded = 0, skipped = 0;
    int closed = 0;
    for (int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); tile < L.ntiles; tile += (int)gridDim.x * 4) {
        int64_t z, y, x0;
        const int nx = mgc_reach_row(L, tile, lane, z, y, x0);
        if (!BACK && tsum && tsum[tile] == 0) { /* (wave-uniform) */
            skipped++;
            continue;
        }
        const bool tr0_ok = L.ndir != 6 || tflags[tile] != 0;
        if (BACK && L.ndir == 6 && !(L.status[tile] & MGC_ST_SINK)) continue; /* (wave-uniform) no residual sink link in this tile */
        const int64_t at = (int64_t)tile * MGC_TV + lane * 8;
        const double* cp = (BACK ? L.sink : L.excess) + at;
        unsigned long long m = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= nx) continue;
            const double c = cp[k];
            if (!(c > 0.0)) continue;
            if (mgc_tol_tlink_open(c, tol, tr0_ok ? tr0[at + k] : 0.0, scale[at + k])) m |= 1ull << (8 * k);
            else closed++;
        }
        if (m) *(unsigned long long*)(marks + at) = m;
        if (__ballot(m != 0ull) != 0ull) {
            if (lane == 0) mgc_reach_append(L, list, cnt, tile);
            seeded++;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) closed += __shfl_down(closed, off, 64);
    if (lane == 0) {
        if (seeded) atomicAdd(seeded_out, seeded);
        if (skipped && skipped_out) atomicAdd(skipped_out, skipped);
        if (closed) atomicAdd(closed_out, (unsigned long long)closed);
    }
}

/* One wave per tile, lane = row (z, y): the two mark planes to C order.  from_source = forward mark, to_sink = backward mark,
 * ambiguous = neither, not_sink = !to_sink (the "source side" plane of the cut around V \ R_t); each output may be NULL.
 * cnt3[3 * tile + {0, 1, 2}] = voxels of the tile from the source / to the sink / ambiguous. */
__global__ __launch_bounds__(256) void k_reach_readout_tol(MgcLattice L, const uint8_t* fwd, const uint8_t* bwd, uint8_t* from_source, uint8_t* to_sink, uint8_t* ambiguous,
                                                           uint8_t* not_sink, int32_t* cnt3)
{
    const int lane = threadIdx.x & 63;
    const bool rows8 = L.dx % 8 == 0;
    for (int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); tile < L.ntiles; tile += (int)gridDim.x * 4) {
        int64_t z, y, x0;
        const int nx = mgc_reach_row(L, tile, lane, z, y, x0);
        const unsigned long long ones = 0x0101010101010101ull;
        const unsigned long long inside = nx >= 8 ? ones : (ones & ((1ull << (8 * nx)) - 1ull));
        unsigned long long f = *(const unsigned long long*)(fwd + (int64_t)tile * MGC_TV + lane * 8);
        unsigned long long b = *(const unsigned long long*)(bwd + (int64_t)tile * MGC_TV + lane * 8);
        f &= inside; /* (a mark is the byte 1; padding voxels carry none, the mask says so once more) */
        b &= inside;
        const unsigned long long am = inside & ~(f | b), ns = inside & ~b;
        int n_fs = __popcll(f), n_ts = __popcll(b), n_am = __popcll(am);
        if (nx > 0) {
            const int64_t at = (z * L.dy + y) * L.dx + x0;
            if (rows8) {
                if (from_source) *(unsigned long long*)(from_source + at) = f;
                if (to_sink) *(unsigned long long*)(to_sink + at) = b;
                if (ambiguous) *(unsigned long long*)(ambiguous + at) = am;
                if (not_sink) *(unsigned long long*)(not_sink + at) = ns;
            } else {
                for (int k = 0; k < nx; ++k) {
                    if (from_source) from_source[at + k] = (uint8_t)((f >> (8 * k)) & 1ull);
                    if (to_sink) to_sink[at + k] = (uint8_t)((b >> (8 * k)) & 1ull);
                    if (ambiguous) ambiguous[at + k] = (uint8_t)((am >> (8 * k)) & 1ull);
                    if (not_sink) not_sink[at + k] = (uint8_t)((ns >> (8 * k)) & 1ull);
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n_fs += __shfl_down(n_fs, off, 64);
            n_ts += __shfl_down(n_ts, off, 64);
            n_am += __shfl_down(n_am, off, 64);
        }
        if (lane == 0) {
            cnt3[3 * (int64_t)tile + 0] = n_fs;
            cnt3[3 * (int64_t)tile + 1] = n_ts;
            cnt3[3 * (int64_t)tile + 2] = n_am;
        }
    }
}

#endif /* __HIPCC__ */

#endif /* MGC_REACH_TOL_OPS_INL */
