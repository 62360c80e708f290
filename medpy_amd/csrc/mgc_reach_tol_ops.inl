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
 *   (forward flood)     k_reach_flood of mgc_reach_ops.inl as it is, on a lattice whose mask pointer is the thresholded plane
 *   k_reach_flood_back  one workgroup per listed tile: mgc_reach_tile_step_back, the mirror image of the forward step
 *   k_reach_readout_tol the two mark planes -> C order: from_source, to_sink, ambiguous, and the plane "not to_sink" the cut value
 *                       kernel reads; three counts per tile for k_reach_sum
 *
 * The steps of ONE tile are plain C++ over (first index, stride[, barrier]) as in mgc_reach_ops.inl: the kernels run them with 512
 * threads, tests/hostsim/reach_tol_main.cpp with one.
 */
#ifndef MGC_REACH_TOL_OPS_INL
#define MGC_REACH_TOL_OPS_INL

#include "mgc_reach_ops.inl"
#include "mgc_reach_tol.h"

/* slots of the info block (mgc_get_cut_sets_tol_info): 0 .. 2 the counts as in mgc_reach_ops.inl, 3 .. 5 passes / visits / seeded tiles
 * of the forward flood (the slots k_reach_flood writes), then: */
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

/* Can cell `me` step along an open arc of ITS OWN into a marked cell?  (Backward: me reaches the sink if somebody it has an open arc
 * to does.)  A bit towards a cell that is no voxel of the volume finds that cell unmarked. */
template <int NDIR>
MGC_HD bool mgc_reach_pull_back(const uint8_t* mk, const uint32_t* ms, int me)
{
    const uint32_t m = ms[me];
    for (int d = 0; d < NDIR; ++d) {
        if (!((m >> d) & 1u)) continue;
        int dz, dy, dx;
        mgc_reach_offset<NDIR>(d, dz, dy, dx);
        if (mk[me + (dz * 10 + dy) * 10 + dx]) return true;
    }
    return false;
}

/* The neighbour tiles that hold an unmarked voxel with an open arc INTO the marked voxel (z, y, x) of this tile, judged by the
 * neighbour voxel's staged mask: the wake bits of mgc_reach_wake. */
template <int NDIR>
MGC_HD uint32_t mgc_reach_wake_back(const uint8_t* mk, const uint32_t* ms, int z, int y, int x)
{
    uint32_t w = 0;
    for (int d = 0; d < NDIR; ++d) {
        int dz, dy, dx;
        mgc_reach_offset<NDIR>(d, dz, dy, dx);
        const int nz = z + dz, ny = y + dy, nx = x + dx;
        const int oz = nz < 0 ? -1 : (nz > 7 ? 1 : 0), oy = ny < 0 ? -1 : (ny > 7 ? 1 : 0), ox = nx < 0 ? -1 : (nx > 7 ? 1 : 0);
        if (!(oz | oy | ox)) continue;
        const int n = mgc_reach_cell(nz, ny, nx);
        if ((ms[n] & MGC_REACH_VALID) && !mk[n] && ((ms[n] >> mgc_reach_opposite<NDIR>(d)) & 1u)) w |= 1u << ((oz + 1) * 9 + (oy + 1) * 3 + (ox + 1));
    }
    return w;
}

/* The backward flood step of ONE tile: mgc_reach_tile_step with the arcs turned round.  `me` gets a mark when a marked neighbour n
 * exists and the arc me -> n is open: me's own bit.  Staging, fixpoint, the 0 -> 1 argument for races and the reason why the wake test
 * runs over every marked voxel are those of the forward step; a queued neighbour tile marks at least the voxel it was queued for. */
template <int NDIR, class Mask, class Sync>
MGC_HD uint32_t mgc_reach_tile_step_back(const MgcLattice& L, uint8_t* marks, const Mask* masks, int tile, uint8_t* mk, uint32_t* ms, int t0, int nt, Sync& sync)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    for (int k = t0; k < MGC_REACH_BLOCK; k += nt) {
        int loc;
        const int home = mgc_reach_cell_home<NDIR>(L, tz, ty, tx, k, loc);
        uint8_t m = 0;
        uint32_t a = 0;
        if (home >= 0) {
            const int64_t at = (int64_t)home * MGC_TV + loc;
            m = marks[at];
            a = (uint32_t)masks[at] | MGC_REACH_VALID;
        }
        mk[k] = m;
        ms[k] = a;
    }
    sync(0);
    for (;;) {
        int changed = 0;
        for (int v = t0; v < MGC_TV; v += nt) {
            const int me = mgc_reach_cell(v >> 6, (v >> 3) & 7, v & 7);
            if (!mk[me] && (ms[me] & MGC_REACH_VALID) && mgc_reach_pull_back<NDIR>(mk, ms, me)) {
                mk[me] = 1;
                changed = 1;
            }
        }
        if (!sync(changed)) break;
    }
    uint32_t wake = 0;
    for (int v = t0; v < MGC_TV; v += nt) {
        const int z = v >> 6, y = (v >> 3) & 7, x = v & 7;
        if (!mk[mgc_reach_cell(z, y, x)]) continue;
        const int64_t at = (int64_t)tile * MGC_TV + v;
        if (!marks[at]) marks[at] = 1;
        wake |= mgc_reach_wake_back<NDIR>(mk, ms, z, y, x);
    }
    return wake;
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
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        const int64_t z = (int64_t)tz * 8 + (lane >> 3), y = (int64_t)ty * 8 + (lane & 7), x0 = (int64_t)tx * 8;
        const int nx = !(z < L.dz && y < L.dy) ? 0 : (L.dx - x0 < 8 ? (int)(L.dx - x0) : 8); /* voxels of this row inside the volume */
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
            if (lane == 0) {
                const int sh = (int)(blockIdx.x & (unsigned)(L.nshard - 1));
                const int pos = atomicAdd(mgc_counter(L, cnt, sh), 1);
                L.list[list][(int64_t)sh * L.shard_cap + pos] = tile;
            }
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

/* k_reach_flood with the arcs turned round, on the mask plane it is given: one workgroup per tile of list `list`, then every neighbour
 * tile that holds an unmarked voxel with an open arc into a marked border voxel goes on list `next`.  info: passes at [0], visits at [1]. */
template <int NDIR>
__global__ __launch_bounds__(MGC_TV) void k_reach_flood_back(MgcLattice L, const void* omask, uint8_t* marks, uint32_t* stamp, int list, int cnt, uint32_t epoch, int next, unsigned long long* info)
{
    __shared__ uint8_t mk[MGC_REACH_BLOCK];
    __shared__ uint32_t ms[MGC_REACH_BLOCK];
    __shared__ uint32_t wake_all;
    const int t = threadIdx.x;
    MgcListView view;
    const int n = mgc_list_view(L, cnt, view);
    if (blockIdx.x == 0 && t == 0 && n > 0) {
        atomicAdd(info + 0, 1ull);
        atomicAdd(info + 1, (unsigned long long)n);
    }
    MgcReachBarrier barrier;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int tile = mgc_list_at(L, list, view, i);
        if (t == 0) wake_all = 0u;
        uint32_t wake;
        if (NDIR == 6) wake = mgc_reach_tile_step_back<6>(L, marks, (const uint8_t*)omask, tile, mk, ms, t, MGC_TV, barrier);
        else wake = mgc_reach_tile_step_back<26>(L, marks, (const uint32_t*)omask, tile, mk, ms, t, MGC_TV, barrier);
        if (wake) atomicOr(&wake_all, wake);
        __syncthreads();
        const uint32_t w = wake_all;
        if (t < 27 && ((w >> t) & 1u)) {
            const int nt = mgc_reach_wake_tile(L, tile, t);
            if (nt >= 0 && atomicExch(stamp + nt, epoch) != epoch) {
                const int sh = (int)(blockIdx.x & (unsigned)(L.nshard - 1));
                const int pos = atomicAdd(mgc_counter(L, next, sh), 1);
                L.list[next][(int64_t)sh * L.shard_cap + pos] = nt;
            }
        }
        __syncthreads(); /* (the next tile of this workgroup rewrites the block and the wake word) */
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
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        const int64_t z = (int64_t)tz * 8 + (lane >> 3), y = (int64_t)ty * 8 + (lane & 7), x0 = (int64_t)tx * 8;
        const int nx = !(z < L.dz && y < L.dy) ? 0 : (L.dx - x0 < 8 ? (int)(L.dx - x0) : 8);
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
