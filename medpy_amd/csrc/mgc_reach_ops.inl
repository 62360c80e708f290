/*
 * mgc_reach_ops.inl -- the source side of the minimum cut and the ambiguity set of a solved lattice (mgc_cut_sets); DESIGN 13.
 *
 * A converged solve leaves a maximum PREFLOW in HBM: every voxel that still holds excess stands at MGC_HINF, no flow is in flight,
 * and bit d of a voxel's mask says that its residual arc in direction d is open (rcap[d] > 0).  R_t, the voxels that can reach the
 * sink, is what the labels report (height < MGC_HINF).  R_s, the voxels the source can reach in the residual graph of the maximum
 * flow this preflow turns into, is the set reachable from {excess > 0} along open arcs (the argument: DESIGN 13): one forward flood,
 * the mirror image of the global relabel -- it starts from the excess instead of the sink and follows the arcs the way they point.
 * What is in neither set is the AMBIGUITY SET: the voxels some minimum cut puts on either side.
 *
 *   k_reach_seed     one wave per tile: tiles wholly on the sink side are skipped, the others mark their excess > 0 voxels in a
 *                    tile-major byte plane and go on the first work list
 *   k_reach_flood    one workgroup per listed tile: own marks and masks plus the one-voxel halo of the neighbours' marks AND masks
 *                    in LDS, a fixpoint inside the tile, then the neighbour tiles an open arc leads into are queued (stamp de-duplicated);
 *                    <NDIR, BACK>: BACK follows the arcs against their direction (the sink side of mgc_cut_sets_tol, mgc_reach_tol_ops.inl)
 *   k_reach_readout  marks -> C order (from_source) and ambiguous = !mark && height == MGC_HINF, three counts per tile
 *   k_reach_sum      the per-tile counts in a fixed order
 *
 * The step of ONE tile, mgc_reach_tile_step<NDIR, BACK>, is plain C++ over (first index, stride, barrier): the kernel runs it with 512
 * threads and __syncthreads_or, the stand-alone host programs of the CPU test tier (tests/hostsim/reach_main.cpp, reach_tol_main.cpp)
 * with one thread and no barrier.  Only mgc_common.h is needed on the host.
 */
#ifndef MGC_REACH_OPS_INL
#define MGC_REACH_OPS_INL

#include "mgc_common.h"

#define MGC_REACH_BLOCK 1000            /* the 10 x 10 x 10 cells around (and including) a tile */
#define MGC_REACH_VALID 0x80000000u     /* cell flag next to the mask bits: a voxel of the volume that this neighbourhood can reach from the tile */
/* slots of the info block (mgc_get_cut_sets_info) */
#define MGC_REACH_N_SOURCE 0
#define MGC_REACH_N_SINK 1
#define MGC_REACH_N_AMBIGUOUS 2
#define MGC_REACH_PASSES 3
#define MGC_REACH_VISITS 4
#define MGC_REACH_SEEDED 5
#define MGC_REACH_SKIPPED 6

/* offset of direction d (6: 0 = -x .. 5 = +z; 26: the encoding of mgc26_offset) and the direction that points back */
template <int NDIR>
MGC_HD void mgc_reach_offset(int d, int& dz, int& dy, int& dx)
{
    if (NDIR == 6) {
        dz = (d >> 1) == 2 ? ((d & 1) ? 1 : -1) : 0;
        dy = (d >> 1) == 1 ? ((d & 1) ? 1 : -1) : 0;
        dx = (d >> 1) == 0 ? ((d & 1) ? 1 : -1) : 0;
    } else {
        const int c = d < 13 ? d : d + 1;
        dz = c / 9 - 1;
        dy = (c / 3) % 3 - 1;
        dx = c % 3 - 1;
    }
}
template <int NDIR>
MGC_HD int mgc_reach_opposite(int d) { return NDIR == 6 ? (d ^ 1) : 25 - d; }

/* cell of the block that holds local voxel (z, y, x), -1 <= z, y, x <= 8 */
MGC_HD int mgc_reach_cell(int z, int y, int x) { return ((z + 1) * 10 + (y + 1)) * 10 + (x + 1); }

/* Where block cell k of tile (tz, ty, tx) lives: its tile (loc = its local index there), or -1 for a cell that can never carry a
 * mark into this tile nor take one from it: outside the tile grid, a padding voxel of a partial tile, or (6-neighbourhood) a cell
 * of the block's edges and corners. */
template <int NDIR>
MGC_HD int mgc_reach_cell_home(const MgcLattice& L, int tz, int ty, int tx, int k, int& loc)
{
    const int bz = k / 100 - 1, by = (k / 10) % 10 - 1, bx = k % 10 - 1;
    const int oz = bz < 0 ? -1 : (bz > 7 ? 1 : 0), oy = by < 0 ? -1 : (by > 7 ? 1 : 0), ox = bx < 0 ? -1 : (bx > 7 ? 1 : 0);
    loc = 0;
    if (NDIR == 6 && (oz != 0) + (oy != 0) + (ox != 0) > 1) return -1;
    const int nz = tz + oz, ny = ty + oy, nx = tx + ox;
    if (nz < 0 || nz >= L.gz || ny < 0 || ny >= L.gy || nx < 0 || nx >= L.gx) return -1;
    const int lz = bz & 7, ly = by & 7, lx = bx & 7;
    if ((int64_t)nz * 8 + lz >= L.dz || (int64_t)ny * 8 + ly >= L.dy || (int64_t)nx * 8 + lx >= L.dx) return -1;
    loc = mgc_local(lz, ly, lx);
    return mgc_tile_id(L, nz, ny, nx);
}

/* Does an open arc lead into cell `me` from a marked cell?  The arc n -> me is open iff the bit of N's mask for the direction
 * n -> me is set: the neighbour's mask, not me's own (residual capacities are not symmetric). */
template <int NDIR>
MGC_HD bool mgc_reach_pull(const uint8_t* mk, const uint32_t* ms, int me)
{
    for (int d = 0; d < NDIR; ++d) {
        int dz, dy, dx;
        mgc_reach_offset<NDIR>(d, dz, dy, dx);
        const int n = me + (dz * 10 + dy) * 10 + dx;
        if (mk[n] && ((ms[n] >> mgc_reach_opposite<NDIR>(d)) & 1u)) return true;
    }
    return false;
}

/* The neighbour tiles a marked voxel (z, y, x) of the tile opens an arc into, towards a voxel that is staged as unmarked: bit
 * (oz + 1) * 9 + (oy + 1) * 3 + (ox + 1) per neighbour tile. */
template <int NDIR>
MGC_HD uint32_t mgc_reach_wake(const uint8_t* mk, const uint32_t* ms, int z, int y, int x)
{
    const uint32_t m = ms[mgc_reach_cell(z, y, x)];
    uint32_t w = 0;
    for (int d = 0; d < NDIR; ++d) {
        if (!((m >> d) & 1u)) continue;
        int dz, dy, dx;
        mgc_reach_offset<NDIR>(d, dz, dy, dx);
        const int nz = z + dz, ny = y + dy, nx = x + dx;
        const int oz = nz < 0 ? -1 : (nz > 7 ? 1 : 0), oy = ny < 0 ? -1 : (ny > 7 ? 1 : 0), ox = nx < 0 ? -1 : (nx > 7 ? 1 : 0);
        if (!(oz | oy | ox)) continue;
        const int n = mgc_reach_cell(nz, ny, nx);
        if ((ms[n] & MGC_REACH_VALID) && !mk[n]) w |= 1u << ((oz + 1) * 9 + (oy + 1) * 3 + (ox + 1));
    }
    return w;
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

/* The flood step of ONE tile, run by `nt` workers of which this is number t0; sync(v) is a barrier that returns the OR of every
 * worker's v (one worker: the identity).  mk / ms: MGC_REACH_BLOCK cells shared by the workers.  marks: the tile-major mark plane,
 * masks: a tile-major mask plane in the bit layout of L.rmask (6 directions) or L.rmask32 (26).  Returns the worker's share of the
 * wake bits (mgc_reach_wake / mgc_reach_wake_back), to be OR-ed.
 *   BACK = false, the default, follows the arcs the way they point: `me` gets a mark when a marked neighbour n exists and the arc n -> me is open,
 *   the NEIGHBOUR's bit towards me.  BACK = true follows them against their direction: `me` gets a mark when a marked neighbour n
 *   exists and the arc me -> n is open, MY OWN bit towards the neighbour.  Staging, fixpoint and write-back are the same.
 *   Marks only ever go 0 -> 1.  A worker may therefore read a cell another one is marking in the same sweep, and a tile may read a
 *   halo mark its neighbour is writing in the same launch: a stale 0 costs one more sweep or one more visit -- whoever marks a
 *   border voxel with an open arc (in the flood's direction) between it and an unmarked neighbour voxel queues that neighbour for the
 *   NEXT launch, which sees the mark -- never a wrong set.  The same reasoning as for the labels of a relabel pass, which only ever
 *   go down.
 *   The wake test runs over every marked voxel of the tile, not only the ones this visit marked: the seed voxels of the first
 *   pass were marked by the seeding kernel.  A queued neighbour marks at least the voxel it was queued for (it is a voxel of the
 *   volume and the arc is open) unless somebody did so meanwhile, so the lists run empty. */
template <int NDIR, bool BACK = false, class Mask, class Sync>
MGC_HD uint32_t mgc_reach_tile_step(const MgcLattice& L, uint8_t* marks, const Mask* masks, int tile, uint8_t* mk, uint32_t* ms, int t0, int nt, Sync& sync)
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
            if (!mk[me] && (ms[me] & MGC_REACH_VALID) && (BACK ? mgc_reach_pull_back<NDIR>(mk, ms, me) : mgc_reach_pull<NDIR>(mk, ms, me))) {
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
        wake |= BACK ? mgc_reach_wake_back<NDIR>(mk, ms, z, y, x) : mgc_reach_wake<NDIR>(mk, ms, z, y, x);
    }
    return wake;
}

/* the neighbour tile of wake bit c, or -1 outside the grid */
MGC_HD int mgc_reach_wake_tile(const MgcLattice& L, int tile, int c)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    const int nz = tz + c / 9 - 1, ny = ty + (c / 3) % 3 - 1, nx = tx + c % 3 - 1;
    if (c == 13 || nz < 0 || nz >= L.gz || ny < 0 || ny >= L.gy || nx < 0 || nx >= L.gx) return -1;
    return mgc_tile_id(L, nz, ny, nx);
}

#if defined(__HIPCC__)

struct MgcReachBarrier {
    __device__ __forceinline__ int operator()(int v) const { return __syncthreads_or(v); }
};

/* The row of the one-wave-per-tile kernels: lane = row (z, y) of eight voxels of `tile`, x0 its first x.  Returns the number of the
 * row's voxels that lie inside the volume (0 for a padding row). */
__device__ __forceinline__ int mgc_reach_row(const MgcLattice& L, int tile, int lane, int64_t& z, int64_t& y, int64_t& x0)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    z = (int64_t)tz * 8 + (lane >> 3), y = (int64_t)ty * 8 + (lane & 7), x0 = (int64_t)tx * 8;
    return !(z < L.dz && y < L.dy) ? 0 : (L.dx - x0 < 8 ? (int)(L.dx - x0) : 8);
}

/* `tile` on list `list`, counted in counter slot `cnt`, in the shard of this workgroup */
__device__ __forceinline__ void mgc_reach_append(const MgcLattice& L, int list, int cnt, int tile)
{
    const int sh = (int)(blockIdx.x & (unsigned)(L.nshard - 1));
    const int pos = atomicAdd(mgc_counter(L, cnt, sh), 1);
    L.list[list][(int64_t)sh * L.shard_cap + pos] = tile;
}

/* One wave per tile, lane = row (z, y) of eight voxels.  tsum: the label summaries k_labels8 left (0: every voxel of the tile can
 * reach the sink -- no voxel of R_s lives there, the tile is skipped unread) or NULL where the read-out keeps none (rows that are
 * no whole runs of eight): the wave then looks at the tile's labels itself.  Padding voxels of partial tiles are never marked.
 * The mark plane arrives zeroed. */
__global__ __launch_bounds__(256) void k_reach_seed(MgcLattice L, const uint8_t* tsum, uint8_t* marks, int list, int cnt, unsigned long long* info)
{
    const int lane = threadIdx.x & 63;
    unsigned long long seeded = 0, skipped = 0; /* (lane 0 of each wave) */
    for (int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); tile < L.ntiles; tile += (int)gridDim.x * 4) {
        int64_t z, y, x0;
        const int nx = mgc_reach_row(L, tile, lane, z, y, x0);
        bool skip;
        if (tsum) skip = tsum[tile] == 0;
        else {
            const int4* hp = (const int4*)(L.height + (int64_t)tile * MGC_TV + lane * 8);
            const int4 a = hp[0], b = hp[1];
            const int32_t hv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            bool inf = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) inf = inf || (k < nx && hv[k] >= MGC_HINF);
            skip = __ballot(inf) == 0ull;
        }
        if (skip) { /* (wave-uniform) */
            skipped++;
            continue;
        }
        const double* ep = L.excess + (int64_t)tile * MGC_TV + lane * 8;
        unsigned long long m = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nx && ep[k] > 0.0) m |= 1ull << (8 * k);
        if (m) *(unsigned long long*)(marks + (int64_t)tile * MGC_TV + lane * 8) = m;
        if (__ballot(m != 0ull) != 0ull) {
            if (lane == 0) mgc_reach_append(L, list, cnt, tile);
            seeded++;
        }
    }
    if (lane == 0) {
        if (seeded) atomicAdd(info + MGC_REACH_SEEDED, seeded);
        if (skipped) atomicAdd(info + MGC_REACH_SKIPPED, skipped);
    }
}

/* One workgroup per tile of list `list` (length in counter slot `cnt`): mgc_reach_tile_step<NDIR, BACK> on the mask plane `masks`
 * (uint8_t for 6 directions, uint32_t for 26: the stored L.rmask / L.rmask32 or a thresholded plane), then every neighbour tile the
 * step's wake bits name goes on list `next` unless this pass (stamp == epoch) has queued it already.  info: passes at [0], visits at
 * [1].  A pass over an empty list does nothing. */
template <int NDIR, bool BACK>
__global__ __launch_bounds__(MGC_TV) void k_reach_flood(MgcLattice L, const void* masks, uint8_t* marks, uint32_t* stamp, int list, int cnt, uint32_t epoch, int next, unsigned long long* info)
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
        if (NDIR == 6) wake = mgc_reach_tile_step<6, BACK>(L, marks, (const uint8_t*)masks, tile, mk, ms, t, MGC_TV, barrier);
        else wake = mgc_reach_tile_step<26, BACK>(L, marks, (const uint32_t*)masks, tile, mk, ms, t, MGC_TV, barrier);
        if (wake) atomicOr(&wake_all, wake);
        __syncthreads();
        const uint32_t w = wake_all;
        if (t < 27 && ((w >> t) & 1u)) {
            const int nt = mgc_reach_wake_tile(L, tile, t);
            if (nt >= 0 && atomicExch(stamp + nt, epoch) != epoch) mgc_reach_append(L, next, next, nt);
        }
        __syncthreads(); /* (the next tile of this workgroup rewrites the block and the wake word) */
    }
}

/* One wave per tile, lane = row (z, y): the marks to C order and ambiguous = neither marked nor able to reach the sink; either
 * output may be NULL.  cnt3[3 * tile + {0, 1, 2}] = voxels of the tile from the source / to the sink / ambiguous. */
__global__ __launch_bounds__(256) void k_reach_readout(MgcLattice L, const uint8_t* marks, uint8_t* from_source, uint8_t* ambiguous, int32_t* cnt3)
{
    const int lane = threadIdx.x & 63;
    const bool rows8 = L.dx % 8 == 0;
    for (int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); tile < L.ntiles; tile += (int)gridDim.x * 4) {
        int64_t z, y, x0;
        const int nx = mgc_reach_row(L, tile, lane, z, y, x0);
        const unsigned long long m = *(const unsigned long long*)(marks + (int64_t)tile * MGC_TV + lane * 8);
        const int4* hp = (const int4*)(L.height + (int64_t)tile * MGC_TV + lane * 8);
        const int4 a = hp[0], b = hp[1];
        const int32_t hv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        unsigned long long fs = 0ull, am = 0ull;
        int n_fs = 0, n_ts = 0, n_am = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= nx) continue;
            const bool marked = ((m >> (8 * k)) & 0xffull) != 0ull, sink = hv[k] < MGC_HINF;
            if (marked) { fs |= 1ull << (8 * k); n_fs++; }
            if (sink) n_ts++;
            if (!marked && !sink) { am |= 1ull << (8 * k); n_am++; }
        }
        if (nx > 0) {
            const int64_t at = (z * L.dy + y) * L.dx + x0;
            if (rows8) {
                if (from_source) *(unsigned long long*)(from_source + at) = fs;
                if (ambiguous) *(unsigned long long*)(ambiguous + at) = am;
            } else {
                for (int k = 0; k < nx; ++k) {
                    if (from_source) from_source[at + k] = (uint8_t)((fs >> (8 * k)) & 1ull);
                    if (ambiguous) ambiguous[at + k] = (uint8_t)((am >> (8 * k)) & 1ull);
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

/* one workgroup: the three per-tile counts summed in a fixed order (thread t takes tiles t, t + 512, ...; then a tree) */
__global__ __launch_bounds__(MGC_TV) void k_reach_sum(const int32_t* cnt3, int ntiles, unsigned long long* info)
{
    __shared__ unsigned long long s[3][MGC_TV];
    const int t = threadIdx.x;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    for (int tile = t; tile < ntiles; tile += MGC_TV)
        for (int k = 0; k < 3; ++k) acc[k] += (unsigned long long)cnt3[3 * (int64_t)tile + k];
    for (int k = 0; k < 3; ++k) s[k][t] = acc[k];
    __syncthreads();
    for (int off = MGC_TV / 2; off > 0; off >>= 1) {
        if (t < off)
            for (int k = 0; k < 3; ++k) s[k][t] += s[k][t + off];
        __syncthreads();
    }
    if (t < 3) info[MGC_REACH_N_SOURCE + t] = s[t][0];
}

#endif /* __HIPCC__ */

#endif /* MGC_REACH_OPS_INL */
