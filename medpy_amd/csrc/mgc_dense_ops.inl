/*
 * mgc_dense_ops.inl -- whole n-link weight arrays of a user-defined boundary term (mgc_add_nweights): one array per
 * lattice offset in C order, checked on the device, put into a tile-major STORE that stays with the handle, and added to the
 * residual graph by every build.  Build-side kernels only: the solver does not know where a capacity came from.
 *
 *   k_dense_check       every entry that feeds an arc must be finite and >= 0; the first offender's index comes back
 *   k_dense_accumulate  C-order array(s) of one offset -> += into two direction planes of the store
 *   k_dense_apply       mgc_build: rcap += store, cap0 += store, masks, "is every n-link of the volume residual?"
 *
 * Semantics: Graph::sum_edge (graph.h:457-480) -- an arc's capacity is the sum of what it was given, added ONE AFTER THE OTHER in
 * call order as f64, on top of the weight of the built-in term.  The first array a direction plane receives goes into the store
 * proper (the layout of cap0); an array that reaches a plane which already holds one gets a plane of its own (MgcDenseLayers),
 * because (built + w1) + w2 is not built + (w1 + w2) in floating point and the built weight is only known at the build.
 */
#ifndef MGC_DENSE_OPS_INL
#define MGC_DENSE_OPS_INL

#include <float.h>

#define MGC_DENSE_NONE (~0ull)
#define MGC_DENSE_ROW 72 /* LDS row pitch of the 64 x 64 staging block in doubles: the eight rows a wave reads back lie 16 banks apart */

MGC_HD bool mgc_dense_inside(const MgcLattice& L, int64_t z, int64_t y, int64_t x)
{
    return z >= 0 && z < L.dz && y >= 0 && y < L.dy && x >= 0 && x < L.dx;
}

/* One pass over the uploaded array(s) of offset (oz, oy, ox): entry p counts when p + offset lies inside the volume (the rule of
 * k_get_nweights_offset; what an ignored entry holds is never looked at beyond the load).  A wave takes whole x-rows, so the division
 * that finds (z, y) is per row.  key = 2 * flat index + (0: there, 1: back); the lowest bad key of a wave is found with shuffles
 * when its ballot says there is one, the waves of a workgroup meet in LDS, and one atomic min per workgroup reaches *first. */
template <class T>
__global__ __launch_bounds__(256) void k_dense_check(MgcLattice L, const T* __restrict__ there, const T* __restrict__ back, int oz, int oy, int ox,
                                                    unsigned long long* first)
{
    __shared__ unsigned long long wave_min[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t rows = L.dz * L.dy;
    unsigned long long best = MGC_DENSE_NONE;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t y = r % L.dy, z = r / L.dy;
        if (z + oz < 0 || z + oz >= L.dz || y + oy < 0 || y + oy >= L.dy) continue; /* (uniform over the wave) */
        for (int64_t x = lane; x < L.dx; x += 64) {
            if (x + ox < 0 || x + ox >= L.dx) continue;
            const int64_t id = r * L.dx + x;
            const double a = (double)there[id];
            if (!(a >= 0.0 && a <= DBL_MAX) && 2ull * (unsigned long long)id < best) best = 2ull * (unsigned long long)id;
            if (back) {
                const double b = (double)back[id];
                if (!(b >= 0.0 && b <= DBL_MAX) && 2ull * (unsigned long long)id + 1ull < best) best = 2ull * (unsigned long long)id + 1ull;
            }
        }
    }
    if (__ballot(best != MGC_DENSE_NONE) != 0ull) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o = __shfl_xor(best, s);
            if (o < best) best = o;
        }
    }
    if (lane == 0) wave_min[wv] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k)
            if (wave_min[k] < best) best = wave_min[k];
        if (best != MGC_DENSE_NONE) atomicMin(first, best);
    }
}

/* One call of mgc_add_nweights: plane d (the arcs v -> v + offset) receives there[v], plane dr (the arcs v -> v - offset) receives
 * back[v - offset] (`back` NULL: there[v - offset]).  The mapping goes by the DESTINATION voxel v, so every slot has one writer and
 * the kernel needs no atomics.  A workgroup owns a STRIP of up to eight tiles that are neighbours along x -- 64 x 8 x 8 voxels --
 * and a wave reads whole 512-byte x-rows of the strip from the C-order array (eight rows each, all sixteen loads of a lane in
 * flight before the first is used); the rows meet in LDS and leave tile by tile as the 4 KiB streams of the tile-major layout.
 * Read tile by tile instead, a wave would fetch eight separate 64-byte pieces per load.
 * Plane p of tile `tile` starts at base_p + tile * stride_p (the store proper: stride ndir * 512; a plane of its own: 512).
 * Padding voxels and voxels whose neighbour is outside the volume add +0.0, which changes nothing (the store holds no -0.0). */
template <class T>
__global__ __launch_bounds__(MGC_TV) void k_dense_accumulate(MgcLattice L, const T* __restrict__ there, const T* __restrict__ back, int oz, int oy, int ox,
                                                            double* base_d, int64_t stride_d, double* base_r, int64_t stride_r)
{
    __shared__ double stage[64 * MGC_DENSE_ROW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const T* const rev = back ? back : there;
    const int gxs = (L.gx + 7) / 8;
    const int nstrips = L.gz * L.gy * gxs;
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        const int xs = s % gxs, ty = (s / gxs) % L.gy, tz = s / (gxs * L.gy);
        const int64_t x = (int64_t)xs * 64 + lane;
        double a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = wv * 8 + k; /* row (lz, ly) of the strip */
            const int64_t z = (int64_t)tz * 8 + (r >> 3), y = (int64_t)ty * 8 + (r & 7);
            a[k] = 0.0;
            b[k] = 0.0;
            if (mgc_dense_inside(L, z, y, x)) {
                if (mgc_dense_inside(L, z + oz, y + oy, x + ox)) a[k] = (double)there[(z * L.dy + y) * L.dx + x];
                if (mgc_dense_inside(L, z - oz, y - oy, x - ox)) b[k] = (double)rev[((z - oz) * L.dy + (y - oy)) * L.dx + (x - ox)];
            }
        }
        const int ntl = L.gx - xs * 8 < 8 ? L.gx - xs * 8 : 8;
        const int64_t tile0 = ((int64_t)tz * L.gy + ty) * L.gx + (int64_t)xs * 8;
        const int back_at = (t >> 3) * MGC_DENSE_ROW + (t & 7); /* this voxel's slot in the first tile of the strip */
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int k = 0; k < 8; ++k) stage[(wv * 8 + k) * MGC_DENSE_ROW + lane] = half ? b[k] : a[k];
            __syncthreads();
            double* const base = half ? base_r : base_d;
            const int64_t stride = half ? stride_r : stride_d;
            for (int j = 0; j < ntl; ++j) {
                double* const p = base + (tile0 + j) * stride + t;
                *p = *p + stage[back_at + j * 8];
            }
            __syncthreads();
        }
    }
}

/* the planes that hold the second, third ... array a direction received: plane[k * ndir + d] (tile-major, 512 per tile) or NULL */
struct MgcDenseLayers {
    const double* const* plane;
    int n; /* layers */
};

/* mgc_build, behind k_build and in front of k_add_edges: one workgroup per tile.  rcap += store and cap0 += store are two adds --
 * the pre-push of a build with a regional term has already moved flow, rcap != cap0 there, and that flow stays.  The masks are
 * rebuilt (sink bit: the rule of k_refresh_mask), and MGC_CNT_NOT_FULL counts the tiles that hold an arc inside the volume which is
 * not residual now (mgc_build cleared the word: what k_build counted there was the graph without the store). */
template <bool FULL>
__global__ __launch_bounds__(MGC_TV) void k_dense_apply(MgcLattice L, const double* __restrict__ dense, MgcDenseLayers X)
{
    constexpr int NDIR = FULL ? MGC26_NDIR : MGC_NDIR;
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        const int t = threadIdx.x;
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        const int64_t gz = (int64_t)tz * 8 + (t >> 6), gy = (int64_t)ty * 8 + ((t >> 3) & 7), gx = (int64_t)tx * 8 + (t & 7);
        const bool valid = mgc_dense_inside(L, gz, gy, gx);
        const bool snk = (FULL || (L.status[tile] & MGC_ST_SINK)) && L.sink[(int64_t)tile * MGC_TV + t] > 0.0;
        uint32_t m = 0;
        bool not_full = false;
        for (int d = 0; d < NDIR; ++d) {
            const int64_t o = ((int64_t)tile * NDIR + d) * MGC_TV + t;
            double r = L.rcap[o], c = L.cap0[o];
            const double w = dense[o];
            r = r + w;
            c = c + w;
            for (int k = 0; k < X.n; ++k) {
                const double* const p = X.plane[k * NDIR + d];
                if (p) {
                    const double wk = p[(int64_t)tile * MGC_TV + t];
                    r = r + wk;
                    c = c + wk;
                }
            }
            L.rcap[o] = r;
            L.cap0[o] = c;
            if (r > 0.0) m |= 1u << d;
            int dz, dy, dx;
            if (FULL) mgc26_offset(d, dz, dy, dx);
            else {
                dz = (d >> 1) == 2 ? ((d & 1) ? 1 : -1) : 0;
                dy = (d >> 1) == 1 ? ((d & 1) ? 1 : -1) : 0;
                dx = (d >> 1) == 0 ? ((d & 1) ? 1 : -1) : 0;
            }
            if (valid && mgc_dense_inside(L, gz + dz, gy + dy, gx + dx) && !(r > 0.0)) not_full = true;
        }
        if (FULL) L.rmask32[(int64_t)tile * MGC_TV + t] = m | (snk ? MGC26_MASK_SINK : 0u);
        else L.rmask[(int64_t)tile * MGC_TV + t] = (uint8_t)(m | (snk ? MGC_MASK_SINK : 0));
        if (__syncthreads_or((int)not_full) && t == 0) atomicAdd(&L.count[MGC_CNT_NOT_FULL], 1);
    }
}

#endif /* MGC_DENSE_OPS_INL */
