/*
 * mgc_edt_ops.inl -- the kernels of mgc_distance_transform, mgc_surface_distances and mgc_overlap_counts.  The steps
 * themselves are mgc_edt.h; here they get their waves and workgroups:
 *
 *   k_edt_rows     the last axis: one wave per row, mgc_edt_row_step with the wave's ballot as the seed mask
 *   k_edt_panels   another axis, lines of up to MGC_EDT_PANEL_LINE voxels: one workgroup per panel, mgc_edt_panel_step in LDS, in place
 *   k_edt_long     another axis, longer lines: a thread per voxel, mgc_edt_long_voxel from one plane into a second
 *   k_edt_fill     a plane of one value (+inf: no seed)
 *   k_edt_border   a thread per voxel: mgc_edt_is_border
 *   k_edt_count    one wave per segment of MGC_EDT_COUNT_SEG voxels: the four overlap classes of (p, q), and the voxels of p
 *   (k_labels_delta_scan of mgc_edit_ops.inl turns the counts of p into offsets)
 *   k_edt_reduce   one workgroup: the segments' sums in a fixed order
 *   k_edt_gather   one wave per segment: g[v] of the voxels of p, in ascending voxel id, to out[rank] for rank < cap
 *
 * Every kernel is a template over a parameter E that nothing reads (instantiated as <0>), for the reason mgc_cc_ops.inl gives: the
 * instances of templates are emitted behind all plain kernels, so the kernels of the solve keep their places in the code object.
 *
 * A phase boundary is a kernel boundary.  No kernel here writes a word that another workgroup of the same launch reads: a row, a
 * panel, a voxel of the second plane, a segment's counts and a rank's entry each have one owner.  No atomics on device memory, no
 * waiting between workgroups.
 *
 * LDS: k_edt_panels takes n * MGC_EDT_PANEL_COLS * 8 bytes for lines of n voxels -- 64 KiB at the threshold n = 512, where TWO
 * workgroups are resident on the 160 KiB of a CU (8 waves: LDS is what limits them there, and says so here), 32 KiB and five
 * workgroups at n = 256, 16 KiB and eight (the limit of 2048 threads) from n = 128 down.  A thread keeps one column: its reads of the
 * panel go to one bank group with its 15 neighbours at the next 15 words, whatever the distance d of the walk.
 */
#ifndef MGC_EDT_OPS_INL
#define MGC_EDT_OPS_INL

#include "mgc_edt.h"

struct MgcEdtWaveDev {
    __device__ __forceinline__ uint64_t seed_mask(const uint8_t* row, int side, int64_t x0, int64_t n, int lane) const
    {
        const int64_t x = x0 + lane;
        return (uint64_t)__ballot(x < n && ((row[x] != 0) == (side != 0)));
    }
};

struct MgcEdtBarrier {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

/* rows of n bytes, row r at plane + r * n; the loop bounds of mgc_edt_row_step are the same in every lane, so all 64 meet in each ballot */
template <int E>
__global__ __launch_bounds__(256) void k_edt_rows(const uint8_t* plane, int side, int64_t rows, int64_t n, double s, double* g)
{
    MgcEdtWaveDev wave;
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) mgc_edt_row_step(plane + r * n, side, n, s, g + r * n, lane, wave);
}

/* panel p: block p / ppo of n * stride entries, columns (p % ppo) * MGC_EDT_PANEL_COLS on; ppo = panels per block.  Dynamic LDS:
 * n * MGC_EDT_PANEL_COLS doubles (the host checks n <= MGC_EDT_PANEL_LINE). */
template <int E>
__global__ __launch_bounds__(256) void k_edt_panels(double* g, int64_t n, int64_t stride, int64_t npanels, int64_t ppo, double s)
{
    extern __shared__ double mgc_edt_panel[];
    MgcEdtBarrier barrier;
    for (int64_t p = blockIdx.x; p < npanels; p += gridDim.x) {
        const int64_t c0 = (p % ppo) * MGC_EDT_PANEL_COLS;
        const int64_t left = stride - c0;
        mgc_edt_panel_step<0>(g, (p / ppo) * n * stride + c0, stride, n, (int)(left < MGC_EDT_PANEL_COLS ? left : MGC_EDT_PANEL_COLS), s, mgc_edt_panel, (int)threadIdx.x, 256, barrier);
    }
}

template <int E>
__global__ __launch_bounds__(256) void k_edt_long(const double* src, double* dst, int64_t nvox, int64_t n, int64_t stride, double s)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) mgc_edt_long_voxel<0>(src, dst, v, n, stride, s);
}

template <int E>
__global__ __launch_bounds__(256) void k_edt_fill(double* g, int64_t nvox, double value)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) g[v] = value;
}

template <int E>
__global__ __launch_bounds__(256) void k_edt_border(const uint8_t* plane, int64_t dz, int64_t dy, int64_t dx, int ndim, int connectivity, uint8_t* out)
{
    const int64_t nvox = dz * dy * dx;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const int64_t x = v % dx, r = v / dx;
        out[v] = mgc_edt_is_border(plane, dz, dy, dx, ndim, connectivity, r / dy, r % dy, x) ? 1 : 0;
    }
}

/* one wave per segment.  cnt[s]: voxels of p in the segment; part[4 * s + k]: voxels of class k (mgc_edt_overlap_class; q may be NULL) */
template <int E>
__global__ __launch_bounds__(256) void k_edt_count(const uint8_t* p, const uint8_t* q, int64_t nvox, int64_t nseg, unsigned long long* cnt, unsigned long long* part)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        unsigned c[4] = {0u, 0u, 0u, 0u};
        for (int it = 0; it < MGC_EDT_COUNT_SEG / 64; ++it) {
            const int64_t v = s * MGC_EDT_COUNT_SEG + it * 64 + lane;
            if (v >= nvox) break;
            const int k = mgc_edt_overlap_class(p, q, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] += k == j ? 1u : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c[j] += (unsigned)__shfl_xor((int)c[j], d, 64);
        if (lane == 0) {
            cnt[s] = c[0] + c[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) part[4 * s + j] = c[j];
        }
    }
}

/* one workgroup: thread t takes segments t, t + 256, ...; then a tree: the same order whatever ran when */
template <int E>
__global__ __launch_bounds__(256) void k_edt_reduce(const unsigned long long* part, int64_t nseg, unsigned long long* out4)
{
    __shared__ unsigned long long s_sum[4][256];
    const int t = threadIdx.x;
    unsigned long long sum[4] = {0ull, 0ull, 0ull, 0ull};
    for (int64_t s = t; s < nseg; s += 256)
        for (int j = 0; j < 4; ++j) sum[j] += part[4 * s + j];
    for (int j = 0; j < 4; ++j) s_sum[j][t] = sum[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off)
            for (int j = 0; j < 4; ++j) s_sum[j][t] += s_sum[j][t + off];
        __syncthreads();
    }
    if (t < 4) out4[t] = s_sum[t][0];
}

/* one wave per segment; off[s]: voxels of p in the segments before s (off[nseg]: all).  out[rank] = g[v] for the voxels v of p in
 * ascending order, rank < cap. */
template <int E>
__global__ __launch_bounds__(256) void k_edt_gather(const uint8_t* p, const double* g, int64_t nvox, int64_t nseg, const unsigned long long* off, int64_t cap, double* out)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        if (off[s + 1] == off[s]) continue; /* (uniform over the wave) */
        int64_t at = (int64_t)off[s];
        for (int it = 0; it < MGC_EDT_COUNT_SEG / 64; ++it) {
            const int64_t v = s * MGC_EDT_COUNT_SEG + it * 64 + lane;
            const bool mine = v < nvox && p[v] != 0;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                const int64_t rank = at + __popcll(m & ((1ull << lane) - 1ull));
                if (rank < cap) out[rank] = g[v];
            }
            at += __popcll(m);
        }
    }
}

#endif /* MGC_EDT_OPS_INL */
