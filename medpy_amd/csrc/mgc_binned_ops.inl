/*
 * mgc_binned_ops.inl -- the kernels of the binned regional term: the histograms of a feature image under the two
 * marker planes, and the expansion of two small tables over the image into the t-link store of mgc_tweight_ops.inl.  The rule of
 * the bin is mgc_binned.h's.  Build-side streaming kernels over C-order planes, nothing tiled; integer atomics only (counts do not
 * depend on their order), no floating-point atomics, every slot of the store has one writer.  Included by mgc_binned_driver.inl
 * at the very end of the library's one translation unit, behind every other kernel.
 *
 *   k_binned_check   a float feature image must be finite; the first offender's flat index comes back
 *   k_marker_hist    counts per bin of the voxels under the fg plane and under the bg plane
 *   k_tw_binned      (image, tables) -> the two planes of the store, on top of what it holds or on top of zero
 */
#ifndef MGC_BINNED_OPS_INL
#define MGC_BINNED_OPS_INL

#include <float.h>

#include "mgc_binned.h"

#define MGC_BINNED_NONE (~0ull)

/* the lowest flat index of a value that is not finite: shuffles in a wave whose ballot is not empty, LDS across the four waves,
 * one atomic min per workgroup (the scheme of k_tw_check).  A thread takes the pair (2 i, 2 i + 1); an odd volume's last entry is
 * read on its own.  T: float or double. */
template <class T>
__global__ __launch_bounds__(256) void k_binned_check(int64_t n, const T* __restrict__ image, unsigned long long* first)
{
    __shared__ unsigned long long wave_min[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t npairs = (n + 1) / 2;
    unsigned long long best = MGC_BINNED_NONE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        double v[2] = {0.0, 0.0};
        if (2 * i + 1 < n) {
            const MgcTwPair<T> p = ((const MgcTwPair<T>*)image)[i];
            v[0] = (double)p.a; v[1] = (double)p.b;
        } else {
            v[0] = (double)image[2 * i];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned long long key = (unsigned long long)(2 * i + j);
            if (!(fabs(v[j]) <= DBL_MAX) && key < best) best = key;
        }
    }
    if (__ballot(best != MGC_BINNED_NONE) != 0ull) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d);
            if (o < best) best = o;
        }
    }
    if (lane == 0) wave_min[wv] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (wave_min[w] < best) best = wave_min[w];
        if (best != MGC_BINNED_NONE) atomicMin(first, best);
    }
}

/* hist[bin(p)] += 1 for every voxel p under the fg plane, hist[nbins + bin(p)] += 1 for every voxel under the bg plane (a voxel
 * under both counts in both; a plane that is NULL counts nothing).  A thread takes 16 neighbouring voxels: one 16-byte load per
 * plane, and the image is read only where a marker byte is set -- strokes are a small fraction of the volume, so the pass moves
 * about 2 bytes per voxel.  LDS: the counts of a workgroup go into its own histogram in LDS (32-bit adds there; a workgroup sees
 * far fewer than 2^32 voxels) and the bins that are not zero are flushed with 64-bit integer adds; else (more than
 * MGC_BINNED_LDS_MAX bins) every count is a 64-bit integer add in device memory.  The voxels behind the last whole group of 16 --
 * all of them in a volume of fewer than 16 -- are taken one per thread by the first threads of the grid.
 *   out4 += {counts under fg, counts under bg, counts the clamp raised into bin 0 (value below lo), counts the clamp lowered into
 * the last bin (value at or above lo + nbins * width)}.  is_float: a marked value that is not finite is not counted; the lowest
 * flat index of such a value reaches *first. */
template <bool LDS>
__global__ __launch_bounds__(256) void k_marker_hist(int64_t n, const uint8_t* __restrict__ fg, const uint8_t* __restrict__ bg, const void* __restrict__ image,
                                                    int dtype, int is_float, int64_t nbins, double lo, double width, unsigned long long* hist,
                                                    unsigned long long* out4, unsigned long long* first)
{
    __shared__ unsigned int lh[LDS ? 2 * MGC_BINNED_LDS_MAX : 1];
    if (LDS) {
        for (int b = threadIdx.x; b < 2 * (int)nbins; b += 256) lh[b] = 0u;
        __syncthreads();
    }
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    unsigned long long bad = MGC_BINNED_NONE;
    const double top = (double)(nbins - 1);
    auto count = [&](int64_t id, bool mf, bool mb) {
        const double v = mgc_load_as_double(image, dtype, id, false);
        if (is_float && !(fabs(v) <= DBL_MAX)) {
            if ((unsigned long long)id < bad) bad = (unsigned long long)id;
            return;
        }
        const double f = mgc_binned_floor(v, lo, width);
        const int64_t b = mgc_binned_clamp(f, nbins);
        const unsigned both = (mf ? 1u : 0u) + (mb ? 1u : 0u);
        cnt[0] += mf ? 1u : 0u;
        cnt[1] += mb ? 1u : 0u;
        cnt[2] += f < 0.0 ? both : 0u;
        cnt[3] += f > top ? both : 0u;
        if (LDS) {
            if (mf) atomicAdd(&lh[b], 1u);
            if (mb) atomicAdd(&lh[nbins + b], 1u);
        } else {
            if (mf) atomicAdd(&hist[b], 1ull);
            if (mb) atomicAdd(&hist[nbins + b], 1ull);
        }
    };
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = n / 16;
    for (int64_t g = gid; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        const uint4 f4 = fg ? ((const uint4*)fg)[g] : zero;
        const uint4 b4 = bg ? ((const uint4*)bg)[g] : zero;
        if (!(f4.x | f4.y | f4.z | f4.w | b4.x | b4.y | b4.z | b4.w)) continue;
        const unsigned fw[4] = {f4.x, f4.y, f4.z, f4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (!(fw[w] | bw[w])) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool mf = ((fw[w] >> (8 * k)) & 0xffu) != 0u, mb = ((bw[w] >> (8 * k)) & 0xffu) != 0u;
                if (mf || mb) count(g * 16 + w * 4 + k, mf, mb);
            }
        }
    }
    {
        const int64_t id = groups * 16 + gid;
        if (id < n) {
            const bool mf = fg && fg[id] != 0, mb = bg && bg[id] != 0;
            if (mf || mb) count(id, mf, mb);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < 2 * (int)nbins; b += 256) {
            const unsigned c = lh[b];
            if (c) atomicAdd(&hist[b], (unsigned long long)c);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned c = cnt[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&out4[j], (unsigned long long)c);
    }
    if (bad != MGC_BINNED_NONE) atomicMin(first, bad);
}

/* k_tw_merge with the two array loads replaced by one image load, the bin and two table reads: voxel p gets one
 * Graph::add_tweights(source_table[bin(p)], sink_table[bin(p)]) on top of what the store holds (FRESH false:
 * mgc_add_tweights_binned) or on top of a zero t-link and a zero share (FRESH true: mgc_update_tweights_binned).  A thread takes
 * two neighbouring voxels -- one load of 2 * sizeof(T) bytes from the image, one 16-byte load and store per plane of the store; the
 * last entry of an odd volume on its own.  The tables (at most 65536 entries each) are read through the caches.  changed (or NULL):
 * += voxels whose t-link is not bit for bit what it was. */
template <class T, bool FRESH>
__global__ __launch_bounds__(256) void k_tw_binned(int64_t n, const T* __restrict__ image, int64_t nbins, double lo, double width,
                                                  const double* __restrict__ source_table, const double* __restrict__ sink_table, double* __restrict__ tr_plane,
                                                  double* __restrict__ share_plane, unsigned long long* changed)
{
    const int64_t npairs = (n + 1) / 2;
    unsigned c = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        const bool two = 2 * i + 1 < n;
        double v[2] = {0.0, 0.0}, tr[2] = {0.0, 0.0}, fc[2] = {0.0, 0.0}, old[2];
        if (two) {
            const MgcTwPair<T> ip = ((const MgcTwPair<T>*)image)[i];
            const MgcTwPair<double> tp = ((const MgcTwPair<double>*)tr_plane)[i];
            v[0] = (double)ip.a; v[1] = (double)ip.b;
            old[0] = tp.a; old[1] = tp.b;
            if (!FRESH) {
                const MgcTwPair<double> fp = ((const MgcTwPair<double>*)share_plane)[i];
                fc[0] = fp.a; fc[1] = fp.b;
            }
        } else {
            v[0] = (double)image[2 * i];
            old[0] = old[1] = tr_plane[2 * i];
            if (!FRESH) fc[0] = share_plane[2 * i];
        }
        if (!FRESH) { tr[0] = old[0]; tr[1] = old[1]; }
        const int64_t b0 = mgc_binned_bin(v[0], lo, width, nbins);
        mgc_add_tweights(tr[0], fc[0], source_table[b0], sink_table[b0]);
        if (two) {
            const int64_t b1 = mgc_binned_bin(v[1], lo, width, nbins);
            mgc_add_tweights(tr[1], fc[1], source_table[b1], sink_table[b1]);
        } else {
            tr[1] = old[1];
        }
        c += (mgc_same_bits(tr[0], old[0]) ? 0u : 1u) + (mgc_same_bits(tr[1], old[1]) ? 0u : 1u);
        if (two) {
            MgcTwPair<double> tp, fp;
            tp.a = tr[0]; tp.b = tr[1]; fp.a = fc[0]; fp.b = fc[1];
            ((MgcTwPair<double>*)tr_plane)[i] = tp;
            ((MgcTwPair<double>*)share_plane)[i] = fp;
        } else {
            tr_plane[2 * i] = tr[0];
            share_plane[2 * i] = fc[0];
        }
    }
    if (changed) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
    }
}

#endif /* MGC_BINNED_OPS_INL */
