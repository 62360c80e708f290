/*
 * mgc_label_hist_ops.inl -- the kernel of mgc_label_histograms: the histograms of the feature image over EVERY voxel,
 * split by one C-order label plane.  The rule of the bin is mgc_binned.h's, the run merging mgc_label_hist.h's.  A streaming kernel
 * over C-order planes, nothing tiled; integer atomics only (counts do not depend on their order), no floating-point atomics.
 * Included by mgc_label_hist_driver.inl at the very end of the library's one translation unit, behind every other kernel.
 *
 *   k_label_hist     one pass over (labels, image): fg counts where the label is not zero, bg counts where it is
 */
#ifndef MGC_LABEL_HIST_OPS_INL
#define MGC_LABEL_HIST_OPS_INL

#include <float.h>

#include <type_traits>

#include "mgc_binned.h"
#include "mgc_label_hist.h"

/* 16 bytes of an image of T, loaded as one vector (the image starts on a 16-byte border, a group on a multiple of 16 entries) */
template <class T>
struct alignas(16) MgcLhVec {
    T v[16 / sizeof(T)];
};

/* hist[bin(p)] += 1 for every voxel p with labels[p] != 0, hist[nbins + bin(p)] += 1 for every other voxel.  A thread takes groups
 * of MGC_LH_GROUP neighbouring voxels: one 16-byte load of the label plane and sizeof(T) 16-byte loads of the image, typed -- every
 * voxel counts here, so nothing is skipped and nothing goes through a run-time dtype switch.  The 16 (label, bin) keys of a group
 * are merged into runs (mgc_label_hist_runs) and every run is ONE add of its length: on a volume whose neighbours share label and
 * bin (the air of a CT volume) a group is one add, not sixteen on one address.  LDS: the adds go to the workgroup's own 2 * nbins
 * 32-bit counters in LDS (dynamic: 8 * nbins bytes; a workgroup sees far fewer than 2^32 voxels) and the counters that are not zero
 * are flushed with 64-bit integer adds; else (more than MGC_BINNED_LDS_MAX bins) every run is a 64-bit integer add in device
 * memory.  Groups beyond one trip of the grid are taken by a grid-stride loop.  The voxels behind the last whole group -- all of
 * them in a volume of fewer than 16 -- form one short group, read entry by entry by the first thread of the grid.
 *   out4 += {voxels with a label, voxels without, counts the clamp raised into bin 0 (value below lo), counts the clamp lowered
 * into the last bin (value at or above lo + nbins * width)}.  T float or double: the lowest flat index of a value that is not finite
 * reaches *first (the caller then drops the counts). */
template <class T, bool LDS>
__global__ __launch_bounds__(256) void k_label_hist(int64_t n, const uint8_t* __restrict__ labels, const T* __restrict__ image, int64_t nbins, double lo,
                                                   double width, unsigned long long* hist, unsigned long long* out4, unsigned long long* first)
{
    extern __shared__ unsigned int mgc_lh_counts[];
    constexpr int PER = 16 / (int)sizeof(T); /* entries of one vector */
    constexpr bool IS_FLOAT = std::is_floating_point<T>::value;
    if (LDS) {
        for (int b = threadIdx.x; b < 2 * (int)nbins; b += 256) mgc_lh_counts[b] = 0u;
        __syncthreads();
    }
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    unsigned long long bad = MGC_BINNED_NONE;
    const double top = (double)(nbins - 1);
    auto key_of = [&](double v, bool fg, int64_t id) -> uint32_t {
        if (IS_FLOAT && !(fabs(v) <= DBL_MAX) && (unsigned long long)id < bad) bad = (unsigned long long)id;
        const double f = mgc_binned_floor(v, lo, width);
        cnt[0] += fg ? 1u : 0u;
        cnt[1] += fg ? 0u : 1u;
        cnt[2] += f < 0.0 ? 1u : 0u;
        cnt[3] += f > top ? 1u : 0u;
        return mgc_label_hist_key(fg, mgc_binned_clamp(f, nbins), nbins);
    };
    auto add = [&](uint32_t key, uint32_t run) {
        if (LDS) atomicAdd(&mgc_lh_counts[key], run);
        else atomicAdd(&hist[key], (unsigned long long)run);
    };
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = n / MGC_LH_GROUP;
    for (int64_t g = gid; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const uint4 l4 = ((const uint4*)labels)[g];
        MgcLhVec<T> vec[sizeof(T)];
#pragma unroll
        for (int j = 0; j < (int)sizeof(T); ++j) vec[j] = ((const MgcLhVec<T>*)image)[g * (int64_t)sizeof(T) + j];
        const unsigned lw[4] = {l4.x, l4.y, l4.z, l4.w};
        uint32_t key[MGC_LH_GROUP];
#pragma unroll
        for (int i = 0; i < MGC_LH_GROUP; ++i)
            key[i] = key_of((double)vec[i / PER].v[i % PER], ((lw[i >> 2] >> (8 * (i & 3))) & 0xffu) != 0u, g * MGC_LH_GROUP + i);
        mgc_label_hist_runs(key, MGC_LH_GROUP, add);
    }
    const int tail = (int)(n - groups * MGC_LH_GROUP);
    if (gid == 0 && tail) {
        const int64_t base = groups * MGC_LH_GROUP;
        uint32_t key[MGC_LH_GROUP];
#pragma unroll
        for (int i = 0; i < MGC_LH_GROUP; ++i) key[i] = i < tail ? key_of((double)image[base + i], labels[base + i] != 0, base + i) : 0u;
        mgc_label_hist_runs(key, tail, add);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < 2 * (int)nbins; b += 256) {
            const unsigned c = mgc_lh_counts[b];
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
    if (IS_FLOAT && bad != MGC_BINNED_NONE) atomicMin(first, bad);
}

#endif /* MGC_LABEL_HIST_OPS_INL */
