/*
 * mgc_tweight_ops.inl -- whole t-link weight arrays of a user-defined regional term (mgc_add_tweights, mgc_update_tweights) and
 * their edits by voxel list (mgc_edit_tweights); DESIGN 12.  The caller's source and sink weights are merged per voxel with
 * Graph::add_tweights (graph.h:416-425, the body mgc_add_tweights of mgc_kernels.hip) into a STORE that stays with the handle:
 * two f64 planes in C order, the merged explicit t-link -- the array k_build and k_update_tlinks read as tr_in -- and the voxel's
 * accumulated share of the flow constant.  Build-side streaming kernels over C-order planes, nothing tiled: plain loads and
 * stores, every slot has one writer, no floating-point atomics.  Included by mgc_kernels.hip behind mgc_add_tweights.
 *
 *   k_tw_check     both arrays must be finite; the first offender's index comes back
 *   k_tw_merge     source / sink arrays -> the two planes of the store, on top of what it holds or on top of zero
 *   k_tw_scatter   the entries of a list -> their slots of the store (REPLACE)
 *   k_tw_partials  the share plane's sums per segment, in a fixed order
 *
 * The flow constant of the store is k_sum_partials over the segment partials: a list edit sums only the segments it touched again
 * and then the partials, and gets bit for bit what the pass over the whole plane gives.
 */
#ifndef MGC_TWEIGHT_OPS_INL
#define MGC_TWEIGHT_OPS_INL

#include <float.h>

#include "mgc_tweight_edit.h"

#define MGC_TW_NONE (~0ull)

/* two neighbouring entries of an array, loaded and stored as one vector (the arrays and both planes start on 16-byte borders) */
template <class T>
struct alignas(2 * sizeof(T)) MgcTwPair {
    T a, b;
};

/* key = 2 * flat index + (0: source, 1: sink); the lowest bad key of a wave is found with shuffles when its ballot says there is
 * one, the waves of a workgroup meet in LDS, and one atomic min per workgroup reaches *first (the scheme of k_dense_check).
 * A thread takes the pair of entries (2 i, 2 i + 1); an odd array's last entry is read on its own. */
template <class T>
__global__ __launch_bounds__(256) void k_tw_check(int64_t n, const T* __restrict__ source, const T* __restrict__ sink, unsigned long long* first)
{
    __shared__ unsigned long long wave_min[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t npairs = (n + 1) / 2;
    unsigned long long best = MGC_TW_NONE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        double s[2] = {0.0, 0.0}, k[2] = {0.0, 0.0};
        if (2 * i + 1 < n) {
            const MgcTwPair<T> sp = ((const MgcTwPair<T>*)source)[i], kp = ((const MgcTwPair<T>*)sink)[i];
            s[0] = (double)sp.a; s[1] = (double)sp.b; k[0] = (double)kp.a; k[1] = (double)kp.b;
        } else {
            s[0] = (double)source[2 * i]; k[0] = (double)sink[2 * i];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned long long key = 2ull * (unsigned long long)(2 * i + j);
            if (!(fabs(s[j]) <= DBL_MAX) && key < best) best = key;
            if (!(fabs(k[j]) <= DBL_MAX) && key + 1ull < best) best = key + 1ull;
        }
    }
    if (__ballot(best != MGC_TW_NONE) != 0ull) {
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
        if (best != MGC_TW_NONE) atomicMin(first, best);
    }
}

/* One Graph::add_tweights per voxel: (tr, share) <- add_tweights(source[id], sink[id]) on top of what the store holds (fresh == 0:
 * mgc_add_tweights, calls accumulate in call order) or on top of a zero t-link and a zero share (fresh != 0: mgc_update_tweights,
 * what a cleared store and one call leave).  changed (or NULL): += voxels whose t-link is not bit for bit what it was. */
template <class T>
__global__ __launch_bounds__(256) void k_tw_merge(int64_t n, const T* __restrict__ source, const T* __restrict__ sink, double* __restrict__ tr_plane,
                                                 double* __restrict__ share_plane, int fresh, unsigned long long* changed)
{
    const int64_t npairs = (n + 1) / 2;
    unsigned c = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        const bool two = 2 * i + 1 < n;
        double s[2] = {0.0, 0.0}, k[2] = {0.0, 0.0}, tr[2] = {0.0, 0.0}, fc[2] = {0.0, 0.0}, old[2];
        if (two) {
            const MgcTwPair<T> sp = ((const MgcTwPair<T>*)source)[i], kp = ((const MgcTwPair<T>*)sink)[i];
            const MgcTwPair<double> tp = ((const MgcTwPair<double>*)tr_plane)[i];
            s[0] = (double)sp.a; s[1] = (double)sp.b; k[0] = (double)kp.a; k[1] = (double)kp.b;
            old[0] = tp.a; old[1] = tp.b;
            if (!fresh) {
                const MgcTwPair<double> fp = ((const MgcTwPair<double>*)share_plane)[i];
                fc[0] = fp.a; fc[1] = fp.b;
            }
        } else {
            s[0] = (double)source[2 * i]; k[0] = (double)sink[2 * i];
            old[0] = old[1] = tr_plane[2 * i];
            if (!fresh) fc[0] = share_plane[2 * i];
        }
        if (!fresh) { tr[0] = old[0]; tr[1] = old[1]; }
        mgc_add_tweights(tr[0], fc[0], s[0], k[0]);
        if (two) mgc_add_tweights(tr[1], fc[1], s[1], k[1]);
        else tr[1] = old[1];
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

/* one thread per entry; the host has checked the ids (in range, none twice: mgc_tweight_edit.h): no two threads write one slot.
 * REPLACE: the slot gets what one add_tweights(source[k], sink[k]) leaves on a zero t-link and a zero share. */
__global__ __launch_bounds__(256) void k_tw_scatter(int64_t n, int64_t nvox, const int64_t* __restrict__ ids, const double* __restrict__ source,
                                                   const double* __restrict__ sink, double* __restrict__ tr_plane, double* __restrict__ share_plane,
                                                   unsigned long long* changed)
{
    unsigned c = 0u;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[k];
        if (id < 0 || id >= nvox) continue;
        double tr = 0.0, fc = 0.0;
        mgc_add_tweights(tr, fc, source[k], sink[k]);
        c += mgc_same_bits(tr, tr_plane[id]) ? 0u : 1u;
        tr_plane[id] = tr;
        share_plane[id] = fc;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

/* part[s] = sum of the share plane over segment s = [s * MGC_TW_SEG, (s + 1) * MGC_TW_SEG) of the volume, one wave per segment:
 * lane l adds its entries l, l + 64, ... in ascending order, then the lanes meet in a butterfly -- one order of additions per
 * segment, whichever launch asks.  segs == NULL: the segments 0 .. nsegs - 1; else the nsegs segments segs names. */
__global__ __launch_bounds__(256) void k_tw_partials(const double* __restrict__ share_plane, int64_t nvox, int64_t nsegs, const int64_t* __restrict__ segs,
                                                    double* __restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t all = (nvox + MGC_TW_SEG - 1) / MGC_TW_SEG;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nsegs; w += (int64_t)gridDim.x * 4) {
        const int64_t s = segs ? segs[w] : w;
        if (s < 0 || s >= all) continue; /* (uniform over the wave) */
        const int64_t lo = s * MGC_TW_SEG;
        double v = 0.0;
#pragma unroll 8
        for (int it = 0; it < MGC_TW_SEG / 64; ++it) {
            const int64_t id = lo + (int64_t)it * 64 + lane;
            if (id < nvox) v = v + share_plane[id];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
        if (lane == 0) part[s] = v;
    }
}

#endif /* MGC_TWEIGHT_OPS_INL */
