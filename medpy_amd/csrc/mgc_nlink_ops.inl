/*
 * mgc_nlink_ops.inl -- warm update of the boundary term (mgc_update_boundary; DESIGN 10, "The boundary term"): the n-link side of
 * dynamic graph cuts next to k_update_tlinks.  The capacities as built are a pure function of the resident image
 * (mgc_built_capacity), so a change of the term, of sigma, of the spacing or of the image itself is folded into the residual graph
 * by evaluating every arc's capacity under the OLD and under the NEW arguments in registers: no copy of the built capacities is
 * kept.  Included by mgc_kernels.hip behind MgcBuildArgs and k_update_tlinks.
 */
#ifndef MGC_NLINK_OPS_INL
#define MGC_NLINK_OPS_INL

#include "mgc_nlink_fold.h"

/* what mgc_get_boundary_update_info reports */
struct MgcFoldCounts {
    unsigned long long arcs_changed;   /* arcs whose capacity changed */
    unsigned long long arcs_clamped;   /* ... whose flow no longer fitted */
    unsigned long long voxels_changed; /* voxels whose excess or residual sink link changed */
    unsigned long long tiles_flagged;  /* tiles that gained a t-link flag */
};

__device__ __forceinline__ bool mgc_term_takes_abs(int term)
{
    return term == MGC_TERM_MAXIMUM_LINEAR || term == MGC_TERM_MAXIMUM_EXPONENTIAL || term == MGC_TERM_MAXIMUM_POWER;
}

/* the 10 x 10 x 10 block of a tile (the tile and a one-voxel halo) as k_build stages it: 0 outside the volume */
__device__ __forceinline__ void mgc_fold_stage(const MgcLattice& L, const MgcBuildArgs& A, int64_t z0, int64_t y0, int64_t x0, int t, double* img)
{
    const bool take_abs = mgc_term_takes_abs(A.term);
    for (int k = t; k < 1000; k += MGC_TV) {
        const int64_t gz = z0 + k / 100 - 1, gy = y0 + (k / 10) % 10 - 1, gx = x0 + k % 10 - 1;
        double v = 0.0;
        if (gz >= 0 && gz < L.dz && gy >= 0 && gy < L.dy && gx >= 0 && gx < L.dx)
            v = mgc_load_as_double(A.image, A.img_dtype, (gz * L.dy + gy) * L.dx + gx, take_abs);
        img[k] = v;
    }
}

/* weight of the pair (lower voxel img[lo], upper voxel img[hi]) as mgc_built_capacity evaluates it; div = the spacing's divisor */
template <bool TABLE>
__device__ __forceinline__ double mgc_fold_weight(const MgcBuildArgs& A, const double* img, int lo, int hi, double div)
{
    double w = mgc_boundary_g(A.term, img[lo], img[hi], A.p0, TABLE ? A.lut : nullptr, TABLE ? A.lut_n : 0);
    if (A.has_spacing) w = w / div;
    return w;
}

/* A0: the arguments the graph was built (or last updated) with, A1: the new ones; both describe resident images of the handle's
 * shape and a built-in term.  Every voxel applies mgc_nlink_fold to the arcs that leave it, from its own residual, and takes what no
 * longer fits back into its signed excess x = excess - sink, split as k_update_tlinks splits it.  A kernel instance writes only the
 * state of its own voxels: one launch, no order between tiles.  Each pair's two weights are evaluated once per tile and shared
 * through LDS (6-neighbourhood: the three planes of forward weights of k_build; full neighbourhood: pair by pair, the lower voxel's
 * weight handed to the upper one).  Flags, status words, stamps and the count of sink tiles as k_update_tlinks leaves them; the
 * t-links themselves (tr0, the flow constant) do not change.
 * TABLE: one of the two terms is evaluated by table. */
template <bool FULL, bool TABLE>
__global__ __launch_bounds__(MGC_TV) void k_update_nlinks(MgcLattice L, MgcBuildArgs A0, MgcBuildArgs A1, MgcFoldCounts* counts)
{
    __shared__ double img0[1000], img1[1000];
    __shared__ double wsh[FULL ? 4 * MGC_TV : 6 * 576]; /* 6: [old / new][axis][c][u][v] as k_build's wf; 26: [pair parity][old / new][512] */
    __shared__ int vote;
    const int t = threadIdx.x;
    const int lz = t >> 6, ly = (t >> 3) & 7, lx = t & 7;
    const int me = mgc_hs_index(lz, ly, lx);
    /* one block serves both argument sets when they read the same image the same way (uniform) */
    const bool one_image = A0.image == A1.image && A0.img_dtype == A1.img_dtype && mgc_term_takes_abs(A0.term) == mgc_term_takes_abs(A1.term);
    const double* const imgN = one_image ? img0 : img1;
    int flagged_sink = 0; /* (thread 0) tiles with tflags bit 1 */
    unsigned n_changed = 0, n_clamped = 0, n_voxels = 0, n_flagged = 0;
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        const int64_t z0 = (int64_t)tz * 8, y0 = (int64_t)ty * 8, x0 = (int64_t)tx * 8;
        const int64_t gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
        const bool valid = gz < L.dz && gy < L.dy && gx < L.dx;
        const int64_t v = (int64_t)tile * MGC_TV + t;
        if (t == 0) vote = 0;
        mgc_fold_stage(L, A0, z0, y0, x0, t, img0);
        if (!one_image) mgc_fold_stage(L, A1, z0, y0, x0, t, img1);
        __syncthreads();
        /* the voxel's state; the planes tr0 and sink are read under the flags (k_update_tlinks, "FLAGS") */
        const uint32_t st = L.status[tile];
        const uint32_t tf_old = A0.tflags[tile];
        const bool tr0_ok = FULL || tf_old != 0u, sink_ok = FULL || (st & MGC_ST_SINK) != 0u;
        const double tr = tr0_ok ? A0.tr0[v] : 0.0;
        const double sk_old = sink_ok ? L.sink[v] : 0.0;
        const double e_old = L.excess[v];
        double x = e_old - sk_old;
        bool gave = false, touched = false;
        uint32_t m = 0;
        if (FULL) m = L.rmask32[v];
        else m = L.rmask[v];
        auto fold_arc = [&](int d, double c, double c1) __attribute__((always_inline)) {
            if (mgc_same_bits(c, c1)) return;
            const int64_t o = ((int64_t)tile * (FULL ? MGC26_NDIR : MGC_NDIR) + d) * MGC_TV + t;
            double r = L.rcap[o];
            bool clamped;
            const double back = mgc_nlink_fold(c, c1, &r, &clamped);
            MGC_STORE_STREAM(&L.rcap[o], r);
            m = (m & ~(1u << d)) | (r > 0.0 ? 1u << d : 0u); /* (NaN is not residual) */
            if (back != 0.0) { x += back; gave = true; }
            touched = true;
            n_changed++;
            n_clamped += clamped ? 1u : 0u;
        };
        if constexpr (!FULL) {
            /* every pair's weights once, by its lower voxel, and the pairs that enter through the lower faces: k_build's hand-over */
            auto pair = [&](const MgcBuildArgs& A, const double* img, int axis, int lo, bool ok) -> double {
                if (!ok) return 0.0;
                return mgc_fold_weight<TABLE>(A, img, lo, lo + (axis == 0 ? 1 : (axis == 1 ? 10 : 100)), A.inv_axis[axis]);
            };
            double* const wf0 = wsh;
            double* const wf1 = wsh + 3 * 576;
            const bool okx = valid && gx + 1 < L.dx, oky = valid && gy + 1 < L.dy, okz = valid && gz + 1 < L.dz;
            wf0[0 * 576 + (lx + 1) * 64 + lz * 8 + ly] = pair(A0, img0, 0, me, okx);
            wf1[0 * 576 + (lx + 1) * 64 + lz * 8 + ly] = pair(A1, imgN, 0, me, okx);
            wf0[1 * 576 + (ly + 1) * 64 + lz * 8 + lx] = pair(A0, img0, 1, me, oky);
            wf1[1 * 576 + (ly + 1) * 64 + lz * 8 + lx] = pair(A1, imgN, 1, me, oky);
            wf0[2 * 576 + (lz + 1) * 64 + ly * 8 + lx] = pair(A0, img0, 2, me, okz);
            wf1[2 * 576 + (lz + 1) * 64 + ly * 8 + lx] = pair(A1, imgN, 2, me, okz);
            if (t < 192) {
                const int axis = t >> 6, u = (t >> 3) & 7, w = t & 7;
                const int lo = axis == 0 ? mgc_hs_index(u, w, -1) : (axis == 1 ? mgc_hs_index(u, -1, w) : mgc_hs_index(-1, u, w));
                const bool ok = axis == 0 ? (x0 > 0 && z0 + u < L.dz && y0 + w < L.dy)
                                          : (axis == 1 ? (y0 > 0 && z0 + u < L.dz && x0 + w < L.dx) : (z0 > 0 && y0 + u < L.dy && x0 + w < L.dx));
                wf0[axis * 576 + u * 8 + w] = pair(A0, img0, axis, lo, ok);
                wf1[axis * 576 + u * 8 + w] = pair(A1, imgN, axis, lo, ok);
            }
            __syncthreads();
            if (valid) {
#pragma unroll
                for (int d = 0; d < MGC_NDIR; ++d) {
                    const int c = ((d >> 1) == 0 ? lx : ((d >> 1) == 1 ? ly : lz)) + (d & 1);
                    const int uv = (d >> 1) == 0 ? lz * 8 + ly : ((d >> 1) == 1 ? lz * 8 + lx : ly * 8 + lx);
                    fold_arc(d, wf0[(d >> 1) * 576 + c * 64 + uv], wf1[(d >> 1) * 576 + c * 64 + uv]);
                }
            }
        } else {
            /* pair i: direction dA = i points to the LOWER voxel of the pair, dB = 25 - i to the upper one.  Every voxel evaluates the
             * weight of its dB arc -- it is the lower voxel there -- and leaves it for the voxel above, whose dA arc it is; a voxel
             * whose lower neighbour lies in another tile evaluates that pair itself.  Two buffers: one barrier per pair. */
            for (int i = 0; i < 13; ++i) {
                const int dA = i, dB = 25 - i;
                int oz, oy, ox;
                mgc26_offset(dA, oz, oy, ox);
                const int step = oz * 100 + oy * 10 + ox; /* in the staged blocks, towards the lower voxel */
                double* const buf0 = wsh + (i & 1) * 2 * MGC_TV;
                double* const buf1 = buf0 + MGC_TV;
                const bool hasB = valid && gz - oz >= 0 && gz - oz < L.dz && gy - oy >= 0 && gy - oy < L.dy && gx - ox >= 0 && gx - ox < L.dx;
                const bool hasA = valid && gz + oz >= 0 && gz + oz < L.dz && gy + oy >= 0 && gy + oy < L.dy && gx + ox >= 0 && gx + ox < L.dx;
                const double cB0 = hasB ? mgc_fold_weight<TABLE>(A0, img0, me, me - step, A0.div26[dB]) : 0.0;
                const double cB1 = hasB ? mgc_fold_weight<TABLE>(A1, imgN, me, me - step, A1.div26[dB]) : 0.0;
                buf0[t] = cB0;
                buf1[t] = cB1;
                __syncthreads();
                const int za = lz + oz, ya = ly + oy, xa = lx + ox;
                double cA0 = 0.0, cA1 = 0.0;
                if (za >= 0 && za < 8 && ya >= 0 && ya < 8 && xa >= 0 && xa < 8) {
                    const int ta = t + oz * 64 + oy * 8 + ox;
                    cA0 = buf0[ta];
                    cA1 = buf1[ta];
                } else if (hasA) {
                    cA0 = mgc_fold_weight<TABLE>(A0, img0, me + step, me, A0.div26[dA]);
                    cA1 = mgc_fold_weight<TABLE>(A1, imgN, me + step, me, A1.div26[dA]);
                }
                if (valid) {
                    fold_arc(dA, cA0, cA1);
                    fold_arc(dB, cB0, cB1);
                }
            }
        }
        double e = e_old, sk = sk_old;
        if (gave) {
            e = x > 0.0 ? x : 0.0;
            sk = x < 0.0 ? -x : 0.0;
        }
        /* (6-neighbourhood: the barrier behind the weights separates the reset of the vote word from the votes; full neighbourhood: the pairs' barriers) */
        const int bits = (__ballot(tr > 0.0) ? 1 : 0) | (__ballot(tr < 0.0 || sk > 0.0) ? 2 : 0) | (__ballot(e > 0.0) ? 4 : 0) | (__ballot(sk > 0.0) ? 8 : 0);
        if ((t & 63) == 0 && bits) atomicOr(&vote, bits);
        __syncthreads();
        const int tb = vote;
        const uint32_t tf_new = (uint32_t)tb & 3u;
        if (!FULL) {
            if (tf_new != 0u && !tr0_ok) A0.tr0[v] = tr; /* (a tile that gains a flag: both planes in full) */
            if ((tf_new & 2u) && (!sink_ok || sk != sk_old)) L.sink[v] = sk;
        } else if (sk != sk_old) {
            L.sink[v] = sk;
        }
        if (e != e_old) MGC_STORE_STREAM(&L.excess[v], e);
        if (touched || (sk > 0.0) != (sk_old > 0.0)) {
            if (FULL) L.rmask32[v] = (m & ~MGC26_MASK_SINK) | (sk > 0.0 ? MGC26_MASK_SINK : 0u);
            else L.rmask[v] = (uint8_t)((m & ~(uint32_t)MGC_MASK_SINK) | (sk > 0.0 ? MGC_MASK_SINK : 0));
        }
        n_voxels += (e != e_old || sk != sk_old) ? 1u : 0u;
        if (t == 0) {
            L.status[tile] = ((tb & 8) ? MGC_ST_SINK : 0u) | ((tb & 4) ? MGC_ST_EXCESS : 0u) | ((!FULL && (tb & 1)) ? MGC_ST_SOURCE : 0u);
            A0.tflags[tile] = (uint8_t)tf_new;
            L.stamp[tile] = 0;
            L.rstamp[tile] = 0;
            flagged_sink += (tf_new & 2u) ? 1 : 0;
            n_flagged += (tf_new & ~tf_old) ? 1u : 0u;
        }
        __syncthreads(); /* everybody has read the vote word, the blocks and the weights before the next tile overwrites them */
    }
    if (!FULL && t == 0 && flagged_sink) atomicAdd(&L.count[MGC_CNT_SINK_TILES], flagged_sink);
    /* the counters: summed over the wave, one atomic per wave and counter */
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_changed += (unsigned)__shfl_xor((int)n_changed, d, 64);
        n_clamped += (unsigned)__shfl_xor((int)n_clamped, d, 64);
        n_voxels += (unsigned)__shfl_xor((int)n_voxels, d, 64);
    }
    if ((t & 63) == 0) {
        if (n_changed) atomicAdd(&counts->arcs_changed, (unsigned long long)n_changed);
        if (n_clamped) atomicAdd(&counts->arcs_clamped, (unsigned long long)n_clamped);
        if (n_voxels) atomicAdd(&counts->voxels_changed, (unsigned long long)n_voxels);
        if (t == 0 && n_flagged) atomicAdd(&counts->tiles_flagged, (unsigned long long)n_flagged);
    }
}

#endif /* MGC_NLINK_OPS_INL */
