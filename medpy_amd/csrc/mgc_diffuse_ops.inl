/*
 * mgc_diffuse_ops.inl -- the kernels of mgc_diffuse_image / mgc_diffuse.  Included once, from mgc_diffuse_driver.inl.
 * The arithmetic is mgc_diffuse.h's; this file only decides who computes which flux.
 *
 * k_diffuse<OPT>: one launch advances the whole volume by one iteration.  A workgroup of 512 threads (8 waves) owns a brick of
 * MGC_AD_BZ x MGC_AD_BY x MGC_AD_BX = 8 x 8 x 64 voxels and loads it with a one-voxel halo into LDS as float32 (10 x 10 x 66 words,
 * 26.4 KB); the input is any dtype (first iteration) or float32, the output float32.  Lane = x, wave = y, and a thread walks its
 * column of the brick in z.  Every forward flux is evaluated once by the voxel at its low end and handed to the neighbour at its
 * high end, which needs it as its backward flux:
 *   z: kept in a register from one step of the walk to the next;
 *   x: one lane up (__shfl_up);
 *   y: through a plane of LDS per z (8 x 8 x 64 words, 16 KB), written by every wave before the walk starts.
 * The fluxes across the three low faces of the brick are recomputed from the halo (z: before the first step of the walk; y: by
 * wave 0; x: by lanes 0 .. 7 of a wave, one step of the walk each, and broadcast to lane 0 step by step): the same inputs through
 * the same lines give the same bits.  42.8 KB of LDS: three workgroups, 24 waves, per compute unit.
 * Rows of a float32 image whose length is a multiple of 4 are loaded as float4 where the brick is whole in x; every other row,
 * the halo columns and the stores move one word per lane, a wave a contiguous 256 bytes.
 */
#include "mgc_diffuse.h"

/* element i of an image of any dtype as float32, converted directly (no detour through double: one rounding) */
__device__ __forceinline__ float mgc_ad_load(const void* p, int dtype, int64_t i)
{
    switch (dtype) {
    case MGC_U8: return (float)((const uint8_t*)p)[i];
    case MGC_I8: return (float)((const int8_t*)p)[i];
    case MGC_U16: return (float)((const uint16_t*)p)[i];
    case MGC_I16: return (float)((const int16_t*)p)[i];
    case MGC_U32: return (float)((const uint32_t*)p)[i];
    case MGC_I32: return (float)((const int32_t*)p)[i];
    case MGC_U64: return (float)((const uint64_t*)p)[i];
    case MGC_I64: return (float)((const int64_t*)p)[i];
    case MGC_F32: return ((const float*)p)[i];
    default: return (float)((const double*)p)[i];
    }
}

#define MGC_AD_PX (MGC_AD_BX + 2)
#define MGC_AD_PY (MGC_AD_BY + 2)
#define MGC_AD_PZ (MGC_AD_BZ + 2)
#define MGC_AD_THREADS (MGC_AD_BX * MGC_AD_BY)

struct MgcAdDims {
    int64_t dz, dy, dx;
    int bz, by, bx; /* bricks along each axis */
};

template <int OPT>
__global__ __launch_bounds__(MGC_AD_THREADS) void k_diffuse(MgcAdDims D, MgcDiffuse P, const void* __restrict__ in, int dtype, int vec4, float* __restrict__ out)
{
    __shared__ float T[MGC_AD_PZ][MGC_AD_PY][MGC_AD_PX];
    __shared__ float PY[MGC_AD_BZ][MGC_AD_BY][MGC_AD_BX];
    const int tid = (int)threadIdx.x;
    const int tx = tid & (MGC_AD_BX - 1), ty = tid >> 6;
    int b = (int)blockIdx.x;
    const int64_t x0 = (int64_t)(b % D.bx) * MGC_AD_BX;
    b /= D.bx;
    const int64_t y0 = (int64_t)(b % D.by) * MGC_AD_BY;
    const int64_t z0 = (int64_t)(b / D.by) * MGC_AD_BZ;

    /* the brick and its halo: wave w takes rows w, w + 8, .. of the 10 x 10 rows; what lies outside the volume reads as 0 and is
       never used (the differences are guarded by the voxel's place in the volume, not by what the halo holds) */
    const bool whole_x = vec4 && x0 + MGC_AD_BX <= D.dx;
    for (int row = ty; row < MGC_AD_PZ * MGC_AD_PY; row += MGC_AD_BY) {
        const int lz = row / MGC_AD_PY, ly = row - lz * MGC_AD_PY;
        const int64_t gz = z0 - 1 + lz, gy = y0 - 1 + ly;
        const bool row_in = gz >= 0 && gz < D.dz && gy >= 0 && gy < D.dy;
        const int64_t base = row_in ? (gz * D.dy + gy) * D.dx : 0;
        float* const dst = &T[lz][ly][0];
        if (whole_x) {
            if (tx < MGC_AD_BX / 4) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (row_in) v = *(const float4*)((const float*)in + base + x0 + 4 * tx);
                dst[1 + 4 * tx] = v.x; dst[2 + 4 * tx] = v.y; dst[3 + 4 * tx] = v.z; dst[4 + 4 * tx] = v.w;
            } else if (tx < MGC_AD_BX / 4 + 2) {
                const int lx = tx == MGC_AD_BX / 4 ? 0 : MGC_AD_PX - 1;
                const int64_t gx = x0 - 1 + lx;
                dst[lx] = row_in && gx >= 0 && gx < D.dx ? ((const float*)in)[base + gx] : 0.0f;
            }
        } else {
            for (int lx = tx; lx < MGC_AD_PX; lx += MGC_AD_BX) {
                const int64_t gx = x0 - 1 + lx;
                dst[lx] = row_in && gx >= 0 && gx < D.dx ? mgc_ad_load(in, dtype, base + gx) : 0.0f;
            }
        }
    }
    __syncthreads();

    const int64_t gx = x0 + tx, gy = y0 + ty;
    const bool hi_x = gx < D.dx - 1, hi_y = gy < D.dy - 1;
    const bool lo_x = gx >= 1, lo_y = gy >= 1;
    const float sz = P.s[0], sy = P.s[1], sx = P.s[2];

    /* the y fluxes of the brick, each by the voxel at its low end */
#pragma unroll
    for (int z = 0; z < MGC_AD_BZ; ++z) {
        const float u = T[z + 1][ty + 1][tx + 1];
        PY[z][ty][tx] = mgc_ad_flux(mgc_ad_diff(u, T[z + 1][ty + 2][tx + 1], hi_y), sy, P.kappa, P.kappa_s, OPT);
    }
    __syncthreads();

    /* the walk in z; the flux across the low z face of the brick from the halo */
    float phi_z_lo = 0.0f;
    if (z0 >= 1) phi_z_lo = mgc_ad_flux(mgc_ad_diff(T[0][ty + 1][tx + 1], T[1][ty + 1][tx + 1], true), sz, P.kappa, P.kappa_s, OPT);
    /* the fluxes across the low x face of the brick, for the whole walk at once: lane z of a wave evaluates the one of step z (one
       evaluation per wave instead of one per step, which every lane of the wave would sit through) */
    float phi_x_face = 0.0f;
    if (tx < MGC_AD_BZ && x0 >= 1) phi_x_face = mgc_ad_flux(mgc_ad_diff(T[tx + 1][ty + 1][0], T[tx + 1][ty + 1][1], true), sx, P.kappa, P.kappa_s, OPT);
    const bool store_xy = gx < D.dx && gy < D.dy;
#pragma unroll
    for (int z = 0; z < MGC_AD_BZ; ++z) {
        const int64_t gz = z0 + z;
        const float u = T[z + 1][ty + 1][tx + 1];
        const float phi_z = mgc_ad_flux(mgc_ad_diff(u, T[z + 2][ty + 1][tx + 1], gz < D.dz - 1), sz, P.kappa, P.kappa_s, OPT);
        const float phi_x = mgc_ad_flux(mgc_ad_diff(u, T[z + 1][ty + 1][tx + 2], hi_x), sx, P.kappa, P.kappa_s, OPT);
        float phi_x_lo = __shfl_up(phi_x, 1); /* every lane of the wave is here: the loop bounds are the brick's, not the volume's */
        const float from_face = __shfl(phi_x_face, z);
        if (tx == 0) phi_x_lo = from_face;
        const float phi_y = PY[z][ty][tx];
        float phi_y_lo;
        if (ty > 0) phi_y_lo = PY[z][ty - 1][tx];
        else phi_y_lo = lo_y ? mgc_ad_flux(mgc_ad_diff(T[z + 1][0][tx + 1], u, true), sy, P.kappa, P.kappa_s, OPT) : 0.0f;
        const float mz = mgc_ad_div(phi_z, phi_z_lo, gz >= 1);
        const float my = mgc_ad_div(phi_y, phi_y_lo, lo_y);
        const float mx = mgc_ad_div(phi_x, phi_x_lo, lo_x);
        if (store_xy && gz < D.dz) out[(gz * D.dy + gy) * D.dx + gx] = mgc_ad_update(u, P.gamma, P.ndim, mz, my, mx);
        phi_z_lo = phi_z;
    }
}

/* niter = 0: the float32 copy */
template <int DUMMY>
__global__ __launch_bounds__(256) void k_diffuse_convert(int64_t n, const void* __restrict__ in, int dtype, float* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = mgc_ad_load(in, dtype, i);
}
