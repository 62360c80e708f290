/*
 * mgc_geo_ops.inl -- the kernels of mgc_geodesic_distance and of the geodesic regional term.  The steps themselves are
 * mgc_geo.h; here they get their workgroups and the agent-scope atomics of the work lists:
 *
 *   k_geo_init      a thread per voxel: mgc_geo_init_voxel, and the count of the seeds
 *   k_geo_tile      one workgroup of 512 threads per ACTIVE tile: mgc_geo_tile_step
 *   k_geo_finite    the voxels with a finite distance
 *   k_tw_geodesic   (D_F, D_B, lam) -> the two planes of the t-link store, on top of what it holds or on top of zero
 *
 * Every kernel here is a template, the plain ones over a parameter GEO that nothing reads (instantiated as <0>): only as templates do
 * they land behind the last kernel of the library in the code object ("Headline check"; mgc_cc_ops.inl says why).
 *
 * Work lists.  A round is one launch of k_geo_tile over list[cur]; it fills list[nxt].  A tile is appended by whoever first turns
 * its word of flag[nxt] from 0 to 1 (one exchange, then one add on the length: integer atomics, the order of a list cannot matter);
 * the visit of a tile clears its word of flag[cur], which nobody else touches in that launch.  No workgroup waits for another and
 * nothing spins: a phase boundary is a kernel boundary.
 *
 * Coherence.  A visit reads the border cells of its neighbours from the plane while those neighbours may be writing them in the same
 * launch, with plain loads and stores.  That is safe for two reasons only: an aligned 8-byte word is not torn and only ever falls,
 * so whatever is read -- old or new -- is the sum of a real path; and whoever lowers such a cell wakes its readers for the NEXT
 * round, whose launch sees every store of this one.  A stale read costs a visit, never a wrong number.  No floating-point atomics.
 */
#ifndef MGC_GEO_OPS_INL
#define MGC_GEO_OPS_INL

#include "mgc_geo.h"

/* the work lists of a call and its counts, in blocks of the pool */
struct MgcGeoLists {
    int32_t* list[2];            /* [ntiles] each */
    uint32_t* flag[2];           /* [ntiles] each: 1 = the tile is in the list */
    uint32_t* len;               /* [2] */
    unsigned long long* info;    /* [8]: the slots of out8 */
};

struct MgcGeoWake {
    int32_t* list;
    uint32_t* flag;
    uint32_t* len;
    __device__ __forceinline__ void wake(int t) const
    {
        if (__hip_atomic_exchange(flag + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
            list[__hip_atomic_fetch_add(len, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = t;
    }
};

struct MgcGeoDev : MgcGeoWake {
    const void* img;
    int dtype;
    unsigned long long* info;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ int vote(int b) const { return __syncthreads_or(b); }
    __device__ __forceinline__ double load(const double* p) const { return *p; }
    __device__ __forceinline__ void store(double* p, double v) const { *p = v; }
    __device__ __forceinline__ double image(int64_t id) const { return mgc_load_as_double(img, dtype, id, false); }
    __device__ __forceinline__ void visited(int sweeps, bool capped) const
    {
        atomicAdd(info + MGC_GEO_SWEEPS, (unsigned long long)sweeps);
        if (capped) atomicAdd(info + MGC_GEO_CAPPED, 1ull);
    }
};

template <int GEO>
__global__ __launch_bounds__(256) void k_geo_init(MgcLattice L, const uint8_t* seeds, int full, double* plane, MgcGeoLists W)
{
    MgcGeoWake dev;
    dev.list = W.list[0];
    dev.flag = W.flag[0];
    dev.len = W.len;
    unsigned c = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < L.nvox; v += (int64_t)gridDim.x * 256) c += mgc_geo_init_voxel<0>(L, seeds, v, full != 0, plane, dev) ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(W.info + MGC_GEO_SEEDS, (unsigned long long)c);
}

/* one workgroup per entry of list[cur]; grid = its length */
template <bool FULL>
__global__ __launch_bounds__(MGC_TV) void k_geo_tile(MgcLattice L, MgcGeoSteps S, double gamma, const void* image, int dtype, double* plane, MgcGeoLists W, int cur)
{
    __shared__ double sd[MGC_GEO_CELLS], si[MGC_GEO_CELLS];
    __shared__ uint8_t wake[32];
    const int tile = W.list[cur][blockIdx.x];
    if (threadIdx.x == 0) W.flag[cur][tile] = 0u;
    MgcGeoDev dev;
    dev.list = W.list[cur ^ 1];
    dev.flag = W.flag[cur ^ 1];
    dev.len = W.len + (cur ^ 1);
    dev.img = image;
    dev.dtype = dtype;
    dev.info = W.info;
    mgc_geo_tile_step<FULL, 0, MGC_TV>(L, S, gamma, image != nullptr, tile, plane, sd, si, wake, (int)threadIdx.x, dev);
}

template <int GEO>
__global__ __launch_bounds__(256) void k_geo_finite(const double* plane, int64_t nvox, unsigned long long* info)
{
    unsigned c = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) c += plane[v] < MGC_EDT_INF ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(info + MGC_GEO_FINITE, (unsigned long long)c);
}

/* k_tw_binned with the image, bin and table reads replaced by the two distance planes and the rule of the term (mgc_geo_term): voxel p
 * gets one Graph::add_tweights(S(p), K(p)) on top of what the store holds (FRESH false: mgc_add_tweights_geodesic) or on top of a zero
 * t-link and a zero share (FRESH true: mgc_update_tweights_geodesic).  A thread takes two neighbouring voxels; the last entry of an
 * odd volume on its own.  changed (or NULL): += voxels whose t-link is not bit for bit what it was. */
template <bool FRESH>
__global__ __launch_bounds__(256) void k_tw_geodesic(int64_t n, const double* __restrict__ dist_f, const double* __restrict__ dist_b, double lam, double* __restrict__ tr_plane,
                                                    double* __restrict__ share_plane, unsigned long long* changed)
{
    const int64_t npairs = (n + 1) / 2;
    unsigned c = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        const bool two = 2 * i + 1 < n;
        double df[2] = {0.0, 0.0}, db[2] = {0.0, 0.0}, tr[2] = {0.0, 0.0}, fc[2] = {0.0, 0.0}, old[2];
        if (two) {
            const MgcTwPair<double> fp2 = ((const MgcTwPair<double>*)dist_f)[i];
            const MgcTwPair<double> bp2 = ((const MgcTwPair<double>*)dist_b)[i];
            const MgcTwPair<double> tp = ((const MgcTwPair<double>*)tr_plane)[i];
            df[0] = fp2.a; df[1] = fp2.b;
            db[0] = bp2.a; db[1] = bp2.b;
            old[0] = tp.a; old[1] = tp.b;
            if (!FRESH) {
                const MgcTwPair<double> fp = ((const MgcTwPair<double>*)share_plane)[i];
                fc[0] = fp.a; fc[1] = fp.b;
            }
        } else {
            df[0] = dist_f[2 * i];
            db[0] = dist_b[2 * i];
            old[0] = old[1] = tr_plane[2 * i];
            if (!FRESH) fc[0] = share_plane[2 * i];
        }
        if (!FRESH) { tr[0] = old[0]; tr[1] = old[1]; }
        double s, k;
        mgc_geo_term(df[0], db[0], lam, &s, &k);
        mgc_add_tweights(tr[0], fc[0], s, k);
        if (two) {
            mgc_geo_term(df[1], db[1], lam, &s, &k);
            mgc_add_tweights(tr[1], fc[1], s, k);
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

#endif /* MGC_GEO_OPS_INL */
