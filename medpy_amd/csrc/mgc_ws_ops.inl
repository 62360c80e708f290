/*
 * mgc_ws_ops.inl -- the kernels of mgc_watershed_image and mgc_local_minima_image.  The steps themselves are mgc_ws.h;
 * here they get their workgroups and the agent-scope atomics of the work lists:
 *
 *   k_ws_init          a thread per voxel: mgc_ws_init_voxel, and the count of the seeds
 *   k_ws_tile          one workgroup of 512 threads per ACTIVE tile: mgc_ws_tile_step
 *   k_ws_parent        a thread per voxel: mgc_ws_parent, and the count of the reached voxels
 *   k_ws_jump          parent[p] = parent[parent[p]]; a device counter says whether anything moved
 *   k_ws_label         labels[p] = markers[root of p], 0 where there is none
 *   k_ws_keys          image -> the plane of its keys
 *   k_minfilter_axis   the running minimum of window `size` along one axis of a key plane, scipy's `reflect` border
 *   k_ws_minima        mask[p] = (key(p) == min(p)), and their count
 *
 * Every kernel here is a template, the plain ones over a parameter WS that nothing reads (instantiated as <0>): only as templates do
 * they land where the host code first names them in the code object ("Headline check"; mgc_cc_ops.inl says why).
 *
 * Work lists and coherence are those of mgc_geo_ops.inl: a round is one launch of k_ws_tile over list[cur], it fills list[nxt]; a
 * visit reads the border cells of its neighbours from the plane while they may be writing them, with plain loads and stores of
 * aligned 8-byte words that only ever fall and are each the key of a real path, and whoever lowers one wakes its readers for the
 * NEXT round.  A stale read costs a visit, never a wrong word.  k_ws_jump reads words other threads of the launch replace: an
 * aligned 4-byte word, old or new an ancestor of the reader in the same tree.
 */
#ifndef MGC_WS_OPS_INL
#define MGC_WS_OPS_INL

#include "mgc_ws.h"

struct MgcWsLists {
    int32_t* list[2];         /* [ntiles] each */
    uint32_t* flag[2];        /* [ntiles] each: 1 = the tile is in the list */
    uint32_t* len;            /* [2] */
    unsigned long long* info; /* [8]: the slots of out8; [8]: did a jump round move anything */
};

struct MgcWsWake {
    int32_t* list;
    uint32_t* flag;
    uint32_t* len;
    __device__ __forceinline__ void wake(int t) const
    {
        if (__hip_atomic_exchange(flag + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
            list[__hip_atomic_fetch_add(len, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = t;
    }
};

struct MgcWsDev : MgcWsWake {
    unsigned long long* info;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ int vote(int b) const { return __syncthreads_or(b); }
    __device__ __forceinline__ uint64_t load(const uint64_t* p) const { return *p; }
    __device__ __forceinline__ void store(uint64_t* p, uint64_t v) const { *p = v; }
    __device__ __forceinline__ void visited(int sweeps, bool capped) const
    {
        atomicAdd(info + MGC_WS_SWEEPS, (unsigned long long)sweeps);
        if (capped) atomicAdd(info + MGC_WS_CAPPED, 1ull);
    }
};

/* sum over the wave, one atomic per wave that has something */
__device__ __forceinline__ void mgc_ws_count(unsigned c, unsigned long long* slot)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(slot, (unsigned long long)c);
}

template <int WS>
__global__ __launch_bounds__(256) void k_ws_init(MgcLattice L, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, uint64_t* plane, MgcWsLists W)
{
    MgcWsWake dev;
    dev.list = W.list[0];
    dev.flag = W.flag[0];
    dev.len = W.len;
    unsigned c = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < L.nvox; v += (int64_t)gridDim.x * 256) c += mgc_ws_init_voxel(L, image, dtype, markers, mask, v, plane, dev) ? 1u : 0u;
    mgc_ws_count(c, W.info + MGC_WS_SEEDS);
}

/* one workgroup per entry of list[cur]; grid = its length */
template <int WS>
__global__ __launch_bounds__(MGC_TV) void k_ws_tile(MgcLattice L, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, uint64_t* plane, MgcWsLists W, int cur)
{
    __shared__ uint64_t st[MGC_WS_CELLS];
    __shared__ uint8_t wake[8];
    const int tile = W.list[cur][blockIdx.x];
    if (threadIdx.x == 0) W.flag[cur][tile] = 0u;
    MgcWsDev dev;
    dev.list = W.list[cur ^ 1];
    dev.flag = W.flag[cur ^ 1];
    dev.len = W.len + (cur ^ 1);
    dev.info = W.info;
    mgc_ws_tile_step<0, MGC_TV>(L, image, dtype, markers, mask, tile, plane, st, wake, (int)threadIdx.x, dev);
}

template <int WS>
__global__ __launch_bounds__(256) void k_ws_parent(MgcLattice L, const uint64_t* plane, const int32_t* markers, const uint8_t* mask, uint32_t* parent, unsigned long long* info)
{
    unsigned c = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < L.nvox; v += (int64_t)gridDim.x * 256) {
        const uint32_t q = mgc_ws_parent(L, plane, markers, mask, v);
        parent[v] = q;
        c += q != MGC_WS_NONE ? 1u : 0u;
    }
    mgc_ws_count(c, info + MGC_WS_REACHED);
}

/* one round of pointer jumping; *moved becomes 1 where a word changed */
template <int WS>
__global__ __launch_bounds__(256) void k_ws_jump(int64_t nvox, uint32_t* parent, unsigned long long* moved)
{
    bool any = false;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const uint32_t q = parent[v];
        if (q == MGC_WS_NONE) continue;
        const uint32_t r = parent[q];
        if (r != q) { parent[v] = r; any = true; }
    }
    if (__syncthreads_or(any ? 1 : 0) && threadIdx.x == 0) *moved = 1ull;
}

template <int WS>
__global__ __launch_bounds__(256) void k_ws_label(int64_t nvox, const uint32_t* parent, const int32_t* markers, int32_t* labels)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const uint32_t q = parent[v];
        labels[v] = q == MGC_WS_NONE ? 0 : markers[q];
    }
}

template <int WS>
__global__ __launch_bounds__(256) void k_ws_keys(int64_t nvox, const void* image, int dtype, uint32_t* keys)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) keys[v] = mgc_ws_key(image, dtype, v);
}

/* dst[p] = min of the window of `size` along the axis whose extent is n and whose stride is `stride` (in words) */
template <int WS>
__global__ __launch_bounds__(256) void k_minfilter_axis(int64_t nvox, int64_t n, int64_t stride, int size, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const int64_t i = (v / stride) % n;
        dst[v] = mgc_ws_window_min(src + (v - i * stride), stride, n, i, size);
    }
}

template <int WS>
__global__ __launch_bounds__(256) void k_ws_minima(int64_t nvox, const uint32_t* keys, const uint32_t* mins, uint8_t* mask, unsigned long long* count)
{
    unsigned c = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const bool m = keys[v] == mins[v];
        mask[v] = m ? 1 : 0;
        c += m ? 1u : 0u;
    }
    mgc_ws_count(c, count);
}

#endif /* MGC_WS_OPS_INL */
