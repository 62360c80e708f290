/*
 * mgc_cc_ops.inl -- the kernels of mgc_components and mgc_clean_labels.  The steps themselves are mgc_cc.h; here they
 * get their workgroups, the agent-scope atomics of the device, and the ranking:
 *
 *   k_cc_normalise   a caller's plane to 0 / 1 bytes, in place (what the changed list of mgc_clean_labels compares)
 *   k_cc_tile        one workgroup per tile: mgc_cc_tile_step
 *   k_cc_merge       one workgroup per tile, a thread per voxel: mgc_cc_merge_voxel
 *   k_cc_flatten     a thread per voxel: mgc_cc_flatten_voxel
 *   k_cc_gather      a thread per voxel: mgc_cc_gather_voxel
 *   k_cc_seg_count   one wave per segment of MGC_CC_SEG voxels: roots, voxels of this side, the largest root of the segment
 *   (k_labels_delta_scan of mgc_edit_ops.inl turns the root counts into offsets: the roots come out ascending)
 *   k_cc_seg_reduce  one workgroup: the segments' sums and maxima in a fixed order
 *   k_cc_rank_write  one wave per segment: the rows of the table, and rank + 1 into the root's count word
 *   k_cc_ids         parent word -> id of the component (0: the other side), in place
 *   k_cc_apply       out = base | keep[id - 1]
 *
 * Every kernel here is a template, the plain ones over a parameter CC that nothing reads (instantiated as <0>): the compiler emits the
 * instances of templates behind all plain kernels of the file, so only as templates do these land behind the last kernel of the
 * library in the code object and leave the addresses of the kernels of the solve where they were ("Headline check";
 * k_label_hist is behind them for the same reason).
 *
 * Visibility between workgroups (MI355X: the L2s of the eight XCDs are not coherent for plain loads, a CU's L1 is never refreshed by
 * another CU's stores): a phase boundary is a kernel boundary, nothing here spins on a word or waits for another workgroup.  Inside
 * k_cc_merge and k_cc_flatten, the two kernels whose workgroups write words that others read in the same launch, every access to the
 * parent plane is an agent-scope atomic; and no plain-loaded "I am a root" is trusted: the value fetch_min returns decides.
 */
#ifndef MGC_CC_OPS_INL
#define MGC_CC_OPS_INL

#include "mgc_cc.h"

struct MgcCcAtomDev {
    __device__ __forceinline__ uint32_t load(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(uint32_t* p, uint32_t v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t* p, uint32_t v) const { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void add(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    /* byte i of a plane whose base is aligned to four bytes (every block of the pool is): an OR on the word that holds it */
    __device__ __forceinline__ void or_byte(uint8_t* base, uint32_t i, uint8_t f) const
    {
        (void)__hip_atomic_fetch_or((uint32_t*)(base + (i & ~3u)), (uint32_t)f << (8u * (i & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    /* words in LDS */
    __device__ __forceinline__ void chip_add(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void chip_or(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct MgcCcBarrier {
    __device__ __forceinline__ int operator()(int v) const { return __syncthreads_or(v); }
    __device__ __forceinline__ int bits(int v) const
    {
        /* the OR of every thread's bits, not of their truth values: one vote per bit */
        int r = 0;
        for (int b = 0; b < 3; ++b)
            if (__syncthreads_or(v & (1 << b))) r |= 1 << b;
        return r;
    }
};

template <int CC>
__global__ __launch_bounds__(256) void k_cc_normalise(uint8_t* plane, int64_t nvox)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) plane[v] = plane[v] ? 1 : 0;
}

/* tsum: the label summaries of the current cut (k_labels8: 0 all sink side, 1 all source side, 2 both) or NULL */
template <bool FULL>
__global__ __launch_bounds__(MGC_TV) void k_cc_tile(MgcLattice L, const uint8_t* plane, int side, const uint8_t* tsum, const uint8_t* fg, const uint8_t* bg, uint32_t* parent,
                                                    uint32_t* count, uint8_t* flags, unsigned long long* info)
{
    __shared__ uint16_t lab[MGC_CC_BLOCK];
    __shared__ uint32_t acc[2 * MGC_TV];
    MgcCcAtomDev at;
    MgcCcBarrier barrier;
    unsigned long long skipped = 0, processed = 0; /* (thread 0) */
    for (int tile = (int)blockIdx.x; tile < L.ntiles; tile += (int)gridDim.x) {
        const int s = tsum ? (int)tsum[tile] : 2;
        const int hint = s == 2 ? 0 : ((s != 0) == (side != 0) ? 2 : 1);
        if (hint) skipped++;
        else processed++;
        mgc_cc_tile_step<FULL>(L, plane, side, hint, fg, bg, tile, parent, count, flags, lab, acc, (int)threadIdx.x, MGC_TV, at, barrier);
        __syncthreads(); /* (the next tile of this workgroup rewrites the cells) */
    }
    if (threadIdx.x == 0) {
        if (skipped) atomicAdd(info + MGC_CC_TILES_SKIPPED, skipped);
        if (processed) atomicAdd(info + MGC_CC_TILES_PROCESSED, processed);
    }
}

template <bool FULL>
__global__ __launch_bounds__(MGC_TV) void k_cc_merge(MgcLattice L, uint32_t* parent, unsigned long long* info)
{
    __shared__ uint32_t s_unions, s_walk;
    MgcCcAtomDev at;
    if (threadIdx.x == 0) s_unions = s_walk = 0u;
    __syncthreads();
    uint32_t unions = 0u, walk = 0u;
    for (int tile = (int)blockIdx.x; tile < L.ntiles; tile += (int)gridDim.x) {
        int tz, ty, tx;
        mgc_tile_coords(L, tile, tz, ty, tx);
        mgc_cc_merge_voxel<FULL>(L, parent, tz, ty, tx, (int)threadIdx.x, at, unions, walk);
    }
    if (unions) atomicAdd(&s_unions, unions);
    if (walk) atomicMax(&s_walk, walk);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_unions) atomicAdd(info + MGC_CC_UNIONS, (unsigned long long)s_unions);
        if (s_walk) atomicMax(info + MGC_CC_LONGEST_WALK, (unsigned long long)s_walk);
    }
}

template <int CC>
__global__ __launch_bounds__(256) void k_cc_flatten(uint32_t* parent, int64_t nvox, unsigned long long* info)
{
    __shared__ uint32_t s_walk;
    MgcCcAtomDev at;
    if (threadIdx.x == 0) s_walk = 0u;
    __syncthreads();
    uint32_t walk = 0u;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) mgc_cc_flatten_voxel(parent, (uint32_t)v, at, walk);
    if (walk) atomicMax(&s_walk, walk);
    __syncthreads();
    if (threadIdx.x == 0 && s_walk) atomicMax(info + MGC_CC_LONGEST_WALK, (unsigned long long)s_walk);
}

template <int CC>
__global__ __launch_bounds__(256) void k_cc_gather(const uint32_t* parent, uint32_t* count, uint8_t* flags, int64_t nvox)
{
    MgcCcAtomDev at;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) mgc_cc_gather_voxel(parent, count, flags, (uint32_t)v, at);
}

/* the largest component of a set of roots, ties to the smaller voxel id: the maximum of size << 32 | ~root */
__device__ __forceinline__ unsigned long long mgc_cc_best(uint32_t size, uint32_t root) { return ((unsigned long long)size << 32) | (unsigned long long)(0xffffffffu - root); }

/* one wave per segment.  roots[s]: voxels with parent == own id; part[2 * s]: voxels of this side, part[2 * s + 1]: mgc_cc_best */
template <int CC>
__global__ __launch_bounds__(256) void k_cc_seg_count(const uint32_t* parent, const uint32_t* count, int64_t nvox, int64_t nseg, unsigned long long* roots, unsigned long long* part)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        unsigned n_root = 0u, n_side = 0u;
        unsigned long long best = 0ull;
        for (int it = 0; it < MGC_CC_SEG / 64; ++it) {
            const int64_t v = s * MGC_CC_SEG + it * 64 + lane;
            if (v >= nvox) break;
            const uint32_t p = parent[v];
            if (p == MGC_CC_NONE) continue;
            ++n_side;
            if (p == (uint32_t)v) {
                ++n_root;
                const unsigned long long b = mgc_cc_best(count[v], p);
                if (b > best) best = b;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            n_root += (unsigned)__shfl_xor((int)n_root, d, 64);
            n_side += (unsigned)__shfl_xor((int)n_side, d, 64);
            const unsigned long long o = (unsigned long long)__shfl_xor((long long)best, d, 64);
            if (o > best) best = o;
        }
        if (lane == 0) {
            roots[s] = n_root;
            part[2 * s] = n_side;
            part[2 * s + 1] = best;
        }
    }
}

/* one workgroup: thread t takes segments t, t + 512, ...; then a tree.  info[N_SIDE], info[LARGEST_SIZE]; best_out: mgc_cc_best of the volume */
template <int CC>
__global__ __launch_bounds__(MGC_TV) void k_cc_seg_reduce(const unsigned long long* part, int64_t nseg, unsigned long long* info, unsigned long long* best_out)
{
    __shared__ unsigned long long s_sum[MGC_TV], s_best[MGC_TV];
    const int t = threadIdx.x;
    unsigned long long sum = 0ull, best = 0ull;
    for (int64_t s = t; s < nseg; s += MGC_TV) {
        sum += part[2 * s];
        if (part[2 * s + 1] > best) best = part[2 * s + 1];
    }
    s_sum[t] = sum;
    s_best[t] = best;
    __syncthreads();
    for (int off = MGC_TV / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_sum[t] += s_sum[t + off];
            if (s_best[t + off] > s_best[t]) s_best[t] = s_best[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        info[MGC_CC_N_SIDE] = s_sum[0];
        info[MGC_CC_LARGEST_SIZE] = s_best[0] >> 32;
        *best_out = s_best[0];
    }
}

/* one wave per segment; off[s]: roots in the segments before s.  Row `rank` of the table for rank < cap, then rank + 1 takes the
 * place of the root's count (the table holds the size from here on; k_cc_ids reads the id there). */
template <int CC>
__global__ __launch_bounds__(256) void k_cc_rank_write(const uint32_t* parent, uint32_t* count, const uint8_t* flags, int64_t nvox, int64_t nseg, const unsigned long long* off,
                                                       int64_t cap, int64_t* t_first, int64_t* t_size, uint8_t* t_flags)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        if (off[s + 1] == off[s]) continue; /* (uniform over the wave) */
        int64_t at = (int64_t)off[s];
        for (int it = 0; it < MGC_CC_SEG / 64; ++it) {
            const int64_t v = s * MGC_CC_SEG + it * 64 + lane;
            const bool root = v < nvox && parent[v] == (uint32_t)v;
            const unsigned long long m = __ballot(root);
            if (root) {
                const int64_t rank = at + __popcll(m & ((1ull << lane) - 1ull));
                if (rank < cap) {
                    t_first[rank] = v;
                    t_size[rank] = (int64_t)count[v];
                    t_flags[rank] = flags[v];
                }
                count[v] = (uint32_t)(rank + 1);
            }
            at += __popcll(m);
        }
    }
}

/* in place: the parent word of a voxel becomes the id of its component.  Every thread reads its own word and the count word of a
 * root, which nobody writes here.  best: mgc_cc_best of the volume, whose root's id goes to info[LARGEST_ID]. */
template <int CC>
__global__ __launch_bounds__(256) void k_cc_ids(uint32_t* parent, const uint32_t* count, int64_t nvox, const unsigned long long* best, unsigned long long* info)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long b = *best;
        info[MGC_CC_LARGEST_ID] = (b >> 32) ? (unsigned long long)count[0xffffffffu - (uint32_t)(b & 0xffffffffull)] : 0ull;
    }
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const uint32_t p = parent[v];
        parent[v] = p == MGC_CC_NONE ? 0u : count[p];
    }
}

/* out[v] = base[v] (NULL: 0) or keep[ids[v] - 1]; out may be base */
template <int CC>
__global__ __launch_bounds__(256) void k_cc_apply(const uint32_t* ids, const uint8_t* keep, const uint8_t* base, uint8_t* out, int64_t nvox)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
        const uint32_t id = ids[v];
        out[v] = (uint8_t)(((base && base[v]) || (id && keep[id - 1])) ? 1 : 0);
    }
}

#endif /* MGC_CC_OPS_INL */
