/*
 * mgc_edit_ops.inl -- the two ends of an interactive edit ("Edits by list"): markers edited by a list of voxel ids on
 * the resident mask planes (mgc_edit_markers), and the labels read back as the ascending list of voxels whose label differs from
 * the previous solve's (mgc_labels_delta).  Streaming kernels over byte planes in C order, nothing tiled: plain loads and stores,
 * one wave is the unit of work, no barriers outside the scan of the segment counts.
 */
#ifndef MGC_EDIT_OPS_INL
#define MGC_EDIT_OPS_INL

/* ops of one entry of mgc_edit_markers */
#define MGC_EDIT_SET_FG 1u
#define MGC_EDIT_SET_BG 2u
#define MGC_EDIT_CLEAR_FG 4u
#define MGC_EDIT_CLEAR_BG 8u

/* a wave compares MGC_DELTA_ITERS x 64 lanes x 16 bytes of the two label volumes: one SEGMENT.  The segments' counts are scanned,
 * then every wave writes the ids of its segment behind those of the segments before it: the output is ascending whatever the
 * order in which the waves run. */
#define MGC_DELTA_ITERS 16
#define MGC_DELTA_SEG ((int64_t)MGC_DELTA_ITERS * 64 * 16)
#define MGC_SCAN_THREADS 1024

/* one thread per entry; the host has checked the ids (in range, none twice): no two threads write the same byte */
__global__ __launch_bounds__(256) void k_edit_markers(int64_t n, int64_t nvox, const int64_t* __restrict__ ids, const uint8_t* __restrict__ ops,
                                                      uint8_t* __restrict__ fg, uint8_t* __restrict__ bg)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[k];
        const unsigned op = ops[k];
        if (id < 0 || id >= nvox) continue;
        if (fg) {
            if (op & MGC_EDIT_SET_FG) fg[id] = 1;
            else if (op & MGC_EDIT_CLEAR_FG) fg[id] = 0;
        }
        if (bg) {
            if (op & MGC_EDIT_SET_BG) bg[id] = 1;
            else if (op & MGC_EDIT_CLEAR_BG) bg[id] = 0;
        }
    }
}

/* bit j = byte j of the 16 differs; `vec` = index of the 16-byte vector, the volume's tail (nvox % 16 bytes) is read byte by byte */
__device__ __forceinline__ unsigned mgc_delta_mask(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t vec, int64_t nvox)
{
    const int64_t base = vec * 16;
    if (base >= nvox) return 0u;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (base + 16 <= nvox) {
        const uint4 x = *(const uint4*)(a + base), y = *(const uint4*)(b + base);
        w[0] = x.x ^ y.x; w[1] = x.y ^ y.y; w[2] = x.z ^ y.z; w[3] = x.w ^ y.w;
    } else {
        const int rem = (int)(nvox - base);
        for (int j = 0; j < rem; ++j) w[j >> 2] |= (uint32_t)(a[base + j] ^ b[base + j]) << (8 * (j & 3));
    }
    if (!(w[0] | w[1] | w[2] | w[3])) return 0u;
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((w[q] >> (8 * j)) & 0xffu) m |= 1u << (4 * q + j);
    return m;
}

/* pass 1: cnt[s] = differing voxels of segment s */
__global__ __launch_bounds__(256) void k_labels_delta_count(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int64_t nvox, int64_t nseg,
                                                            unsigned long long* __restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        unsigned c = 0u;
#pragma unroll 4
        for (int it = 0; it < MGC_DELTA_ITERS; ++it)
            c += (unsigned)__popc(mgc_delta_mask(cur, prev, (s * MGC_DELTA_ITERS + it) * 64 + lane, nvox));
        if (__ballot(c != 0u) != 0ull) { /* (an edit flips a few dozen labels: nearly every segment is quiet) */
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += (unsigned)__shfl_xor((int)c, d, 64);
        }
        if (lane == 0) cnt[s] = c;
    }
}

/* in place: cnt[s] -> number of differing voxels in the segments before s; cnt[nseg] = their total.  One workgroup. */
__global__ __launch_bounds__(MGC_SCAN_THREADS) void k_labels_delta_scan(unsigned long long* __restrict__ cnt, int64_t nseg)
{
    __shared__ unsigned long long part[MGC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (nseg + MGC_SCAN_THREADS - 1) / MGC_SCAN_THREADS;
    const int64_t lo = (int64_t)t * per < nseg ? (int64_t)t * per : nseg, hi = lo + per < nseg ? lo + per : nseg;
    unsigned long long sum = 0ull;
    for (int64_t s = lo; s < hi; ++s) sum += cnt[s];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < MGC_SCAN_THREADS; d <<= 1) { /* inclusive scan of the threads' sums */
        const unsigned long long add = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned long long run = part[t] - sum;
    for (int64_t s = lo; s < hi; ++s) {
        const unsigned long long c = cnt[s];
        cnt[s] = run;
        run += c;
    }
    if (t == MGC_SCAN_THREADS - 1) cnt[nseg] = part[t];
}

/* pass 2: the ids of segment s, ascending, from out[off[s]] on; n = the total (nothing is written at or behind out[n]) */
__global__ __launch_bounds__(256) void k_labels_delta_write(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int64_t nvox, int64_t nseg,
                                                            const unsigned long long* __restrict__ off, int64_t n, int64_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
        if (off[s + 1] == off[s]) continue; /* (uniform over the wave) */
        int64_t at = (int64_t)off[s];
        for (int it = 0; it < MGC_DELTA_ITERS; ++it) {
            const int64_t vec = (s * MGC_DELTA_ITERS + it) * 64 + lane;
            unsigned m = mgc_delta_mask(cur, prev, vec, nvox);
            if (__ballot(m != 0u) == 0ull) continue;
            const int c = __popc(m);
            int incl = c; /* inclusive scan of the lanes' counts */
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            int64_t p = at + (incl - c);
            while (m) {
                const int j = __ffs((int)m) - 1;
                m &= m - 1u;
                if (p < n) out[p] = vec * 16 + j;
                ++p;
            }
            at += __shfl(incl, 63, 64);
        }
    }
}

#endif /* MGC_EDIT_OPS_INL */
