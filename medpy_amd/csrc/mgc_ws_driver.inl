/*
 * mgc_ws_driver.inl -- the host side of mgc_watershed_image and mgc_local_minima_image.  Included ONCE, at the end of
 * mgc_kernels.hip behind mgc_diffuse_driver.inl and in front of the block of six drivers that ends the file: the kernels of
 * mgc_ws_ops.inl come in here, behind the kernels of the solve and of the diffusion, which keep their places in the code object
 * ("Headline check"); the kernels of the six drivers move down by the size of these.  Both entries are handle-free, like
 * mgc_diffuse_image: a stream of their own, every block from the pool and every block given back.  Every check comes before the
 * first allocation.
 */
#include "mgc_ws_ops.inl"

struct MgcWsTimes { double upload_ms = 0.0, flood_ms = 0.0, parent_ms = 0.0, resolve_ms = 0.0, download_ms = 0.0; };

/* four events of a call; destroyed with it */
struct MgcWsEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
        return e;
    }
    hipError_t between(int a, int b, double* ms) const
    {
        float f = 0.0f;
        const hipError_t e = hipEventElapsedTime(&f, ev[a], ev[b]);
        *ms = (double)f;
        return e;
    }
    ~MgcWsEvents()
    {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
};

static unsigned mgc_ws_grid(int64_t nvox)
{
    const int64_t b = (nvox + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b < 65536 ? b : 65536));
}

/* what both entries refuse about the volume and the image; MGC_OK with dims (z, y, x) and the voxel count filled */
static int mgc_ws_volume(const char* name, int device, int ndim, const int64_t* shape, const void* image, int dtype, int64_t dims[3], int64_t* nvox)
{
    if (ndim < 1 || ndim > 3) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: ndim = %d: 1 to 3 axes", name, ndim);
    if (!shape) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: shape NULL", name);
    dims[0] = dims[1] = dims[2] = 1;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 1) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: shape[%d] = %lld: every extent must be at least 1", name, i, (long long)shape[i]);
        dims[3 - ndim + i] = shape[i];
        if (shape[i] >= MGC_WS_MAX_VOXELS || n > (MGC_WS_MAX_VOXELS - 1) / shape[i])
            return mgc_fail(nullptr, MGC_ERR_UNSUPPORTED, "%s: volumes of 2^32 - 1 voxels or more are not supported (32-bit step counts and parents)", name);
        n *= shape[i];
    }
    if (!image) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: image NULL", name);
    if (dtype == MGC_U64 || dtype == MGC_I64 || dtype == MGC_F64)
        return mgc_fail(nullptr, MGC_ERR_UNSUPPORTED, "%s: 64-bit images (dtype %d) are not supported: rank the values and send them as MGC_U32", name, dtype);
    if (!mgc_dtype_size(dtype)) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: bad dtype %d", name, dtype);
    if (dtype == MGC_F32) {
        const uint32_t* const bits = (const uint32_t*)image;
        for (int64_t v = 0; v < n; ++v)
            if (!mgc_ws_finite_bits(bits[v])) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: image[%lld] is not finite", name, (long long)v);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return mgc_fail(nullptr, MGC_ERR_NO_DEVICE, "no HIP device: libmedpyhip has no CPU fallback");
    if (device < 0 || device >= ndev) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: device %d of %d", name, device, ndev);
    *nvox = n;
    return MGC_OK;
}

/* the flood, the parents and the labels on `stream`; info: the eight slots of out8 */
static hipError_t mgc_ws_run(hipStream_t stream, MgcBlocks& pool, const MgcLattice& L, const void* d_image, int dtype, const int32_t* d_markers, const uint8_t* d_mask,
                             int32_t* d_labels, unsigned long long info[8], MgcWsTimes* ms, bool* stuck)
{
    const int64_t nvox = L.nvox;
    const size_t nt = (size_t)L.ntiles;
    uint64_t* const plane = (uint64_t*)pool.get((size_t)nvox * sizeof(uint64_t));
    uint32_t* const parent = (uint32_t*)pool.get((size_t)nvox * sizeof(uint32_t));
    int32_t* const lists = (int32_t*)pool.get(2 * nt * sizeof(int32_t));
    uint32_t* const flags = (uint32_t*)pool.get(2 * nt * sizeof(uint32_t));
    unsigned long long* const words = (unsigned long long*)pool.get(10 * sizeof(unsigned long long)); /* info[8], moved, the two lengths */
    *stuck = false;
    for (int k = 0; k < 8; ++k) info[k] = 0ull;
    if (pool.err != hipSuccess) return pool.err;
    MgcWsLists W;
    W.list[0] = lists; W.list[1] = lists + nt;
    W.flag[0] = flags; W.flag[1] = flags + nt;
    W.info = words;
    W.len = (uint32_t*)(words + 9);
    /* flood_ms, parent_ms and resolve_ms lie between four events on the stream */
    MgcWsEvents ev;
    hipError_t e = ev.create();
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 2 * nt * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(words, 0, 10 * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipEventRecord(ev.ev[0], stream);
    if (e != hipSuccess) return e;
    const unsigned grid = mgc_ws_grid(nvox);
    hipLaunchKernelGGL(k_ws_init<0>, dim3(grid), dim3(256), 0, stream, L, d_image, dtype, d_markers, d_mask, plane, W);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t len[2] = {0u, 0u};
    if ((e = hipMemcpyAsync(len, W.len, sizeof(len), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    /* A round is one launch over the tiles the round before woke; the host looks at the length of the next list after every launch
       and stops at the round that woke nobody.  After round r every voxel whose best path has at most r arcs holds its word, and a
       path visits a voxel once: more than nvox + 1 rounds cannot happen, and *stuck says so instead of spinning. */
    int64_t rounds = 0, visits = 0;
    const int64_t max_rounds = nvox + 1;
    for (int cur = 0; len[cur] > 0u; cur ^= 1) {
        if (rounds >= max_rounds) { *stuck = true; return hipSuccess; }
        const int nxt = cur ^ 1;
        if ((e = hipMemsetAsync(W.len + nxt, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_ws_tile<0>, dim3(len[cur]), dim3(MGC_TV), 0, stream, L, d_image, dtype, d_markers, d_mask, plane, W, cur);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&len[nxt], W.len + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        visits += (int64_t)len[cur];
        ++rounds;
    }
    if ((e = hipEventRecord(ev.ev[1], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ws_parent<0>, dim3(grid), dim3(256), 0, stream, L, (const uint64_t*)plane, d_markers, d_mask, parent, words);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev.ev[2], stream)) != hipSuccess) return e;
    /* a round halves the distance to the root at least: chains are shorter than 2^32, so 32 rounds move something at most, and the
       one that moves nothing ends the loop */
    int64_t jumps = 0;
    for (;;) {
        if (jumps > 33) { *stuck = true; return hipSuccess; }
        unsigned long long moved = 0ull;
        if ((e = hipMemsetAsync(words + 8, 0, sizeof(unsigned long long), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_ws_jump<0>, dim3(grid), dim3(256), 0, stream, nvox, parent, words + 8);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&moved, words + 8, sizeof(moved), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        ++jumps;
        if (!moved) break;
    }
    hipLaunchKernelGGL(k_ws_label<0>, dim3(grid), dim3(256), 0, stream, nvox, (const uint32_t*)parent, d_markers, d_labels);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev.ev[3], stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(info, words, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if ((e = ev.between(0, 1, &ms->flood_ms)) != hipSuccess) return e;
    if ((e = ev.between(1, 2, &ms->parent_ms)) != hipSuccess) return e;
    if ((e = ev.between(2, 3, &ms->resolve_ms)) != hipSuccess) return e;
    info[MGC_WS_ROUNDS] = (unsigned long long)rounds;
    info[MGC_WS_VISITS] = (unsigned long long)visits;
    info[MGC_WS_JUMPS] = (unsigned long long)jumps;
    info[7] = 0ull;
    return hipSuccess;
}

extern "C" {

int mgc_watershed_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, int32_t* labels_out, int64_t* out8)
{
    const char* const name = "mgc_watershed_image";
    if (!markers) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: markers NULL", name);
    if (!labels_out) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: labels_out NULL", name);
    int64_t dims[3], nvox = 0;
    { const int rc = mgc_ws_volume(name, device, ndim, shape, image, dtype, dims, &nvox); if (rc) return rc; }
    for (int64_t v = 0; v < nvox; ++v)
        if (markers[v] < 0) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: markers[%lld] = %d: a marker is 0 (none) or a positive label", name, (long long)v, (int)markers[v]);
    MgcLattice L;
    mgc_ws_lattice(dims, &L);
    MGC_HIP(nullptr, hipSetDevice(device));
    hipStream_t stream = nullptr;
    MGC_HIP(nullptr, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    MgcWsTimes ms;
    unsigned long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool stuck = false;
    hipError_t e;
    {
        MgcBlocks pool;
        const size_t ibytes = (size_t)nvox * mgc_dtype_size(dtype), lbytes = (size_t)nvox * sizeof(int32_t);
        void* const d_image = pool.get(ibytes);
        int32_t* const d_markers = (int32_t*)pool.get(lbytes);
        uint8_t* const d_mask = mask ? (uint8_t*)pool.get((size_t)nvox) : nullptr;
        int32_t* const d_labels = (int32_t*)pool.get(lbytes);
        e = pool.err;
        auto t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess) e = hipMemcpyAsync(d_image, image, ibytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_markers, markers, lbytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && mask) e = hipMemcpyAsync(d_mask, mask, (size_t)nvox, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        ms.upload_ms = mgc_ms_since(t0);
        if (e == hipSuccess) e = mgc_ws_run(stream, pool, L, d_image, dtype, d_markers, d_mask, d_labels, info, &ms, &stuck);
        t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess && !stuck) e = hipMemcpyAsync(labels_out, d_labels, lbytes, hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = e2;
        ms.download_ms = mgc_ms_since(t0);
    }
    (void)hipStreamDestroy(stream);
    if (e != hipSuccess) return mgc_hip_fail(nullptr, name, e);
    if (stuck) return mgc_fail(nullptr, MGC_ERR_HIP, "%s: the flood or the label resolve did not reach its fixpoint within its bound of rounds", name);
    if (out8)
        for (int k = 0; k < 8; ++k) out8[k] = (int64_t)info[k];
    /* no error: the note says where the time of this call went (tools/gpu_watershed.py records it) */
    (void)mgc_fail(nullptr, MGC_OK, "%s: upload_ms=%.3f flood_ms=%.3f parent_ms=%.3f resolve_ms=%.3f download_ms=%.3f", name, ms.upload_ms, ms.flood_ms, ms.parent_ms, ms.resolve_ms,
                   ms.download_ms);
    return MGC_OK;
}

int mgc_local_minima_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, int size, uint8_t* mask_out, int64_t* out4)
{
    const char* const name = "mgc_local_minima_image";
    if (!mask_out) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: mask_out NULL", name);
    if (size < 1) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: size = %d: the window must hold at least one voxel", name, size);
    int64_t dims[3], nvox = 0;
    { const int rc = mgc_ws_volume(name, device, ndim, shape, image, dtype, dims, &nvox); if (rc) return rc; }
    MGC_HIP(nullptr, hipSetDevice(device));
    hipStream_t stream = nullptr;
    MGC_HIP(nullptr, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    double upload_ms = 0.0, filter_ms = 0.0, download_ms = 0.0;
    unsigned long long minima = 0ull;
    hipError_t e;
    {
        MgcBlocks pool;
        const size_t ibytes = (size_t)nvox * mgc_dtype_size(dtype), kbytes = (size_t)nvox * sizeof(uint32_t);
        void* const d_image = pool.get(ibytes);
        uint32_t* const keys = (uint32_t*)pool.get(kbytes);
        uint32_t* buf[2] = {(uint32_t*)pool.get(kbytes), (uint32_t*)pool.get(kbytes)};
        uint8_t* const d_mask = (uint8_t*)pool.get((size_t)nvox);
        unsigned long long* const count = (unsigned long long*)pool.get(sizeof(unsigned long long));
        e = pool.err;
        auto t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess) e = hipMemcpyAsync(d_image, image, ibytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemsetAsync(count, 0, sizeof(unsigned long long), stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        upload_ms = mgc_ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        const unsigned grid = mgc_ws_grid(nvox);
        const uint32_t* src = keys;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_ws_keys<0>, dim3(grid), dim3(256), 0, stream, nvox, (const void*)d_image, dtype, keys);
            e = hipGetLastError();
        }
        /* one pass per axis longer than one voxel (an axis of one voxel is its own minimum under `reflect`) */
        const int64_t strides[3] = {dims[1] * dims[2], dims[2], 1};
        int pass = 0;
        for (int a = 0; a < 3 && e == hipSuccess; ++a) {
            if (dims[a] == 1 || size == 1) continue;
            uint32_t* const dst = buf[pass & 1];
            hipLaunchKernelGGL(k_minfilter_axis<0>, dim3(grid), dim3(256), 0, stream, nvox, dims[a], strides[a], size, src, dst);
            e = hipGetLastError();
            src = dst;
            ++pass;
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_ws_minima<0>, dim3(grid), dim3(256), 0, stream, nvox, (const uint32_t*)keys, src, d_mask, count);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        filter_ms = mgc_ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess) e = hipMemcpyAsync(mask_out, d_mask, (size_t)nvox, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&minima, count, sizeof(minima), hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = e2;
        download_ms = mgc_ms_since(t0);
    }
    (void)hipStreamDestroy(stream);
    if (e != hipSuccess) return mgc_hip_fail(nullptr, name, e);
    if (out4) { out4[0] = (int64_t)minima; out4[1] = 0; out4[2] = 0; out4[3] = 0; }
    (void)mgc_fail(nullptr, MGC_OK, "%s: upload_ms=%.3f filter_ms=%.3f download_ms=%.3f", name, upload_ms, filter_ms, download_ms);
    return MGC_OK;
}

} /* extern "C" */
