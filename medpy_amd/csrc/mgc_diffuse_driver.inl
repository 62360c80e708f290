/*
 * mgc_diffuse_driver.inl -- the host side of mgc_diffuse_image and mgc_diffuse.  Included ONCE, at the end of
 * mgc_kernels.hip behind its last function and in front of the block of six drivers that ends the file: the kernels of
 * mgc_diffuse_ops.inl come in here, behind the kernels of the solve, which keep their places in the code object (DESIGN 13,
 * "Headline check"); the kernels of the six drivers move down by the size of these.  Every check comes before the first write.  One driver (mgc_ad_run) serves both entries: two float32 buffers of the pool are ping-ponged, iteration k writes
 * buffer (k - 1) & 1, and the result is that of the last iteration (niter = 0: the float32 copy in buffer 0).  mgc_diffuse with
 * keep = 0 leaves the handle as it was; with keep = 1 the result buffer becomes the handle's feature image, exactly as
 * mgc_set_feature_image of an MGC_F32 image leaves it.  No field of the handle is new.
 */
#include "mgc_diffuse_ops.inl"

/* the image mgc_marker_histograms reads (mgc_binned_driver.inl, which comes in behind this file) */
static bool mgc_binned_image(mgc_handle h, const void** image, int* dtype);

struct MgcAdTimes { double upload_ms = 0.0, iterate_ms = 0.0, download_ms = 0.0; };

/* the iterations on `stream`: d_in (dtype) -> buf[..]; *result is the buffer that holds the answer.  iterate_ms: events around the launches */
static hipError_t mgc_ad_run(hipStream_t stream, const int64_t dims[3], const MgcDiffuse& P, const void* d_in, int dtype, int niter, float* const buf[2], float** result,
                             int64_t* bricks, double* iterate_ms)
{
    MgcAdDims D;
    D.dz = dims[0]; D.dy = dims[1]; D.dx = dims[2];
    D.bz = (int)((D.dz + MGC_AD_BZ - 1) / MGC_AD_BZ);
    D.by = (int)((D.dy + MGC_AD_BY - 1) / MGC_AD_BY);
    D.bx = (int)((D.dx + MGC_AD_BX - 1) / MGC_AD_BX);
    const int64_t nb = (int64_t)D.bz * D.by * D.bx;
    const int64_t nvox = D.dz * D.dy * D.dx;
    *bricks = nb;
    *result = buf[0];
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
    if (e == hipSuccess && niter == 0) {
        const int64_t wgs = (nvox + 255) / 256;
        hipLaunchKernelGGL(k_diffuse_convert<0>, dim3((unsigned)(wgs < 16384 ? wgs : 16384)), dim3(256), 0, stream, nvox, d_in, dtype, buf[0]);
        e = hipGetLastError();
    }
    const void* src = d_in;
    int sdt = dtype;
    for (int k = 0; k < niter && e == hipSuccess; ++k) {
        float* const dst = buf[k & 1];
        const int vec4 = sdt == MGC_F32 && D.dx % 4 == 0 && ((uintptr_t)src & 15u) == 0;
        switch (P.option) {
        case 1: hipLaunchKernelGGL(k_diffuse<1>, dim3((unsigned)nb), dim3(MGC_AD_THREADS), 0, stream, D, P, src, sdt, vec4, dst); break;
        case 2: hipLaunchKernelGGL(k_diffuse<2>, dim3((unsigned)nb), dim3(MGC_AD_THREADS), 0, stream, D, P, src, sdt, vec4, dst); break;
        default: hipLaunchKernelGGL(k_diffuse<3>, dim3((unsigned)nb), dim3(MGC_AD_THREADS), 0, stream, D, P, src, sdt, vec4, dst); break;
        }
        e = hipGetLastError();
        src = dst;
        sdt = MGC_F32;
        *result = dst;
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    *iterate_ms = (double)ms;
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    return e;
}

/* what both entries refuse, before anything else happens; MGC_OK with P and dims filled */
static int mgc_ad_args(mgc_handle h, const char* name, int ndim, const int64_t* shape, int niter, double kappa, double gamma, const double* spacing, int option, MgcDiffuse* P,
                       int64_t dims[3])
{
    char msg[256];
    if (mgc_ad_check(ndim, shape, niter, kappa, gamma, spacing, option, msg, sizeof(msg)) != MGC_AD_OK) return mgc_fail(h, MGC_ERR_INVALID, "%s: %s", name, msg);
    mgc_ad_prepare(ndim, shape, kappa, gamma, spacing, option, P, dims);
    const int64_t nb = ((dims[0] + MGC_AD_BZ - 1) / MGC_AD_BZ) * ((dims[1] + MGC_AD_BY - 1) / MGC_AD_BY) * ((dims[2] + MGC_AD_BX - 1) / MGC_AD_BX);
    if (nb > 0x7fffffffll) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: %lld bricks are more than one launch holds", name, (long long)nb);
    return MGC_OK;
}

extern "C" {

int mgc_diffuse_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, int niter, double kappa, double gamma, const double* spacing, int option, float* out,
                      int64_t* out4)
{
    const char* const name = "mgc_diffuse_image";
    MgcDiffuse P;
    int64_t dims[3];
    { const int rc = mgc_ad_args(nullptr, name, ndim, shape, niter, kappa, gamma, spacing, option, &P, dims); if (rc) return rc; }
    const size_t es = mgc_dtype_size(dtype);
    if (!image || !es) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: image NULL or bad dtype %d", name, dtype);
    if (!out) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: out NULL", name);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return mgc_fail(nullptr, MGC_ERR_NO_DEVICE, "no HIP device: libmedpyhip has no CPU fallback");
    if (device < 0 || device >= ndev) return mgc_fail(nullptr, MGC_ERR_INVALID, "%s: device %d of %d", name, device, ndev);
    MGC_HIP(nullptr, hipSetDevice(device));
    const int64_t nvox = dims[0] * dims[1] * dims[2];
    const size_t fbytes = (size_t)nvox * sizeof(float);
    hipStream_t stream = nullptr;
    MGC_HIP(nullptr, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    MgcAdTimes ms;
    int64_t bricks = 0;
    hipError_t e;
    {
        MgcBlocks pool;
        void* const d_in = pool.get((size_t)nvox * es);
        float* buf[2] = {(float*)pool.get(fbytes), niter > 1 ? (float*)pool.get(fbytes) : nullptr};
        e = pool.err;
        auto t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess) e = hipMemcpyAsync(d_in, image, (size_t)nvox * es, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        ms.upload_ms = mgc_ms_since(t0);
        float* result = nullptr;
        if (e == hipSuccess) e = mgc_ad_run(stream, dims, P, d_in, dtype, niter, buf, &result, &bricks, &ms.iterate_ms);
        t0 = std::chrono::steady_clock::now();
        if (e == hipSuccess) e = hipMemcpyAsync(out, result, fbytes, hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = e2;
        ms.download_ms = mgc_ms_since(t0);
    }
    (void)hipStreamDestroy(stream);
    if (e != hipSuccess) return mgc_hip_fail(nullptr, name, e);
    if (out4) { out4[0] = niter; out4[1] = bricks; out4[2] = 0; out4[3] = 0; }
    /* no error: the note says where the time of this call went (tools/gpu_diffusion.py records it) */
    (void)mgc_fail(nullptr, MGC_OK, "%s: upload_ms=%.3f iterate_ms=%.3f download_ms=%.3f", name, ms.upload_ms, ms.iterate_ms, ms.download_ms);
    return MGC_OK;
}

int mgc_diffuse(mgc_handle h, int niter, double kappa, double gamma, const double* spacing, int option, int keep, float* out, int64_t* out4)
{
    const char* const name = "mgc_diffuse";
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: not on a slab of a multi-GPU volume", name);
    if (keep != 0 && keep != 1) return mgc_fail(h, MGC_ERR_INVALID, "%s: keep must be 0 or 1, got %d", name, keep);
    if (!out && !keep) return mgc_fail(h, MGC_ERR_INVALID, "%s: out NULL with keep = 0", name);
    int64_t shape[3];
    for (int i = 0; i < h->ndim; ++i) shape[i] = i == h->ndim - 1 ? h->L.dx : (i == h->ndim - 2 ? h->L.dy : h->L.dz);
    MgcDiffuse P;
    int64_t dims[3];
    { const int rc = mgc_ad_args(h, name, h->ndim, shape, niter, kappa, gamma, spacing, option, &P, dims); if (rc) return rc; }
    const void* image = nullptr;
    int dtype = 0;
    if (!mgc_binned_image(h, &image, &dtype)) return mgc_fail(h, MGC_ERR_STATE, "%s: the handle holds no feature image (mgc_set_feature_image) and no boundary image (mgc_set_boundary)", name);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_(name);
    const size_t fbytes = (size_t)h->nvox * sizeof(float);
    /* not MgcBlocks: with keep = 1 one of the two stays with the handle */
    float* buf[2] = {nullptr, nullptr};
    hipError_t e = mgc_dmalloc((void**)&buf[0], fbytes);
    if (e == hipSuccess && niter > 1) e = mgc_dmalloc((void**)&buf[1], fbytes);
    MgcAdTimes ms;
    int64_t bricks = 0;
    float* result = nullptr;
    if (e == hipSuccess) e = mgc_ad_run(h->stream, dims, P, image, dtype, niter, buf, &result, &bricks, &ms.iterate_ms);
    auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess && out) e = mgc_staged_copy(h, result, out, fbytes, false);
    ms.download_ms = mgc_ms_since(t0);
    (void)hipStreamSynchronize(h->stream);
    if (e != hipSuccess || !keep) {
        (void)mgc_dfree(buf[0]);
        (void)mgc_dfree(buf[1]);
        if (e != hipSuccess) return mgc_hip_fail(h, name, e);
    } else {
        /* the result is the feature image from here on, kept and counted the way mgc_upload keeps one */
        (void)mgc_dfree(result == buf[0] ? buf[1] : buf[0]);
        size_t& cap = h->buf_cap[(const void*)&h->d_feat];
        if (h->d_feat) { (void)mgc_dfree(h->d_feat); h->device_bytes -= (int64_t)cap; }
        h->d_feat = result;
        h->feat_dtype = MGC_F32;
        cap = fbytes;
        h->device_bytes += (int64_t)fbytes;
    }
    if (out4) { out4[0] = niter; out4[1] = bricks; out4[2] = 0; out4[3] = 0; }
    (void)mgc_fail(h, MGC_OK, "%s: upload_ms=%.3f iterate_ms=%.3f download_ms=%.3f", name, ms.upload_ms, ms.iterate_ms, ms.download_ms);
    return MGC_OK;
}

} /* extern "C" */
