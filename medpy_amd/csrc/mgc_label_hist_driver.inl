/*
 * mgc_label_hist_driver.inl -- the host side of mgc_label_histograms: the histograms of the feature image over every
 * voxel, split by the labels of the current cut or by a label plane of the caller's.  Included ONCE, at the end of
 * mgc_kernels.hip behind mgc_binned_driver.inl: the kernel of mgc_label_hist_ops.inl comes in here, behind those, so that
 * the kernels before it keep their places in the code object ("Headline check").  Every check comes before the first
 * write, and the call leaves the handle as it was: it reads the image and the labels, and what it allocates goes back to the pool
 * before it returns.
 */
#include "mgc_label_hist_ops.inl"

template <class T>
static void mgc_label_hist_launch(mgc_handle h, unsigned grid, const uint8_t* labels, const void* image, int64_t nbins, double lo, double width,
                                  unsigned long long* d_block)
{
    unsigned long long* const out4 = d_block + 2 * nbins;
    if (nbins <= MGC_BINNED_LDS_MAX)
        hipLaunchKernelGGL((k_label_hist<T, true>), dim3(grid), dim3(256), (size_t)(2 * nbins) * sizeof(unsigned int), h->stream, h->nvox, labels, (const T*)image, nbins, lo, width,
                           d_block, out4, out4 + 4);
    else
        hipLaunchKernelGGL((k_label_hist<T, false>), dim3(grid), dim3(256), 0, h->stream, h->nvox, labels, (const T*)image, nbins, lo, width, d_block, out4, out4 + 4);
}

extern "C" {

int mgc_label_histograms(mgc_handle h, const uint8_t* labels, int64_t nbins, double lo, double width, int64_t* fg_hist, int64_t* bg_hist, int64_t* out4)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "mgc_label_histograms: not on a slab of a multi-GPU volume");
    {
        char msg[256];
        if (mgc_binned_check_binning(nbins, lo, width, msg, sizeof(msg)) != MGC_BINNED_OK) return mgc_fail(h, MGC_ERR_INVALID, "mgc_label_histograms: %s", msg);
    }
    if (!fg_hist || !bg_hist) return mgc_fail(h, MGC_ERR_INVALID, "mgc_label_histograms: fg_hist / bg_hist NULL");
    const void* image = nullptr;
    int dtype = 0;
    if (!mgc_binned_image(h, &image, &dtype)) return mgc_fail(h, MGC_ERR_STATE, "mgc_label_histograms: the handle holds no feature image (mgc_set_feature_image) and no boundary image (mgc_set_boundary)");
    if (!labels) { /* the labels of the current cut: only where the handle holds one */
        const int rc = mgc_reach_check_state(h, "mgc_label_histograms (labels NULL)", "labels");
        if (rc != MGC_OK) return rc;
    }
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_label_histograms");
    /* the block of the call: 2 * nbins counts, the four totals, the first offender; a caller's plane goes into a block of its own */
    const size_t words = (size_t)(2 * nbins) + 5;
    std::vector<unsigned long long> host(words, 0ull);
    unsigned long long* d_block = nullptr;
    uint8_t* d_plane = nullptr;
    MGC_HIP(h, mgc_dmalloc((void**)&d_block, words * sizeof(unsigned long long)));
    hipError_t e = hipSuccess;
    if (labels) {
        e = mgc_dmalloc((void**)&d_plane, (size_t)h->nvox);
        if (e == hipSuccess) e = mgc_staged_copy(h, d_plane, const_cast<uint8_t*>(labels), (size_t)h->nvox, true);
    }
    if (e == hipSuccess) e = hipMemsetAsync(d_block, 0, (words - 1) * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_block + words - 1, 0xff, sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) {
        const uint8_t* const plane = labels ? d_plane : h->d_labels;
        const int64_t wgs = (h->nvox / MGC_LH_GROUP + 255) / 256;
        const unsigned grid = (unsigned)(wgs < 1 ? 1 : (wgs < 2048 ? wgs : 2048));
        switch (dtype) {
        case MGC_U8: mgc_label_hist_launch<uint8_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_I8: mgc_label_hist_launch<int8_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_U16: mgc_label_hist_launch<uint16_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_I16: mgc_label_hist_launch<int16_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_U32: mgc_label_hist_launch<uint32_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_I32: mgc_label_hist_launch<int32_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_U64: mgc_label_hist_launch<uint64_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_I64: mgc_label_hist_launch<int64_t>(h, grid, plane, image, nbins, lo, width, d_block); break;
        case MGC_F32: mgc_label_hist_launch<float>(h, grid, plane, image, nbins, lo, width, d_block); break;
        default: mgc_label_hist_launch<double>(h, grid, plane, image, nbins, lo, width, d_block); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_block, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    (void)mgc_dfree(d_block);
    if (d_plane) (void)mgc_dfree(d_plane);
    MGC_HIP(h, e);
    MGC_HIP(h, e2);
    if (host[words - 1] != MGC_BINNED_NONE) {
        const int64_t id = (int64_t)host[words - 1];
        double v = 0.0;
        MGC_HIP(h, mgc_fetch_value(image, dtype, id, &v));
        return mgc_fail(h, MGC_ERR_INVALID, "mgc_label_histograms: image[%lld] = %g: the feature image must be finite", (long long)id, v);
    }
    for (int64_t b = 0; b < nbins; ++b) { fg_hist[b] = (int64_t)host[(size_t)b]; bg_hist[b] = (int64_t)host[(size_t)(nbins + b)]; }
    if (out4)
        for (int k = 0; k < 4; ++k) out4[k] = (int64_t)host[(size_t)(2 * nbins + k)];
    return MGC_OK;
}

} /* extern "C" */
