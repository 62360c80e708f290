/*
 * mgc_binned_driver.inl -- the host side of the binned regional term: mgc_set_feature_image, mgc_marker_histograms,
 * mgc_add_tweights_binned and mgc_update_tweights_binned.  Included ONCE, at the end of mgc_kernels.hip behind
 * mgc_reach_driver.inl: the kernels of mgc_binned_ops.inl come in here, behind the kernels of the solve, which keep their places
 * in the code object ("Headline check").
 *
 * The two table calls leave the store of mgc_tweight_ops.inl exactly as mgc_add_tweights / mgc_update_tweights of the expanded
 * arrays would: they go through mgc_tw_commit as those calls do and differ in the kernel that fills the planes.  Every check
 * comes before the first write.
 */
#include "mgc_binned_ops.inl"

/* the image the binned calls read: the feature image where one is set, else the boundary term's; false where there is neither */
static bool mgc_binned_image(mgc_handle h, const void** image, int* dtype)
{
    if (h->d_feat) { *image = h->d_feat; *dtype = h->feat_dtype; return true; }
    if (h->d_image) { *image = h->d_image; *dtype = h->img_dtype; return true; }
    return false;
}

/* A float image must be finite: checked on the device before the first write of a call.  MGC_OK (an integer image at once), or
 * the refusal that names the lowest flat index of a value that is not; `must`: its last words, which differ from call to call. */
static int mgc_float_image_check(mgc_handle h, const char* what, const void* image, int dtype, const char* must)
{
    if (dtype != MGC_F32 && dtype != MGC_F64) return MGC_OK;
    unsigned long long first = MGC_BINNED_NONE;
    const hipError_t e = mgc_first_offender(h, [&](unsigned long long* d_first) {
        const int64_t wgs = ((h->nvox + 1) / 2 + 255) / 256;
        const unsigned grid = (unsigned)(wgs < 4096 ? wgs : 4096);
        if (dtype == MGC_F32) hipLaunchKernelGGL((k_binned_check<float>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const float*)image, d_first);
        else hipLaunchKernelGGL((k_binned_check<double>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const double*)image, d_first);
    }, &first);
    MGC_HIP(h, e);
    if (first == MGC_BINNED_NONE) return MGC_OK;
    double v = 0.0;
    MGC_HIP(h, mgc_fetch_value(image, dtype, (int64_t)first, &v));
    return mgc_fail(h, MGC_ERR_INVALID, "%s: image[%lld] = %g: %s", what, (long long)first, v, must);
}

template <class T>
static void mgc_binned_expand(mgc_handle h, unsigned grid, bool fresh, const void* image, int64_t nbins, double lo, double width, const double* tables,
                              double* store, double* share, unsigned long long* changed)
{
    if (fresh) hipLaunchKernelGGL((k_tw_binned<T, true>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const T*)image, nbins, lo, width, tables, tables + nbins, store, share, changed);
    else hipLaunchKernelGGL((k_tw_binned<T, false>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const T*)image, nbins, lo, width, tables, tables + nbins, store, share, changed);
}

/* mgc_add_tweights_binned (update false) and mgc_update_tweights_binned (update true) */
static int mgc_binned_tweights(mgc_handle h, const char* what, bool update, int64_t nbins, double lo, double width, const double* source_table,
                               const double* sink_table)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: not on a slab of a multi-GPU volume", what);
    if (update) { const int rc = mgc_update_check(h, what); if (rc) return rc; }
    {
        char msg[256];
        if (mgc_binned_check(nbins, lo, width, source_table, sink_table, nullptr, nullptr, msg, sizeof(msg)) != MGC_BINNED_OK)
            return mgc_fail(h, MGC_ERR_INVALID, "%s: %s", what, msg);
    }
    const void* image = nullptr;
    int dtype = 0;
    if (!mgc_binned_image(h, &image, &dtype)) return mgc_fail(h, MGC_ERR_STATE, "%s: the handle holds no feature image (mgc_set_feature_image) and no boundary image (mgc_set_boundary)", what);
    if (h->d_tr_in && !h->tw_store) return mgc_fail(h, MGC_ERR_STATE, "%s: the handle's explicit t-links came from mgc_set_tweights_merged (mgc_clear_tweights first)", what);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_(what);
    auto t0 = std::chrono::steady_clock::now();
    { const int rc = mgc_float_image_check(h, what, image, dtype, "the feature image must be finite"); if (rc) return rc; }
    const double check_ms = mgc_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    /* what can fail for want of memory comes first: the two tables, then (mgc_tw_commit) the store of a handle that has none */
    MgcBlocks pool;
    double* const d_tables = (double*)pool.get((size_t)(2 * nbins) * sizeof(double));
    MGC_HIP(h, pool.err);
    MgcTwTimes ms;
    ms.fill_ms = mgc_ms_since(t0);
    const int rc = mgc_tw_commit(h, what, update ? MGC_TW_WARM : MGC_TW_COLD, pool, [&](double* store, double* share, unsigned long long* changed) {
        hipError_t e = hipMemcpyAsync(d_tables, source_table, (size_t)nbins * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tables + nbins, sink_table, (size_t)nbins * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return e;
        const int64_t wgs = ((h->nvox + 1) / 2 + 255) / 256;
        const unsigned grid = (unsigned)(wgs < 8192 ? wgs : 8192);
        switch (dtype) {
        case MGC_U8: mgc_binned_expand<uint8_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_I8: mgc_binned_expand<int8_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_U16: mgc_binned_expand<uint16_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_I16: mgc_binned_expand<int16_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_U32: mgc_binned_expand<uint32_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_I32: mgc_binned_expand<int32_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_U64: mgc_binned_expand<uint64_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_I64: mgc_binned_expand<int64_t>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        case MGC_F32: mgc_binned_expand<float>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        default: mgc_binned_expand<double>(h, grid, update, image, nbins, lo, width, d_tables, store, share, changed); break;
        }
        return hipGetLastError();
    }, &ms);
    if (rc) return rc;
    /* no error: the note says where the time of this call went (tools/gpu_histogram_term.py records it) */
    if (!update) (void)mgc_fail(h, MGC_OK, "%s: check_ms=%.3f expand_ms=%.3f flow_const_ms=%.3f", what, check_ms, ms.fill_ms, ms.flow_const_ms);
    else (void)mgc_fail(h, MGC_OK, "%s: check_ms=%.3f expand_ms=%.3f flow_const_ms=%.3f fold_ms=%.3f", what, check_ms, ms.fill_ms, ms.flow_const_ms, ms.fold_ms);
    return MGC_OK;
}

extern "C" {

int mgc_set_feature_image(mgc_handle h, const void* image, int dtype)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "mgc_set_feature_image: not on a slab of a multi-GPU volume");
    MGC_HIP(h, hipSetDevice(h->device));
    if (!image) {
        if (h->d_feat) {
            MGC_HIP(h, hipStreamSynchronize(h->stream));
            (void)mgc_dfree(h->d_feat);
            size_t& cap = h->buf_cap[(const void*)&h->d_feat];
            h->device_bytes -= (int64_t)cap;
            cap = 0;
            h->d_feat = nullptr;
        }
        return MGC_OK;
    }
    const size_t es = mgc_dtype_size(dtype);
    if (!es) return mgc_fail(h, MGC_ERR_INVALID, "mgc_set_feature_image: bad dtype %d", dtype);
    const int rc = mgc_upload(h, &h->d_feat, image, (size_t)h->nvox * es);
    if (rc == MGC_OK) h->feat_dtype = dtype;
    return rc;
}

int mgc_marker_histograms(mgc_handle h, int64_t nbins, double lo, double width, int64_t* fg_hist, int64_t* bg_hist, int64_t* out4)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "mgc_marker_histograms: not on a slab of a multi-GPU volume");
    {
        char msg[256];
        if (mgc_binned_check_binning(nbins, lo, width, msg, sizeof(msg)) != MGC_BINNED_OK) return mgc_fail(h, MGC_ERR_INVALID, "mgc_marker_histograms: %s", msg);
    }
    if (!fg_hist || !bg_hist) return mgc_fail(h, MGC_ERR_INVALID, "mgc_marker_histograms: fg_hist / bg_hist NULL");
    const void* image = nullptr;
    int dtype = 0;
    if (!mgc_binned_image(h, &image, &dtype)) return mgc_fail(h, MGC_ERR_STATE, "mgc_marker_histograms: the handle holds no feature image (mgc_set_feature_image) and no boundary image (mgc_set_boundary)");
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_marker_histograms");
    /* the block of the call: 2 * nbins counts, the four totals, the first offender */
    const size_t words = (size_t)(2 * nbins) + 5;
    std::vector<unsigned long long> host(words, 0ull);
    host[words - 1] = MGC_BINNED_NONE;
    if (h->d_fg || h->d_bg) {
        unsigned long long* d_block = nullptr;
        MGC_HIP(h, mgc_dmalloc((void**)&d_block, words * sizeof(unsigned long long)));
        hipError_t e = hipMemsetAsync(d_block, 0, (words - 1) * sizeof(unsigned long long), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_block + words - 1, 0xff, sizeof(unsigned long long), h->stream);
        if (e == hipSuccess) {
            const int64_t wgs = (h->nvox / 16 + 255) / 256;
            const unsigned grid = (unsigned)(wgs < 1 ? 1 : (wgs < 2048 ? wgs : 2048));
            const int is_float = dtype == MGC_F32 || dtype == MGC_F64;
            if (nbins <= MGC_BINNED_LDS_MAX)
                hipLaunchKernelGGL((k_marker_hist<true>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const uint8_t*)h->d_fg, (const uint8_t*)h->d_bg, image, dtype, is_float,
                                   nbins, lo, width, d_block, d_block + 2 * nbins, d_block + 2 * nbins + 4);
            else
                hipLaunchKernelGGL((k_marker_hist<false>), dim3(grid), dim3(256), 0, h->stream, h->nvox, (const uint8_t*)h->d_fg, (const uint8_t*)h->d_bg, image, dtype, is_float,
                                   nbins, lo, width, d_block, d_block + 2 * nbins, d_block + 2 * nbins + 4);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_block, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        (void)mgc_dfree(d_block);
        MGC_HIP(h, e);
        MGC_HIP(h, e2);
    }
    if (host[words - 1] != MGC_BINNED_NONE) {
        const int64_t id = (int64_t)host[words - 1];
        double v = 0.0;
        MGC_HIP(h, mgc_fetch_value(image, dtype, id, &v));
        return mgc_fail(h, MGC_ERR_INVALID, "mgc_marker_histograms: image[%lld] = %g under a marker: the feature image must be finite", (long long)id, v);
    }
    for (int64_t b = 0; b < nbins; ++b) { fg_hist[b] = (int64_t)host[(size_t)b]; bg_hist[b] = (int64_t)host[(size_t)(nbins + b)]; }
    if (out4)
        for (int k = 0; k < 4; ++k) out4[k] = (int64_t)host[(size_t)(2 * nbins + k)];
    return MGC_OK;
}

int mgc_add_tweights_binned(mgc_handle h, int64_t nbins, double lo, double width, const double* source_table, const double* sink_table)
{
    return mgc_binned_tweights(h, "mgc_add_tweights_binned", false, nbins, lo, width, source_table, sink_table);
}

int mgc_update_tweights_binned(mgc_handle h, int64_t nbins, double lo, double width, const double* source_table, const double* sink_table)
{
    return mgc_binned_tweights(h, "mgc_update_tweights_binned", true, nbins, lo, width, source_table, sink_table);
}

} /* extern "C" */
