/*
 * mgc_geo_driver.inl -- the host side of mgc_geodesic_distance, mgc_add_tweights_geodesic and mgc_update_tweights_geodesic.
 * Included ONCE, as the last of the drivers at the end of mgc_kernels.hip: the kernels of mgc_geo_ops.inl come in here, behind every
 * other kernel of the library, so that the kernels before them keep their places in the code object ("Headline check").
 * Every check comes before the first write.  mgc_geodesic_distance leaves the handle as it was: it reads the image and the marker
 * planes, and every block it uses comes from the pool and goes back before it returns (MgcBlocks, mgc_blocks_end).  The two calls of
 * the term leave the t-link store exactly as mgc_add_tweights / mgc_update_tweights of the expanded arrays would: they go through
 * mgc_tw_commit as those calls do (and mgc_binned_tweights) and differ in what fills the planes; the warm form differs in one more
 * thing, the label snapshot of mgc_labels_delta, which it keeps as mgc_edit_tweights does.  No field of the handle is new.
 */
#include "mgc_geo_ops.inl"

/* the arguments the three calls share, checked: sp and the table of step lengths come back */
static int mgc_geo_args(mgc_handle h, const char* name, int full, double gamma, double step, const double* spacing, MgcGeoSteps* S)
{
    const double top = 1.7976931348623157e308;
    if (full != 0 && full != 1) return mgc_fail(h, MGC_ERR_INVALID, "%s: full must be 0 (face neighbourhood) or 1 (full neighbourhood), got %d", name, full);
    if (!(gamma >= 0.0) || !(gamma <= top)) return mgc_fail(h, MGC_ERR_INVALID, "%s: gamma = %g: gamma must be finite and not negative", name, gamma);
    if (!(step >= 0.0) || !(step <= top)) return mgc_fail(h, MGC_ERR_INVALID, "%s: step = %g: step must be finite and not negative", name, step);
    double sp[3];
    int bad = 0;
    if (!mgc_edt_spacing(h, spacing, sp, &bad)) return mgc_fail(h, MGC_ERR_INVALID, "%s: spacing[%d] = %g: the spacing must be finite and positive", name, bad, spacing[bad]);
    mgc_geo_steps(sp, step, S);
    return MGC_OK;
}

/* The image the arcs read (that of mgc_marker_histograms; none at gamma == 0), and a float image checked on the device: MGC_OK, or
 * the refusal that names the lowest flat index of a value that is not finite. */
static int mgc_geo_image(mgc_handle h, const char* name, double gamma, const void** image, int* dtype)
{
    *image = nullptr;
    *dtype = 0;
    if (gamma == 0.0) return MGC_OK;
    if (!mgc_binned_image(h, image, dtype))
        return mgc_fail(h, MGC_ERR_STATE, "%s: gamma = %g > 0 and the handle holds no feature image (mgc_set_feature_image) and no boundary image (mgc_set_boundary)", name, gamma);
    return mgc_float_image_check(h, name, *image, *dtype, "the image must be finite");
}

/* One transform: *result is a plane of nvox doubles of the pool (C order), info the eight slots of out8.  seeds: a byte plane on the
 * device or NULL (no seeds: +inf everywhere and no round runs).  A round is one launch over the tiles the round before woke; the
 * host looks at the length of the next list after every launch and stops at the round that woke nobody.  After round r every voxel
 * whose best path has at most r arcs holds its value, and a path visits a voxel once: more than nvox + 1 rounds cannot happen, and
 * *stuck says so instead of spinning. */
static hipError_t mgc_geo_transform(mgc_handle h, MgcBlocks& pool, const uint8_t* seeds, int full, double gamma, const MgcGeoSteps& S, const void* image, int dtype,
                                    double** result, unsigned long long info[8], bool* stuck)
{
    const MgcLattice& L = h->L;
    const int64_t nvox = h->nvox;
    const size_t nt = (size_t)L.ntiles;
    double* const plane = (double*)pool.get((size_t)nvox * sizeof(double));
    int32_t* const lists = (int32_t*)pool.get(2 * nt * sizeof(int32_t));
    uint32_t* const flags = (uint32_t*)pool.get(2 * nt * sizeof(uint32_t));
    unsigned long long* const words = (unsigned long long*)pool.get(9 * sizeof(unsigned long long)); /* info[8], then the two lengths */
    *result = plane;
    *stuck = false;
    for (int k = 0; k < 8; ++k) info[k] = 0ull;
    if (pool.err != hipSuccess) return pool.err;
    MgcGeoLists W;
    W.list[0] = lists; W.list[1] = lists + nt;
    W.flag[0] = flags; W.flag[1] = flags + nt;
    W.info = words;
    W.len = (uint32_t*)(words + 8);
    hipError_t e = hipMemsetAsync(flags, 0, 2 * nt * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(words, 0, 9 * sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_geo_init<0>, dim3(mgc_edt_grid((nvox + 255) / 256, 65536)), dim3(256), 0, h->stream, L, seeds, full, plane, W);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t len[2] = {0u, 0u};
    if ((e = hipMemcpyAsync(len, W.len, sizeof(len), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    int64_t rounds = 0, visits = 0;
    const int64_t max_rounds = nvox + 1;
    for (int cur = 0; len[cur] > 0u; cur ^= 1) {
        if (rounds >= max_rounds) { *stuck = true; break; }
        const int nxt = cur ^ 1;
        if ((e = hipMemsetAsync(W.len + nxt, 0, sizeof(uint32_t), h->stream)) != hipSuccess) return e;
        if (full) hipLaunchKernelGGL(k_geo_tile<true>, dim3(len[cur]), dim3(MGC_TV), 0, h->stream, L, S, gamma, image, dtype, plane, W, cur);
        else hipLaunchKernelGGL(k_geo_tile<false>, dim3(len[cur]), dim3(MGC_TV), 0, h->stream, L, S, gamma, image, dtype, plane, W, cur);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&len[nxt], W.len + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
        visits += (int64_t)len[cur];
        ++rounds;
    }
    hipLaunchKernelGGL(k_geo_finite<0>, dim3(mgc_edt_grid((nvox + 255) / 256, 16384)), dim3(256), 0, h->stream, (const double*)plane, nvox, words);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(info, words, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    info[MGC_GEO_ROUNDS] = (unsigned long long)rounds;
    info[MGC_GEO_VISITS] = (unsigned long long)visits;
    return hipSuccess;
}

template <bool FRESH>
static void mgc_geo_expand(mgc_handle h, const double* df, const double* db, double lam, double* store, double* share, unsigned long long* changed)
{
    const int64_t wgs = ((h->nvox + 1) / 2 + 255) / 256;
    const unsigned grid = (unsigned)(wgs < 8192 ? wgs : 8192);
    hipLaunchKernelGGL((k_tw_geodesic<FRESH>), dim3(grid), dim3(256), 0, h->stream, h->nvox, df, db, lam, store, share, changed);
}

/* mgc_add_tweights_geodesic (update false) and mgc_update_tweights_geodesic (update true): mgc_binned_tweights with two transforms
 * in the place of the two tables */
static int mgc_geo_tweights(mgc_handle h, const char* what, bool update, int full, double gamma, double step, const double* spacing, double lam)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: not on a slab of a multi-GPU volume", what);
    if (update) { const int rc = mgc_update_check(h, what); if (rc) return rc; }
    MgcGeoSteps S;
    { const int rc = mgc_geo_args(h, what, full, gamma, step, spacing, &S); if (rc) return rc; }
    if (!(lam >= 0.0) || !(lam <= 1.7976931348623157e308)) return mgc_fail(h, MGC_ERR_INVALID, "%s: lam = %g: lam must be finite and not negative", what, lam);
    if (h->d_tr_in && !h->tw_store) return mgc_fail(h, MGC_ERR_STATE, "%s: the handle's explicit t-links came from mgc_set_tweights_merged (mgc_clear_tweights first)", what);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_(what);
    auto t0 = std::chrono::steady_clock::now();
    const void* image = nullptr;
    int dtype = 0;
    { const int rc = mgc_geo_image(h, what, gamma, &image, &dtype); if (rc) return rc; }
    /* the two planes live for this call only; nothing of the handle has changed while they are computed */
    MgcBlocks pool;
    double* dist[2] = {nullptr, nullptr};
    unsigned long long info[2][8];
    bool stuck = false;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess && !stuck; ++k)
        e = mgc_geo_transform(h, pool, (const uint8_t*)(k == 0 ? h->d_fg : h->d_bg), full, gamma, S, image, dtype, &dist[k], info[k], &stuck);
    if (e != hipSuccess || stuck) {
        const int rc = mgc_blocks_end(h, pool, e, what);
        return rc != MGC_OK ? rc : mgc_fail(h, MGC_ERR_HIP, "%s: the transform did not reach its fixpoint within %lld rounds", what, (long long)(h->nvox + 1));
    }
    const double transform_ms = mgc_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    /* What can fail for want of memory comes first: the label snapshot of a finished cut, then (mgc_tw_commit) the store of a handle
       that has none.  The refit follows a stroke, and the caller asks which voxels the round changed: unlike mgc_update_tweights the
       warm form keeps the snapshot of mgc_labels_delta, the way mgc_edit_tweights does. */
    if (update) { const int rc = mgc_snapshot_reserve(h); if (rc) return rc; }
    MgcTwTimes ms;
    ms.fill_ms = mgc_ms_since(t0);
    const int rc = mgc_tw_commit(h, what, update ? MGC_TW_WARM_KEEP : MGC_TW_COLD, pool, [&](double* store, double* share, unsigned long long* changed) {
        if (update) mgc_geo_expand<true>(h, dist[0], dist[1], lam, store, share, changed);
        else mgc_geo_expand<false>(h, dist[0], dist[1], lam, store, share, nullptr);
        return hipGetLastError();
    }, &ms);
    if (rc) return rc;
    const long long rounds[2] = {(long long)info[0][MGC_GEO_ROUNDS], (long long)info[1][MGC_GEO_ROUNDS]};
    const long long visits[2] = {(long long)info[0][MGC_GEO_VISITS], (long long)info[1][MGC_GEO_VISITS]};
    /* no error: the note says where the time of this call went (tools/gpu_geodesic.py records it) */
    if (!update)
        (void)mgc_fail(h, MGC_OK, "%s: transform_ms=%.3f expand_ms=%.3f flow_const_ms=%.3f rounds_fg=%lld rounds_bg=%lld visits_fg=%lld visits_bg=%lld", what, transform_ms, ms.fill_ms,
                       ms.flow_const_ms, rounds[0], rounds[1], visits[0], visits[1]);
    else
        (void)mgc_fail(h, MGC_OK, "%s: transform_ms=%.3f expand_ms=%.3f flow_const_ms=%.3f fold_ms=%.3f rounds_fg=%lld rounds_bg=%lld visits_fg=%lld visits_bg=%lld", what, transform_ms,
                       ms.fill_ms, ms.flow_const_ms, ms.fold_ms, rounds[0], rounds[1], visits[0], visits[1]);
    return MGC_OK;
}

extern "C" {

int mgc_geodesic_distance(mgc_handle h, const uint8_t* seeds, int source, int full, double gamma, double step, const double* spacing, double* out, int64_t* out8)
{
    if (!h) return MGC_ERR_INVALID;
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "mgc_geodesic_distance: not on a slab of a multi-GPU volume");
    if (source < 0 || source > 2) return mgc_fail(h, MGC_ERR_INVALID, "mgc_geodesic_distance: source must be 0 (a plane of the caller's), 1 (the foreground markers) or 2 (the background markers), got %d", source);
    if (source == 0 && !seeds) return mgc_fail(h, MGC_ERR_INVALID, "mgc_geodesic_distance: seeds NULL with source 0");
    if (source != 0 && seeds) return mgc_fail(h, MGC_ERR_INVALID, "mgc_geodesic_distance: seeds given with source %d (the markers are read where they lie)", source);
    MgcGeoSteps S;
    { const int rc = mgc_geo_args(h, "mgc_geodesic_distance", full, gamma, step, spacing, &S); if (rc) return rc; }
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_geodesic_distance");
    const void* image = nullptr;
    int dtype = 0;
    { const int rc = mgc_geo_image(h, "mgc_geodesic_distance", gamma, &image, &dtype); if (rc) return rc; }
    MgcBlocks pool;
    const uint8_t* d_seeds = (const uint8_t*)(source == 1 ? h->d_fg : h->d_bg);
    hipError_t e = hipSuccess;
    if (source == 0) e = mgc_edt_plane(h, pool, seeds, &d_seeds);
    double* plane = nullptr;
    unsigned long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool stuck = false;
    if (e == hipSuccess) e = mgc_geo_transform(h, pool, d_seeds, full, gamma, S, image, dtype, &plane, info, &stuck);
    if (e == hipSuccess && !stuck && out) e = mgc_staged_copy(h, plane, out, (size_t)h->nvox * sizeof(double), false);
    const int rc = mgc_blocks_end(h, pool, e, "mgc_geodesic_distance");
    if (rc != MGC_OK) return rc;
    if (stuck) return mgc_fail(h, MGC_ERR_HIP, "mgc_geodesic_distance: the transform did not reach its fixpoint within %lld rounds", (long long)(h->nvox + 1));
    if (out8)
        for (int k = 0; k < 8; ++k) out8[k] = (int64_t)info[k];
    return MGC_OK;
}

int mgc_add_tweights_geodesic(mgc_handle h, int full, double gamma, double step, const double* spacing, double lam)
{
    return mgc_geo_tweights(h, "mgc_add_tweights_geodesic", false, full, gamma, step, spacing, lam);
}

int mgc_update_tweights_geodesic(mgc_handle h, int full, double gamma, double step, const double* spacing, double lam)
{
    return mgc_geo_tweights(h, "mgc_update_tweights_geodesic", true, full, gamma, step, spacing, lam);
}

} /* extern "C" */
