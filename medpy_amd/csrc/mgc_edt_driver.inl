/*
 * mgc_edt_driver.inl -- the host side of mgc_distance_transform, mgc_surface_distances and mgc_overlap_counts.  Included
 * ONCE, at the end of mgc_kernels.hip behind mgc_cc_driver.inl: the kernels of mgc_edt_ops.inl come in here, behind those,
 * so that the kernels before them keep their places in the code object ("Headline check").  Every check comes before the
 * first write, and a call leaves the handle as it was: it reads the labels of the current cut or planes of the caller's, and every
 * block it uses comes from the pool and goes back before it returns (MgcBlocks, mgc_blocks_end).  No field of the handle is new.
 */
#include "mgc_edt_ops.inl"

static unsigned mgc_edt_grid(int64_t blocks, int64_t most)
{
    return (unsigned)(blocks < 1 ? 1 : (blocks < most ? blocks : most));
}

/* what the three entry points ask of the handle before anything is written */
static int mgc_edt_check(mgc_handle h, const char* name, const uint8_t* plane)
{
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: not on a slab of a multi-GPU volume", name);
    if (!plane) {
        char who[96];
        snprintf(who, sizeof(who), "%s (plane NULL)", name);
        return mgc_reach_check_state(h, who, "labels");
    }
    return MGC_OK;
}

/* sp[0..2] = the spacing of (z, y, x): the ndim values of the caller for the last ndim axes, 1 elsewhere.  false: a value is not finite and positive */
static bool mgc_edt_spacing(mgc_handle h, const double* spacing, double sp[3], int* bad)
{
    sp[0] = sp[1] = sp[2] = 1.0;
    if (!spacing) return true;
    for (int k = 0; k < h->ndim; ++k) {
        const double v = spacing[k];
        if (!(v > 0.0) || !(v <= 1.7976931348623157e308)) {
            *bad = k;
            return false;
        }
        sp[3 - h->ndim + k] = v;
    }
    return true;
}

/* the device plane of a call: the labels of the current cut where they lie, or a caller's plane in a block of the call */
static hipError_t mgc_edt_plane(mgc_handle h, MgcBlocks& pool, const uint8_t* host, const uint8_t** plane)
{
    if (!host) {
        *plane = h->d_labels;
        return pool.err;
    }
    uint8_t* d = (uint8_t*)pool.get((size_t)h->nvox);
    *plane = d;
    if (pool.err != hipSuccess) return pool.err;
    return mgc_staged_copy(h, d, const_cast<uint8_t*>(host), (size_t)h->nvox, true);
}

/* tot[0..3] = voxels of class tp, fp, fn, tn of p against q (q NULL: all zero); *off (or NULL): the scanned counts of p, nseg + 1 words */
static hipError_t mgc_edt_count(mgc_handle h, MgcBlocks& pool, const uint8_t* p, const uint8_t* q, unsigned long long** off, unsigned long long tot[4])
{
    const int64_t nseg = (h->nvox + MGC_EDT_COUNT_SEG - 1) / MGC_EDT_COUNT_SEG;
    unsigned long long* const cnt = (unsigned long long*)pool.get((size_t)(nseg + 1) * sizeof(unsigned long long));
    unsigned long long* const part = (unsigned long long*)pool.get((size_t)(4 * nseg) * sizeof(unsigned long long));
    unsigned long long* const d_tot = (unsigned long long*)pool.get(4 * sizeof(unsigned long long));
    if (pool.err != hipSuccess) return pool.err;
    hipLaunchKernelGGL(k_edt_count<0>, dim3(mgc_edt_grid((nseg + 3) / 4, 16384)), dim3(256), 0, h->stream, p, q, h->nvox, nseg, cnt, part);
    if (off) hipLaunchKernelGGL(k_labels_delta_scan, dim3(1), dim3(MGC_SCAN_THREADS), 0, h->stream, cnt, nseg);
    hipLaunchKernelGGL(k_edt_reduce<0>, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)part, nseg, d_tot);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (off) *off = cnt;
    return e;
}

/* The transform of `plane` with the seeds of `side`, nseeds of them: *result is a plane of nvox doubles of the pool.  The last axis
 * from the bytes, then y and z where the volume has them (an axis of extent 1 adds fl(g + 0) = g: nothing to do); *long_lines grows
 * by the lines that were too long for a panel. */
static hipError_t mgc_edt_transform(mgc_handle h, MgcBlocks& pool, const uint8_t* plane, int side, const double sp[3], int64_t nseeds, double** result, int64_t* long_lines)
{
    const MgcLattice& L = h->L;
    const int64_t nvox = h->nvox;
    double* g = (double*)pool.get((size_t)nvox * sizeof(double));
    double* tmp = nullptr;
    *result = g;
    if (pool.err != hipSuccess) return pool.err;
    const unsigned g_vox = mgc_edt_grid((nvox + 255) / 256, 65536);
    if (nseeds == 0) {
        hipLaunchKernelGGL(k_edt_fill<0>, dim3(g_vox), dim3(256), 0, h->stream, g, nvox, MGC_EDT_INF);
        return hipGetLastError();
    }
    const int64_t rows = L.dz * L.dy;
    hipLaunchKernelGGL(k_edt_rows<0>, dim3(mgc_edt_grid((rows + 3) / 4, 65536)), dim3(256), 0, h->stream, plane, side, rows, L.dx, sp[2], g);
    const int64_t line[2] = {L.dy, L.dz}, stride[2] = {L.dx, L.dy * L.dx};
    const double s[2] = {sp[1], sp[0]};
    for (int a = 0; a < 2; ++a) {
        const int64_t n = line[a];
        if (n <= 1) continue;
        if (n <= MGC_EDT_PANEL_LINE) {
            const int64_t ppo = (stride[a] + MGC_EDT_PANEL_COLS - 1) / MGC_EDT_PANEL_COLS, npanels = (nvox / (n * stride[a])) * ppo;
            hipLaunchKernelGGL(k_edt_panels<0>, dim3(mgc_edt_grid(npanels, 65536)), dim3(256), (size_t)n * MGC_EDT_PANEL_COLS * sizeof(double), h->stream, g, n, stride[a], npanels, ppo, s[a]);
        } else {
            if (!tmp) tmp = (double*)pool.get((size_t)nvox * sizeof(double));
            if (pool.err != hipSuccess) return pool.err;
            hipLaunchKernelGGL(k_edt_long<0>, dim3(g_vox), dim3(256), 0, h->stream, (const double*)g, tmp, nvox, n, stride[a], s[a]);
            double* const t = g;
            g = tmp;
            tmp = t;
            *long_lines += nvox / n;
        }
    }
    *result = g;
    return hipGetLastError();
}

extern "C" {

int mgc_distance_transform(mgc_handle h, const uint8_t* plane, int side, const double* spacing, double* out_sq, int64_t* out4)
{
    if (!h) return MGC_ERR_INVALID;
    { const int rc = mgc_edt_check(h, "mgc_distance_transform", plane); if (rc != MGC_OK) return rc; }
    if (side != 0 && side != 1) return mgc_fail(h, MGC_ERR_INVALID, "mgc_distance_transform: side must be 0 (the seeds are the zero voxels) or 1 (the non-zero ones), got %d", side);
    double sp[3];
    int bad = 0;
    if (!mgc_edt_spacing(h, spacing, sp, &bad)) return mgc_fail(h, MGC_ERR_INVALID, "mgc_distance_transform: spacing[%d] = %g: the spacing must be finite and positive", bad, spacing[bad]);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_distance_transform");
    MgcBlocks pool;
    const uint8_t* d_plane = nullptr;
    unsigned long long tot[4] = {0, 0, 0, 0};
    double* g = nullptr;
    int64_t nseeds = 0, long_lines = 0;
    hipError_t e = mgc_edt_plane(h, pool, plane, &d_plane);
    if (e == hipSuccess) e = mgc_edt_count(h, pool, d_plane, nullptr, nullptr, tot);
    if (e == hipSuccess) {
        nseeds = side ? (int64_t)(tot[0] + tot[1]) : (int64_t)(tot[2] + tot[3]);
        if (out_sq) e = mgc_edt_transform(h, pool, d_plane, side, sp, nseeds, &g, &long_lines);
    }
    if (e == hipSuccess && out_sq) e = mgc_staged_copy(h, g, out_sq, (size_t)h->nvox * sizeof(double), false);
    const int rc = mgc_blocks_end(h, pool, e, "mgc_distance_transform");
    if (rc != MGC_OK) return rc;
    if (out4) {
        out4[MGC_EDT_SEEDS] = nseeds;
        out4[MGC_EDT_LONG_LINES] = long_lines;
        out4[2] = out4[3] = 0;
    }
    return MGC_OK;
}

int mgc_surface_distances(mgc_handle h, const uint8_t* a, const uint8_t* b, int connectivity, const double* spacing, int64_t cap, double* sds_sq, int64_t* out8)
{
    if (!h) return MGC_ERR_INVALID;
    { const int rc = mgc_edt_check(h, "mgc_surface_distances", a); if (rc != MGC_OK) return rc; }
    if (!b) return mgc_fail(h, MGC_ERR_INVALID, "mgc_surface_distances: b NULL");
    if (connectivity < 1 || connectivity > h->ndim) return mgc_fail(h, MGC_ERR_INVALID, "mgc_surface_distances: connectivity must be 1 .. %d on this handle, got %d", h->ndim, connectivity);
    if (cap < 0) return mgc_fail(h, MGC_ERR_INVALID, "mgc_surface_distances: the capacity of the list must not be negative, got %lld", (long long)cap);
    if (cap > 0 && !sds_sq) return mgc_fail(h, MGC_ERR_INVALID, "mgc_surface_distances: sds_sq NULL with a capacity of %lld", (long long)cap);
    double sp[3];
    int bad = 0;
    if (!mgc_edt_spacing(h, spacing, sp, &bad)) return mgc_fail(h, MGC_ERR_INVALID, "mgc_surface_distances: spacing[%d] = %g: the spacing must be finite and positive", bad, spacing[bad]);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_surface_distances");
    MgcBlocks pool;
    const MgcLattice& L = h->L;
    const int64_t nvox = h->nvox, nseg = (nvox + MGC_EDT_COUNT_SEG - 1) / MGC_EDT_COUNT_SEG;
    const unsigned g_vox = mgc_edt_grid((nvox + 255) / 256, 65536);
    const uint8_t* d_a = nullptr;
    const uint8_t* d_b = nullptr;
    unsigned long long size[4] = {0, 0, 0, 0}, rim[4] = {0, 0, 0, 0};
    unsigned long long* off = nullptr;
    int64_t long_lines = 0;
    uint8_t* const rim_a = (uint8_t*)pool.get((size_t)nvox);
    uint8_t* const rim_b = (uint8_t*)pool.get((size_t)nvox);
    hipError_t e = pool.err;
    if (e == hipSuccess) e = mgc_edt_plane(h, pool, a, &d_a);
    if (e == hipSuccess) e = mgc_edt_plane(h, pool, b, &d_b);
    if (e == hipSuccess) e = mgc_edt_count(h, pool, d_a, d_b, nullptr, size);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_edt_border<0>, dim3(g_vox), dim3(256), 0, h->stream, d_a, L.dz, L.dy, L.dx, h->ndim, connectivity, rim_a);
        hipLaunchKernelGGL(k_edt_border<0>, dim3(g_vox), dim3(256), 0, h->stream, d_b, L.dz, L.dy, L.dx, h->ndim, connectivity, rim_b);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mgc_edt_count(h, pool, rim_a, rim_b, &off, rim);
    const int64_t n_a = (int64_t)(rim[0] + rim[1]), n_b = (int64_t)(rim[0] + rim[2]);
    const int64_t rows = n_a < cap ? n_a : cap;
    if (e == hipSuccess && rows > 0 && n_b > 0) {
        double* g = nullptr;
        e = mgc_edt_transform(h, pool, rim_b, 1, sp, n_b, &g, &long_lines);
        double* const d_out = (double*)pool.get((size_t)rows * sizeof(double));
        if (e == hipSuccess) e = pool.err;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_edt_gather<0>, dim3(mgc_edt_grid((nseg + 3) / 4, 16384)), dim3(256), 0, h->stream, (const uint8_t*)rim_a, (const double*)g, nvox, nseg, (const unsigned long long*)off, rows, d_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = mgc_staged_copy(h, d_out, sds_sq, (size_t)rows * sizeof(double), false);
    }
    const int rc = mgc_blocks_end(h, pool, e, "mgc_surface_distances");
    if (rc != MGC_OK) return rc;
    if (out8) {
        out8[MGC_SD_BORDER_A] = n_a;
        out8[MGC_SD_BORDER_B] = n_b;
        out8[MGC_SD_SIZE_A] = (int64_t)(size[0] + size[1]);
        out8[MGC_SD_SIZE_B] = (int64_t)(size[0] + size[2]);
        out8[MGC_SD_LONG_LINES] = long_lines;
        out8[5] = out8[6] = out8[7] = 0;
    }
    return MGC_OK;
}

int mgc_overlap_counts(mgc_handle h, const uint8_t* a, const uint8_t* b, int64_t* out4)
{
    if (!h) return MGC_ERR_INVALID;
    { const int rc = mgc_edt_check(h, "mgc_overlap_counts", a); if (rc != MGC_OK) return rc; }
    if (!b) return mgc_fail(h, MGC_ERR_INVALID, "mgc_overlap_counts: b NULL");
    if (!out4) return mgc_fail(h, MGC_ERR_INVALID, "mgc_overlap_counts: out4 NULL");
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_overlap_counts");
    MgcBlocks pool;
    const uint8_t* d_a = nullptr;
    const uint8_t* d_b = nullptr;
    unsigned long long tot[4] = {0, 0, 0, 0};
    hipError_t e = mgc_edt_plane(h, pool, a, &d_a);
    if (e == hipSuccess) e = mgc_edt_plane(h, pool, b, &d_b);
    if (e == hipSuccess) e = mgc_edt_count(h, pool, d_a, d_b, nullptr, tot);
    const int rc = mgc_blocks_end(h, pool, e, "mgc_overlap_counts");
    if (rc != MGC_OK) return rc;
    for (int k = 0; k < 4; ++k) out4[k] = (int64_t)tot[k];
    return MGC_OK;
}

} /* extern "C" */
