/*
 * mgc_cc_driver.inl -- the host side of mgc_components and mgc_clean_labels.  Included ONCE, at the end of
 * mgc_kernels.hip behind mgc_label_hist_driver.inl: the kernels of mgc_cc_ops.inl come in here, behind those, so that the
 * kernels before them keep their places in the code object ("Headline check").  Every check comes before the first write,
 * and a call leaves the handle as it was: it reads the labels, the label summaries and the marker planes, and every block it uses
 * comes from the pool and goes back before it returns (MgcBlocks).
 */
#include "mgc_cc_ops.inl"

/* the planes of one call: 9 bytes per voxel, and the per-segment words of the ranking */
struct MgcCcPlanes {
    uint32_t* parent = nullptr;
    uint32_t* count = nullptr;
    uint8_t* flags = nullptr;
    unsigned long long* roots = nullptr; /* nseg + 1: roots per segment, scanned in place */
    unsigned long long* part = nullptr;  /* 2 * nseg */
    unsigned long long* info = nullptr;  /* the eight slots of out8, then mgc_cc_best of the volume */
    int64_t nseg = 0;
};

/* the table of one run, on the device: rows = min(K, cap) entries (the blocks hold at least one) */
struct MgcCcTable {
    int64_t K = 0, rows = 0;
    int64_t* first = nullptr;
    int64_t* size = nullptr;
    uint8_t* flags = nullptr;
};

static void mgc_cc_alloc(mgc_handle h, MgcBlocks& pool, MgcCcPlanes& P)
{
    const size_t n = (size_t)h->nvox;
    P.nseg = (h->nvox + MGC_CC_SEG - 1) / MGC_CC_SEG;
    P.parent = (uint32_t*)pool.get(n * sizeof(uint32_t));
    P.count = (uint32_t*)pool.get(n * sizeof(uint32_t));
    P.flags = (uint8_t*)pool.get((n + 3) & ~(size_t)3);
    P.roots = (unsigned long long*)pool.get((size_t)(P.nseg + 1) * sizeof(unsigned long long));
    P.part = (unsigned long long*)pool.get((size_t)(2 * P.nseg) * sizeof(unsigned long long));
    P.info = (unsigned long long*)pool.get(9 * sizeof(unsigned long long));
}

/* One labelling of `plane` (device, C order): afterwards P.parent holds the ids, T the first min(K, cap) rows, h_info the out8.
 * tsum: the label summaries when the plane is the current cut's labels and the read-out wrote them, else NULL. */
static hipError_t mgc_cc_run(mgc_handle h, MgcBlocks& pool, const MgcCcPlanes& P, const uint8_t* plane, const uint8_t* tsum, int side, int full, int64_t cap, MgcCcTable& T,
                             unsigned long long h_info[8])
{
    const MgcLattice& L = h->L;
    const int64_t nvox = h->nvox, nseg = P.nseg;
    const unsigned g_tile = (unsigned)(L.ntiles < (1 << 18) ? L.ntiles : (1 << 18));
    const int64_t vb = (nvox + 255) / 256, sb = (nseg + 3) / 4;
    const unsigned g_vox = (unsigned)(vb < 65536 ? vb : 65536), g_seg = (unsigned)(sb < 16384 ? sb : 16384);
    hipError_t e = hipMemsetAsync(P.info, 0, 9 * sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) return e;
    if (full) {
        hipLaunchKernelGGL(k_cc_tile<true>, dim3(g_tile), dim3(MGC_TV), 0, h->stream, L, plane, side, tsum, (const uint8_t*)h->d_fg, (const uint8_t*)h->d_bg, P.parent, P.count, P.flags, P.info);
        hipLaunchKernelGGL(k_cc_merge<true>, dim3(g_tile), dim3(MGC_TV), 0, h->stream, L, P.parent, P.info);
    } else {
        hipLaunchKernelGGL(k_cc_tile<false>, dim3(g_tile), dim3(MGC_TV), 0, h->stream, L, plane, side, tsum, (const uint8_t*)h->d_fg, (const uint8_t*)h->d_bg, P.parent, P.count, P.flags, P.info);
        hipLaunchKernelGGL(k_cc_merge<false>, dim3(g_tile), dim3(MGC_TV), 0, h->stream, L, P.parent, P.info);
    }
    hipLaunchKernelGGL(k_cc_flatten<0>, dim3(g_vox), dim3(256), 0, h->stream, P.parent, nvox, P.info);
    hipLaunchKernelGGL(k_cc_gather<0>, dim3(g_vox), dim3(256), 0, h->stream, (const uint32_t*)P.parent, P.count, P.flags, nvox);
    hipLaunchKernelGGL(k_cc_seg_count<0>, dim3(g_seg), dim3(256), 0, h->stream, (const uint32_t*)P.parent, (const uint32_t*)P.count, nvox, nseg, P.roots, P.part);
    hipLaunchKernelGGL(k_labels_delta_scan, dim3(1), dim3(MGC_SCAN_THREADS), 0, h->stream, P.roots, nseg);
    hipLaunchKernelGGL(k_cc_seg_reduce<0>, dim3(1), dim3(MGC_TV), 0, h->stream, (const unsigned long long*)P.part, nseg, P.info, P.info + 8);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned long long k = 0ull;
    if ((e = hipMemcpyAsync(&k, P.roots + nseg, sizeof(k), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    T.K = (int64_t)k;
    T.rows = T.K < cap ? T.K : cap;
    const size_t rows = (size_t)(T.rows > 0 ? T.rows : 1);
    T.first = (int64_t*)pool.get(rows * sizeof(int64_t));
    T.size = (int64_t*)pool.get(rows * sizeof(int64_t));
    T.flags = (uint8_t*)pool.get(rows);
    if (pool.err != hipSuccess) return pool.err;
    hipLaunchKernelGGL(k_cc_rank_write<0>, dim3(g_seg), dim3(256), 0, h->stream, (const uint32_t*)P.parent, P.count, (const uint8_t*)P.flags, nvox, nseg, (const unsigned long long*)P.roots, T.rows,
                       T.first, T.size, T.flags);
    hipLaunchKernelGGL(k_cc_ids<0>, dim3(g_vox), dim3(256), 0, h->stream, P.parent, (const uint32_t*)P.count, nvox, (const unsigned long long*)(P.info + 8), P.info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_info, P.info, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    h_info[MGC_CC_K] = k;
    return hipSuccess;
}

/* what both entry points ask of the handle before anything is written */
static int mgc_cc_check(mgc_handle h, const char* name, const uint8_t* labels)
{
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: not on a slab of a multi-GPU volume", name);
    if (h->nvox >= MGC_CC_MAX_VOXELS) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: %lld voxels: parents are 32-bit, the volume must hold fewer than 2^32 - 1", name, (long long)h->nvox);
    if (!labels) {
        char who[96];
        snprintf(who, sizeof(who), "%s (labels NULL)", name);
        return mgc_reach_check_state(h, who, "labels");
    }
    return MGC_OK;
}

/* *plane: the device plane to label -- the labels of the current cut where they lie, or a caller's plane in a block of the call,
 * brought to 0 / 1 bytes; *tsum: the label summaries that go with it or NULL */
static hipError_t mgc_cc_plane(mgc_handle h, MgcBlocks& pool, const uint8_t* labels, const uint8_t** plane, const uint8_t** tsum)
{
    *tsum = nullptr;
    if (!labels) {
        *plane = h->d_labels;
        if (h->L.dx % 8 == 0) *tsum = h->d_tsum;
        return pool.err;
    }
    uint8_t* d = (uint8_t*)pool.get((size_t)h->nvox);
    *plane = d;
    if (pool.err != hipSuccess) return pool.err;
    hipError_t e = mgc_staged_copy(h, d, const_cast<uint8_t*>(labels), (size_t)h->nvox, true);
    if (e != hipSuccess) return e;
    const int64_t vb = (h->nvox + 255) / 256;
    hipLaunchKernelGGL(k_cc_normalise<0>, dim3((unsigned)(vb < 65536 ? vb : 65536)), dim3(256), 0, h->stream, d, h->nvox);
    return hipGetLastError();
}

extern "C" {

int mgc_components(mgc_handle h, const uint8_t* labels, int side, int full, int32_t* ids, int64_t cap, int64_t* first, int64_t* size, uint8_t* flags, int64_t* out8)
{
    if (!h) return MGC_ERR_INVALID;
    { const int rc = mgc_cc_check(h, "mgc_components", labels); if (rc != MGC_OK) return rc; }
    if (side != 0 && side != 1) return mgc_fail(h, MGC_ERR_INVALID, "mgc_components: side must be 0 (background) or 1 (foreground), got %d", side);
    if (full != 0 && full != 1) return mgc_fail(h, MGC_ERR_INVALID, "mgc_components: full must be 0 (face neighbourhood) or 1 (full neighbourhood), got %d", full);
    if (cap < 0) return mgc_fail(h, MGC_ERR_INVALID, "mgc_components: the capacity of the table must not be negative, got %lld", (long long)cap);
    if (cap > 0 && (!first || !size || !flags)) return mgc_fail(h, MGC_ERR_INVALID, "mgc_components: first / size / flags NULL with a capacity of %lld", (long long)cap);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_components");
    MgcBlocks pool;
    MgcCcPlanes P;
    MgcCcTable T;
    unsigned long long h_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t* plane = nullptr;
    const uint8_t* tsum = nullptr;
    mgc_cc_alloc(h, pool, P);
    hipError_t e = pool.err;
    if (e == hipSuccess) e = mgc_cc_plane(h, pool, labels, &plane, &tsum);
    if (e == hipSuccess) e = mgc_cc_run(h, pool, P, plane, tsum, side, full, cap, T, h_info);
    if (e == hipSuccess && T.rows > 0) {
        e = hipMemcpyAsync(first, T.first, (size_t)T.rows * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(size, T.size, (size_t)T.rows * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(flags, T.flags, (size_t)T.rows, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e == hipSuccess && ids) e = mgc_staged_copy(h, P.parent, ids, (size_t)h->nvox * sizeof(int32_t), false);
    const int rc = mgc_blocks_end(h, pool, e, "mgc_components");
    if (rc != MGC_OK) return rc;
    if (out8)
        for (int k = 0; k < 8; ++k) out8[k] = (int64_t)h_info[k];
    return MGC_OK;
}

int mgc_clean_labels(mgc_handle h, const uint8_t* labels, const mgc_clean_rule* rule, uint8_t* out, int64_t cap, int64_t* changed_ids, int64_t* out8)
{
    if (!h) return MGC_ERR_INVALID;
    { const int rc = mgc_cc_check(h, "mgc_clean_labels", labels); if (rc != MGC_OK) return rc; }
    if (!rule) return mgc_fail(h, MGC_ERR_INVALID, "mgc_clean_labels: rule NULL");
    if (rule->min_size < 1) return mgc_fail(h, MGC_ERR_INVALID, "mgc_clean_labels: min_size must be at least 1, got %lld", (long long)rule->min_size);
    if (rule->largest < 0) return mgc_fail(h, MGC_ERR_INVALID, "mgc_clean_labels: largest must not be negative (0: no limit), got %lld", (long long)rule->largest);
    if ((rule->fg_full | rule->seeded | rule->fill_holes | rule->hole_full) & ~1)
        return mgc_fail(h, MGC_ERR_INVALID, "mgc_clean_labels: fg_full, seeded, fill_holes and hole_full must be 0 or 1, got %d, %d, %d, %d", (int)rule->fg_full, (int)rule->seeded,
                        (int)rule->fill_holes, (int)rule->hole_full);
    if (cap < 0) return mgc_fail(h, MGC_ERR_INVALID, "mgc_clean_labels: the capacity of the list must not be negative, got %lld", (long long)cap);
    MGC_HIP(h, hipSetDevice(h->device));
    MgcRange range_("mgc_clean_labels");
    MgcBlocks pool;
    MgcCcPlanes P;
    int64_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t* plane = nullptr;
    const uint8_t* tsum = nullptr;
    const int64_t nvox = h->nvox, vb = (nvox + 255) / 256;
    const unsigned g_vox = (unsigned)(vb < 65536 ? vb : 65536);
    const int64_t dseg = mgc_labels_delta_segments(nvox);
    mgc_cc_alloc(h, pool, P);
    uint8_t* const d_out = (uint8_t*)pool.get((size_t)nvox);
    unsigned long long* const d_off = (unsigned long long*)pool.get((size_t)(dseg + 1) * sizeof(unsigned long long));
    hipError_t e = pool.err;
    if (e == hipSuccess) e = mgc_cc_plane(h, pool, labels, &plane, &tsum);
    /* step 1: the foreground components, the rule on the host, one keep byte per component back up */
    MgcBlocks own; /* the table and the keep bytes of a step: back to the pool on a drained stream, after an error too */
    for (int step = 0; step < 2 && e == hipSuccess; ++step) {
        if (step == 1 && !rule->fill_holes) break;
        MgcCcTable T;
        unsigned long long h_info[8];
        e = step == 0 ? mgc_cc_run(h, own, P, plane, tsum, 1, rule->fg_full, INT64_MAX, T, h_info) : mgc_cc_run(h, own, P, d_out, nullptr, 0, rule->hole_full, INT64_MAX, T, h_info);
        if (e != hipSuccess) break;
        std::vector<int64_t> size((size_t)T.K);
        std::vector<uint8_t> flags((size_t)T.K), keep;
        if (T.K > 0) {
            e = mgc_staged_copy(h, T.size, size.data(), (size_t)T.K * sizeof(int64_t), false);
            if (e == hipSuccess) e = mgc_staged_copy(h, T.flags, flags.data(), (size_t)T.K, false);
            if (e != hipSuccess) break;
        }
        if (step == 0) {
            res[0] = T.K;
            keep.assign(T.K ? (size_t)T.K : 1, 0);
            mgc_cc_rule_keep(T.K, size.data(), flags.data(), rule->min_size, rule->largest, rule->seeded, keep.data(), &res[1], &res[2]);
        } else { /* the cavities: neither on the border nor held open by a background marker */
            keep.assign(T.K ? (size_t)T.K : 1, 0);
            for (size_t k = 0; k < (size_t)T.K; ++k)
                if (!(flags[k] & (MGC_CC_FLAG_BORDER | MGC_CC_FLAG_BG))) { keep[k] = 1; res[3] += 1; res[4] += size[k]; }
        }
        uint8_t* const d_keep = (uint8_t*)own.get(keep.size());
        if ((e = own.err) != hipSuccess) break;
        e = mgc_staged_copy(h, d_keep, keep.data(), keep.size(), true);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_cc_apply<0>, dim3(g_vox), dim3(256), 0, h->stream, (const uint32_t*)P.parent, (const uint8_t*)d_keep, step == 0 ? (const uint8_t*)nullptr : (const uint8_t*)d_out, d_out, nvox);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) own.release();
    }
    if (!own.held.empty() || own.err != hipSuccess) { /* a step ended on an error */
        (void)hipStreamSynchronize(h->stream);
        own.release();
    }
    /* the voxels the rule changed: the label delta of the cleaned plane against the input plane, both 0 / 1 */
    if (e == hipSuccess) e = mgc_labels_delta_launch(h->stream, d_out, plane, nvox, d_off, 0, nullptr);
    unsigned long long total = 0ull;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d_off + dseg, sizeof(total), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    res[5] = (int64_t)total;
    if (e == hipSuccess && changed_ids && (int64_t)total <= cap) {
        if (total > 0) {
            int64_t* const d_ids = (int64_t*)pool.get((size_t)total * sizeof(int64_t));
            e = pool.err;
            if (e == hipSuccess) e = mgc_labels_delta_launch(h->stream, d_out, plane, nvox, d_off, (int64_t)total, d_ids);
            if (e == hipSuccess) e = mgc_staged_copy(h, d_ids, changed_ids, (size_t)total * sizeof(int64_t), false);
        }
        res[6] = 1;
    }
    if (e == hipSuccess && out) e = mgc_staged_copy(h, d_out, out, (size_t)nvox, false);
    const int rc = mgc_blocks_end(h, pool, e, "mgc_clean_labels");
    if (rc != MGC_OK) return rc;
    if (out8)
        for (int k = 0; k < 8; ++k) out8[k] = res[k];
    return MGC_OK;
}

} /* extern "C" */
