/*
 * mgc_reach_driver.inl -- the host side of mgc_cut_sets and mgc_cut_sets_tol (13b): both drivers, their entry points
 * and info getters, and what the two share.  Included ONCE, as the first of the drivers at the end of mgc_kernels.hip: the kernels of mgc_reach_ops.inl
 * and mgc_reach_tol_ops.inl come in here, behind every other kernel of that file, so that the kernels of the solve keep their places
 * in the code object ("Headline check").
 *
 * Everything a call writes is its own: mark planes, stamps, C-order planes, count block (and, at a tolerance, the scale plane and
 * the thresholded mask plane) come from the pool and go back.  Of the handle a call uses the two relabel lists with their counters
 * (empty between two solves, cleared again on the way out; at a tolerance they carry both floods, one after the other), the counter
 * look of the schedule (read_counts), and the scratch of the cut value (d_part, d_part2, MGC_S_CUT_SOURCE and MGC_S_CUT_SINK of d_scalar).  Labels, label
 * summaries, snapshot and residual state are read only.
 */
#include "mgc_reach_ops.inl"
#include "mgc_reach_tol_ops.inl"

/* One flood to its fixpoint: launch(cur, nxt, epoch) is one pass over list `cur` that fills list `nxt`.  Passes go out in stretches of
 * `batch` between two looks at the length of the list the next pass would consume; both lists are cleared on the way out. */
template <class Dev, class Launch>
static void mgc_reach_run_flood(Dev& dev, const MgcLayout& lay, int batch, uint32_t& epoch, Launch launch)
{
    const int lists[2] = {lay.rl_base, lay.rl_base + 1};
    int cnt[MGC_NCOUNT];
    for (int k = 0;;) {
        for (int b = 0; b < batch; ++b, ++k) {
            dev.zero_count(lists[(k + 1) & 1]);
            dev.flush_zero();
            launch(lists[k & 1], lists[(k + 1) & 1], ++epoch);
            dev.check(hipGetLastError());
        }
        dev.read_counts(cnt);
        if (cnt[lists[k & 1]] == 0 || dev.first_error != hipSuccess) break; /* the last pass queued nobody: fixpoint */
    }
    dev.zero_count(lists[0]);
    dev.zero_count(lists[1]);
    dev.flush_zero();
}

/* What the two drivers share around their launches.  The constructor is the prologue; end() is the epilogue. */
template <class Dev>
struct MgcReachCall {
    typedef std::chrono::steady_clock Clock;
    static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
    mgc_handle h;
    const MgcLattice& L;
    const MgcLayout lay;
    const char* const name; /* of the entry point: the roctx range and the head of an error message */
    MgcRange range;
    MgcBlocks pool;
    Dev dev;
    const bool timing;
    const size_t ntv, nvox8;
    const int seed_list; /* the list the seeding fills and the first pass consumes */
    /* the label summaries are those of the labels on the handle where the read-out of the solve wrote them (k_labels8: rows of whole
     * runs of eight); elsewhere the seed filter reads the labels of a tile itself */
    const uint8_t* const tsum;
    const int batch, wgs; /* passes between two looks; workgroups of the one-wave-per-tile kernels */
    uint32_t epoch = 0;
    Clock::time_point t0, t1; /* device_ms of the note runs from begin() to counts() */

    MgcReachCall(mgc_handle h_, const MgcLayout& lay_, const char* name_)
        : h(h_), L(h_->L), lay(lay_), name(name_), range(name_), timing(h_->timing), ntv((size_t)h_->L.ntiles * MGC_TV), nvox8(((size_t)h_->nvox + 7) & ~(size_t)7),
          seed_list(lay_.rl_base), tsum(h_->L.dx % 8 == 0 ? (const uint8_t*)h_->d_tsum : (const uint8_t*)nullptr),
          batch(h_->params.relabel_batch > 0 ? h_->params.relabel_batch : 8), wgs((h_->L.ntiles + 3) / 4 < 4096 ? (h_->L.ntiles + 3) / 4 : 4096)
    {
        dev.h = h;
        h->timing = false; /* (the event pairs of a solve's launches are not for these) */
    }
    /* the blocks are there (or not: the error): the device part of the call begins */
    hipError_t begin()
    {
        t0 = Clock::now();
        return pool.err;
    }
    void zero_lists()
    {
        dev.zero_count(lay.rl_base);
        dev.zero_count(lay.rl_base + 1);
        dev.flush_zero();
    }
    /* one flood from the tiles on the seed list; info: the (passes, visits) pair to count into */
    template <bool BACK>
    void flood(const void* masks, uint8_t* marks, uint32_t* stamp, unsigned long long* info)
    {
        mgc_reach_run_flood(dev, lay, batch, epoch, [&](int cur, int nxt, uint32_t ep) {
            if (L.ndir == 6) hipLaunchKernelGGL((k_reach_flood<6, BACK>), dim3(dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, masks, marks, stamp, cur, cur, ep, nxt, info);
            else hipLaunchKernelGGL((k_reach_flood<26, BACK>), dim3(dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, masks, marks, stamp, cur, cur, ep, nxt, info);
        });
    }
    /* the capacity of the cut around the C-order plane `side`, into slot k of d_scalar: the label-driven kernel of the solve's read-out
     * (the form without label summaries, with its tflags rule for tr0) on the plane instead of the labels */
    void cut_value(const uint8_t* side, int k)
    {
        const int grid = L.ntiles < h->grid_cap * 4 ? L.ntiles : h->grid_cap * 4;
        hipLaunchKernelGGL(k_cut_value26<0>, dim3((grid + 3) / 4 < 8192 ? (grid + 3) / 4 : 8192), dim3(256), 0, h->stream, L, h->build_args, (const double*)h->d_tr0, side, (const uint8_t*)nullptr, h->d_part);
        mgc_sum_partials(h, (int64_t)L.ntiles, h->d_scalar + k);
    }
    /* the scalars to the host, on a drained stream */
    hipError_t scalars(hipError_t e)
    {
        if (e == hipSuccess) e = hipMemcpyAsync(h->h_scalar, h->d_scalar, MGC_S_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        return e;
    }
    /* the count block to the host: the end of the device part of the call */
    hipError_t counts(hipError_t e, const unsigned long long* info, unsigned long long* h_info, size_t bytes)
    {
        h->timing = timing;
        if (e == hipSuccess) e = hipMemcpy(h_info, info, bytes, hipMemcpyDeviceToHost);
        t1 = Clock::now();
        return e;
    }
    hipError_t download(hipError_t e, const uint8_t* plane, uint8_t* out)
    {
        return e == hipSuccess && out ? mgc_staged_copy(h, (void*)plane, out, (size_t)h->nvox, false) : e;
    }
    /* the blocks go back; an error becomes the handle's message under the entry point's name */
    int end(hipError_t e)
    {
        pool.release();
        return e == hipSuccess ? MGC_OK : mgc_hip_fail(h, name, e);
    }
};

/* mgc_cut_sets on the kernels of either neighbourhood (mgc_reach_ops.inl) */
template <class Dev>
static int mgc_cut_sets_on(mgc_handle h, const MgcLayout lay, uint8_t* from_source, uint8_t* ambiguous)
{
    MgcReachCall<Dev> c(h, lay, "mgc_cut_sets");
    typedef typename MgcReachCall<Dev>::Clock Clock;
    const MgcLattice& L = c.L;
    uint8_t* marks = (uint8_t*)c.pool.get(c.ntv);
    uint8_t* d_fs = (uint8_t*)c.pool.get(c.nvox8);
    uint8_t* d_amb = ambiguous ? (uint8_t*)c.pool.get(c.nvox8) : nullptr;
    uint32_t* stamp = (uint32_t*)c.pool.get((size_t)L.ntiles * sizeof(uint32_t));
    int32_t* cnt3 = (int32_t*)c.pool.get((size_t)L.ntiles * 3 * sizeof(int32_t));
    unsigned long long* info = (unsigned long long*)c.pool.get(8 * sizeof(unsigned long long));
    unsigned long long h_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = c.begin();
    if (e == hipSuccess) e = hipMemsetAsync(marks, 0, c.ntv, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(stamp, 0, (size_t)L.ntiles * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(info, 0, 8 * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) {
        c.zero_lists();
        hipLaunchKernelGGL(k_reach_seed, dim3(c.wgs), dim3(256), 0, h->stream, L, c.tsum, marks, c.seed_list, c.seed_list, info);
        c.dev.check(hipGetLastError());
        c.template flood<false>(L.ndir == 6 ? (const void*)L.rmask : (const void*)L.rmask32, marks, stamp, info + MGC_REACH_PASSES);
        hipLaunchKernelGGL(k_reach_readout, dim3(c.wgs), dim3(256), 0, h->stream, L, (const uint8_t*)marks, d_fs, d_amb, cnt3);
        hipLaunchKernelGGL(k_reach_sum, dim3(1), dim3(MGC_TV), 0, h->stream, (const int32_t*)cnt3, L.ntiles, info);
        c.cut_value(d_fs, MGC_S_CUT_SOURCE); /* (R_s | V \ R_s) */
        c.dev.check(hipGetLastError());
        e = c.dev.first_error;
    }
    e = c.counts(c.scalars(e), info, h_info, sizeof(h_info));
    e = c.download(c.download(e, d_fs, from_source), d_amb, ambiguous);
    const int rc = c.end(e);
    if (rc != MGC_OK) return rc;
    for (int k = 0; k < 8; ++k) h->cut_info[k] = (int64_t)h_info[k];
    h->cut_info[7] = 0;
    h->cut_source = h->flow_const + h->h_scalar[MGC_S_CUT_SOURCE];
    h->cut_info_valid = true;
    /* no error: the note says where the time of this call went (tools/gpu_cut_sets.py records it) */
    (void)mgc_fail(h, MGC_OK, "mgc_cut_sets: device_ms=%.3f download_ms=%.3f", c.ms(c.t0, c.t1), c.ms(c.t1, Clock::now()));
    return MGC_OK;
}

/* mgc_cut_sets_tol on the kernels of either neighbourhood (mgc_reach_tol_ops.inl): all of them, tol = 0 included.  Both floods run on
 * the thresholded plane.  The summary skip of the forward seeding apart, nothing reads labels or label summaries; the backward path
 * reads neither. */
template <class Dev>
static int mgc_cut_sets_tol_on(mgc_handle h, const MgcLayout lay, double tol, uint8_t* from_source, uint8_t* to_sink, uint8_t* ambiguous)
{
    MgcReachCall<Dev> c(h, lay, "mgc_cut_sets_tol");
    typedef typename MgcReachCall<Dev>::Clock Clock;
    const MgcLattice& L = c.L;
    double* scale = (double*)c.pool.get(c.ntv * sizeof(double));
    void* omask = c.pool.get(c.ntv * (L.ndir == 6 ? sizeof(uint8_t) : sizeof(uint32_t)));
    uint8_t* fwd = (uint8_t*)c.pool.get(c.ntv);
    uint8_t* bwd = (uint8_t*)c.pool.get(c.ntv);
    uint8_t* d_fs = (uint8_t*)c.pool.get(c.nvox8);
    uint8_t* d_ns = (uint8_t*)c.pool.get(c.nvox8);
    uint8_t* d_ts = to_sink ? (uint8_t*)c.pool.get(c.nvox8) : nullptr;
    uint8_t* d_amb = ambiguous ? (uint8_t*)c.pool.get(c.nvox8) : nullptr;
    uint32_t* stamp = (uint32_t*)c.pool.get((size_t)L.ntiles * sizeof(uint32_t));
    int32_t* cnt3 = (int32_t*)c.pool.get((size_t)L.ntiles * 3 * sizeof(int32_t));
    unsigned long long* info = (unsigned long long*)c.pool.get(16 * sizeof(unsigned long long));
    unsigned long long h_info[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double ms_phase[5] = {0.0, 0.0, 0.0, 0.0, 0.0}; /* scale, open, forward flood, backward flood, read-out (each ends on a drained stream) */
    hipError_t e = c.begin();
    if (e == hipSuccess) e = hipMemsetAsync(fwd, 0, c.ntv, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bwd, 0, c.ntv, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(stamp, 0, (size_t)L.ntiles * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(info, 0, 16 * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) {
        auto t = Clock::now();
        if (L.ndir == 6) hipLaunchKernelGGL(k_reach_scale<6>, dim3(c.dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, scale, info);
        else hipLaunchKernelGGL(k_reach_scale<26>, dim3(c.dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, scale, info);
        c.dev.check(hipGetLastError());
        c.dev.check(hipStreamSynchronize(h->stream));
        ms_phase[0] = c.ms(t, Clock::now());
        t = Clock::now();
        if (L.ndir == 6) hipLaunchKernelGGL(k_reach_open<6>, dim3(c.dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, (const double*)scale, tol, omask, info);
        else hipLaunchKernelGGL(k_reach_open<26>, dim3(c.dev.grid(L.ntiles)), dim3(MGC_TV), 0, h->stream, L, (const double*)scale, tol, omask, info);
        c.dev.check(hipGetLastError());
        c.dev.check(hipStreamSynchronize(h->stream));
        ms_phase[1] = c.ms(t, Clock::now());
        t = Clock::now();
        c.zero_lists();
        hipLaunchKernelGGL(k_reach_seed_tol<false>, dim3(c.wgs), dim3(256), 0, h->stream, L, (const uint8_t*)h->d_tflags, (const double*)h->d_tr0, (const double*)scale, tol, c.tsum, fwd,
                           c.seed_list, c.seed_list, info + MGC_REACH_SEEDED, info + MGC_REACHT_SKIPPED, info + MGC_REACHT_TLINKS_CLOSED);
        c.dev.check(hipGetLastError());
        c.template flood<false>(omask, fwd, stamp, info + MGC_REACH_PASSES);
        ms_phase[2] = c.ms(t, Clock::now());
        t = Clock::now();
        hipLaunchKernelGGL(k_reach_seed_tol<true>, dim3(c.wgs), dim3(256), 0, h->stream, L, (const uint8_t*)h->d_tflags, (const double*)h->d_tr0, (const double*)scale, tol, (const uint8_t*)nullptr, bwd,
                           c.seed_list, c.seed_list, info + MGC_REACHT_BACK + 2, (unsigned long long*)nullptr, info + MGC_REACHT_TLINKS_CLOSED);
        c.dev.check(hipGetLastError());
        c.template flood<true>(omask, bwd, stamp, info + MGC_REACHT_BACK);
        ms_phase[3] = c.ms(t, Clock::now());
        t = Clock::now();
        hipLaunchKernelGGL(k_reach_readout_tol, dim3(c.wgs), dim3(256), 0, h->stream, L, (const uint8_t*)fwd, (const uint8_t*)bwd, d_fs, d_ts, d_amb, d_ns, cnt3);
        hipLaunchKernelGGL(k_reach_sum, dim3(1), dim3(MGC_TV), 0, h->stream, (const int32_t*)cnt3, L.ntiles, info);
        c.cut_value(d_fs, MGC_S_CUT_SOURCE); /* (R_s | V \ R_s) */
        c.cut_value(d_ns, MGC_S_CUT_SINK); /* (V \ R_t | R_t) */
        c.dev.check(hipGetLastError());
        e = c.scalars(c.dev.first_error);
        ms_phase[4] = c.ms(t, Clock::now());
    }
    e = c.counts(e, info, h_info, sizeof(h_info));
    e = c.download(c.download(c.download(e, d_fs, from_source), d_ts, to_sink), d_amb, ambiguous);
    const int rc = c.end(e);
    if (rc != MGC_OK) return rc;
    for (int k = 0; k < 16; ++k) h->cut_tol_info[k] = k < MGC_REACHT_SCALE_MAX ? (int64_t)h_info[k] : 0;
    double scale_max = 0.0;
    memcpy(&scale_max, &h_info[MGC_REACHT_SCALE_MAX], sizeof(double));
    h->cut_tol_vals[0] = tol;
    h->cut_tol_vals[1] = h->flow_const + h->h_scalar[MGC_S_CUT_SOURCE];
    h->cut_tol_vals[2] = h->flow_const + h->h_scalar[MGC_S_CUT_SINK];
    h->cut_tol_vals[3] = scale_max;
    h->cut_tol_info_valid = true;
    /* no error: the note says where the time of this call went (tools/gpu_cut_sets_tol.py records it) */
    (void)mgc_fail(h, MGC_OK, "mgc_cut_sets_tol: device_ms=%.3f scale_ms=%.3f open_ms=%.3f forward_ms=%.3f backward_ms=%.3f readout_ms=%.3f download_ms=%.3f",
                   c.ms(c.t0, c.t1), ms_phase[0], ms_phase[1], ms_phase[2], ms_phase[3], ms_phase[4], c.ms(c.t1, Clock::now()));
    return MGC_OK;
}

/* what both entry points ask of the handle before anything is written; `what`: "flood" or "floods" */
static int mgc_reach_check_state(mgc_handle h, const char* name, const char* what)
{
    if (h->nranks > 1) return mgc_fail(h, MGC_ERR_UNSUPPORTED, "%s: a slab holds a part of the residual graph only (the %s would have to cross the slab borders)", name, what);
    if (!h->built) return mgc_fail(h, MGC_ERR_STATE, "%s before mgc_build", name);
    if (!h->solved) return mgc_fail(h, MGC_ERR_STATE, "%s before mgc_maxflow (or after an update or edit that the next mgc_maxflow has yet to solve)", name);
    if (!h->converged || h->unconverged) return mgc_fail(h, MGC_ERR_STATE, "%s: the last mgc_maxflow of this handle did not run to a maximum preflow", name);
    return MGC_OK;
}

extern "C" {

int mgc_cut_sets(mgc_handle h, uint8_t* from_source, uint8_t* ambiguous)
{
    if (!h) return MGC_ERR_INVALID;
    const int rc = mgc_reach_check_state(h, "mgc_cut_sets", "flood");
    if (rc != MGC_OK) return rc;
    MGC_HIP(h, hipSetDevice(h->device));
    return h->L.ndir == 6 ? mgc_cut_sets_on<HipDev>(h, mgc_layout6(), from_source, ambiguous) : mgc_cut_sets_on<HipDev26>(h, mgc_layout26(), from_source, ambiguous);
}

int mgc_get_cut_sets_info(mgc_handle h, int64_t* out8, double* source_cut)
{
    if (!h) return MGC_ERR_INVALID;
    if (!h->cut_info_valid) return mgc_fail(h, MGC_ERR_STATE, "mgc_get_cut_sets_info before mgc_cut_sets");
    if (out8) for (int k = 0; k < 8; ++k) out8[k] = h->cut_info[k];
    if (source_cut) *source_cut = h->cut_source;
    return MGC_OK;
}

int mgc_cut_sets_tol(mgc_handle h, double tol, uint8_t* from_source, uint8_t* to_sink, uint8_t* ambiguous)
{
    if (!h) return MGC_ERR_INVALID;
    const int rc = mgc_reach_check_state(h, "mgc_cut_sets_tol", "floods");
    if (rc != MGC_OK) return rc;
    if (!(tol >= 0.0) || !(tol < 1.0)) return mgc_fail(h, MGC_ERR_INVALID, "mgc_cut_sets_tol: tol must be a number in [0, 1), got %g", tol);
    MGC_HIP(h, hipSetDevice(h->device));
    return h->L.ndir == 6 ? mgc_cut_sets_tol_on<HipDev>(h, mgc_layout6(), tol, from_source, to_sink, ambiguous)
                          : mgc_cut_sets_tol_on<HipDev26>(h, mgc_layout26(), tol, from_source, to_sink, ambiguous);
}

int mgc_get_cut_sets_tol_info(mgc_handle h, int64_t* out16, double* out4)
{
    if (!h) return MGC_ERR_INVALID;
    if (!h->cut_tol_info_valid) return mgc_fail(h, MGC_ERR_STATE, "mgc_get_cut_sets_tol_info before mgc_cut_sets_tol");
    if (out16) for (int k = 0; k < 16; ++k) out16[k] = h->cut_tol_info[k];
    if (out4) for (int k = 0; k < 4; ++k) out4[k] = h->cut_tol_vals[k];
    return MGC_OK;
}

} /* extern "C" */
