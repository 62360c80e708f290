/*
 * mgc_edt.h -- the exact Euclidean distance transform of a byte plane on the lattice, and what the surface metrics put on top of it
 * (mgc_distance_transform, mgc_surface_distances, mgc_overlap_counts), stated once.
 *
 * The value.  With seeds S, spacing s and a_k = fl(s_k * (v_k - seed_k)), the transform of voxel v is the minimum over S of
 *     fl(fl(fl(a_x^2) + fl(a_y^2)) + fl(a_z^2))              (x the last array axis, z the first)
 * in f64, every operation rounded on its own: no fused multiply-add.  Rounding is monotone, so the minimum of the rounded sums is
 * the rounded sum of the minima and one pass per axis, last axis first, yields exactly this value as long as each pass finds the true
 * minimum of ITS rounded candidates:
 *
 *   mgc_edt_row_step     the last axis, from the bytes: the nearest seed to the left and to the right of a voxel, found in the seed
 *                        mask of its 64-voxel segment by bit counts, with a carry across segments (two sweeps over the row); the
 *                        nearer of the two gives the minimum because fl(fl(s * d)^2) does not fall when d grows
 *   mgc_edt_window_min   the other axes: g'(i) = min over j of fl(g(j) + fl(fl(s * (i - j))^2)), a WINDOWED EXHAUSTIVE minimum: the
 *                        candidates are taken in pairs j = i -+ d for d = 1, 2, ..., and the walk ends at the first d whose own term
 *                        w(d) = fl(fl(s * d)^2) is no smaller than the best so far -- every later candidate is fl(g(j) + w(d')) with
 *                        g(j) >= 0 and w(d') >= w(d), hence no smaller than w(d) either.  Exact by construction; no lower envelope,
 *                        no division, no intersection abscissa that could round the wrong way
 *   mgc_edt_panel_step   one PANEL of such lines (the whole line x MGC_EDT_PANEL_COLS neighbouring columns, which lie side by side in
 *                        memory) through a shared array: loaded row by row, every voxel's window walked there, written back in place
 *   mgc_edt_long_voxel   the same minimum for one voxel of a line too long for the panel, read from the plane itself and written to
 *                        a second plane
 *   mgc_edt_is_border    the border voxels of an object under scipy.ndimage.generate_binary_structure(ndim, connectivity):
 *                        X ^ binary_erosion(X, structure), everything outside the volume being background
 *
 * Everything is MGC_HD and free of HIP: the kernels of mgc_edt_ops.inl and the stand-alone host program of the CPU test tier
 * (tests/hostsim/edt_main.cpp) compile these very lines.  What differs is passed in: the seed mask of a segment (a wave's ballot on
 * the device, a loop over 64 bytes on the host) and the barrier of a panel (nothing for one worker).
 *
 * NO CONTRACTION.  The three functions that hold the arithmetic switch contraction off for their own statements (#pragma clang fp
 * contract(off), which hipcc honours in host and device code under every -ffp-contract setting but "fast"), the library is built with
 * -ffp-contract=off on top of that (medpy_amd/build.py), and the host program of the tests is compiled with -ffp-contract=off.
 */
#ifndef MGC_EDT_H
#define MGC_EDT_H

#include <stdint.h>

#include "mgc_common.h"

#define MGC_EDT_INF __builtin_huge_val()
#define MGC_EDT_PANEL_COLS 16   /* columns of a panel: 128 bytes of f64 side by side in memory */
#define MGC_EDT_PANEL_LINE 512  /* THE LONG-LINE THRESHOLD: lines of up to this many voxels go through a panel, longer ones through mgc_edt_long_voxel */
#define MGC_EDT_PANEL_BYTES (MGC_EDT_PANEL_LINE * MGC_EDT_PANEL_COLS * 8) /* 64 KiB, the LDS budget of a workgroup: two are resident on the 160 KiB of a CU */
#define MGC_EDT_COUNT_SEG 4096  /* voxels a wave counts and ranks at a time: 64 rounds of 64 lanes */
/* slots of out4 of mgc_distance_transform */
#define MGC_EDT_SEEDS 0
#define MGC_EDT_LONG_LINES 1
/* slots of out8 of mgc_surface_distances */
#define MGC_SD_BORDER_A 0
#define MGC_SD_BORDER_B 1
#define MGC_SD_SIZE_A 2
#define MGC_SD_SIZE_B 3
#define MGC_SD_LONG_LINES 4

/* fl(fl(s * d)^2) */
MGC_HD double mgc_edt_sq(double s, int64_t d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = s * (double)d;
    const double w = a * a;
    return w;
}

/* fl(base + w) */
MGC_HD double mgc_edt_add(double base, double w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double c = base + w;
    return c;
}

/* the seed at or left of `lane` among the seeds `mask` of the segment that starts at x0, else `carry` (the last seed before the segment, -1: none) */
MGC_HD int64_t mgc_edt_left(uint64_t mask, int lane, int64_t x0, int64_t carry)
{
    const uint64_t m = mask & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    return m ? x0 + 63 - __builtin_clzll(m) : carry;
}

/* the seed at or right of `lane`, else `carry` (the first seed behind the segment, -1: none) */
MGC_HD int64_t mgc_edt_right(uint64_t mask, int lane, int64_t x0, int64_t carry)
{
    const uint64_t m = mask >> lane;
    return m ? x0 + lane + __builtin_ctzll(m) : carry;
}

/* One row of n bytes, by the 64 lanes of which this is `lane`: g[x] = fl(fl(s * d)^2) with d the distance to the nearest seed of the
 * row, +inf in a row without one.  A seed is a byte whose being non-zero equals side != 0.  wave.seed_mask(row, side, x0, n, lane): bit
 * l = voxel x0 + l is a seed of the row (every lane gets the same word).  A lane writes and re-reads only its own entries of g. */
template <class Wave>
MGC_HD void mgc_edt_row_step(const uint8_t* row, int side, int64_t n, double s, double* g, int lane, Wave& wave)
{
    const int64_t nseg = (n + 63) / 64;
    int64_t carry = -1;
    for (int64_t seg = 0; seg < nseg; ++seg) { /* left to right: the nearest seed at or left of the voxel */
        const int64_t x0 = seg * 64, x = x0 + lane;
        const uint64_t mask = wave.seed_mask(row, side, x0, n, lane);
        const int64_t left = mgc_edt_left(mask, lane, x0, carry);
        if (x < n) g[x] = left < 0 ? MGC_EDT_INF : mgc_edt_sq(s, x - left);
        if (mask) carry = x0 + 63 - __builtin_clzll(mask);
    }
    carry = -1;
    for (int64_t seg = nseg - 1; seg >= 0; --seg) { /* right to left: the nearest seed at or right of it */
        const int64_t x0 = seg * 64, x = x0 + lane;
        const uint64_t mask = wave.seed_mask(row, side, x0, n, lane);
        const int64_t right = mgc_edt_right(mask, lane, x0, carry);
        if (x < n && right >= 0) {
            const double r = mgc_edt_sq(s, right - x);
            if (r < g[x]) g[x] = r;
        }
        if (mask) carry = x0 + __builtin_ctzll(mask);
    }
}

/* the items of one line: item j lies j * stride entries behind p */
struct MgcEdtLine {
    const double* p;
    int64_t stride;
    MGC_HD double operator()(int64_t j) const { return p[j * stride]; }
};

/* min over j in [0, n) of fl(in(j) + fl(fl(s * (i - j))^2)); in(j) >= 0 or +inf.  SHORT is 0; the test program's doctored build passes
 * 1, which leaves the farthest candidate of every line out. */
template <int SHORT, class In>
MGC_HD double mgc_edt_window_min(const In& in, int64_t n, int64_t i, double s)
{
    double best = in(i);
    const int64_t far = (i > n - 1 - i ? i : n - 1 - i) - SHORT;
    for (int64_t d = 1; d <= far; ++d) {
        const double w = mgc_edt_sq(s, d);
        if (w >= best) break;
        if (i - d >= 0) {
            const double c = mgc_edt_add(in(i - d), w);
            if (c < best) best = c;
        }
        if (i + d < n) {
            const double c = mgc_edt_add(in(i + d), w);
            if (c < best) best = c;
        }
    }
    return best;
}

/* One panel, by `nt` workers of which this is number t0: the lines of n items, `stride` entries apart, that start at
 * g[base .. base + cols), cols <= MGC_EDT_PANEL_COLS.  panel: n * MGC_EDT_PANEL_COLS doubles shared by the workers; sync(): their
 * barrier.  With nt a multiple of MGC_EDT_PANEL_COLS (the kernel's 256) a worker keeps one column.  In place: every read of g comes
 * before the first barrier, every write behind it, and no other panel holds these entries. */
template <int SHORT, class Sync>
MGC_HD void mgc_edt_panel_step(double* g, int64_t base, int64_t stride, int64_t n, int cols, double s, double* panel, int t0, int nt, Sync& sync)
{
    const int64_t items = n * MGC_EDT_PANEL_COLS;
    for (int64_t k = t0; k < items; k += nt) {
        const int c = (int)(k % MGC_EDT_PANEL_COLS);
        panel[k] = c < cols ? g[base + (k / MGC_EDT_PANEL_COLS) * stride + c] : MGC_EDT_INF;
    }
    sync();
    for (int64_t k = t0; k < items; k += nt) {
        const int c = (int)(k % MGC_EDT_PANEL_COLS);
        if (c >= cols) continue;
        const int64_t i = k / MGC_EDT_PANEL_COLS;
        const MgcEdtLine line = {panel + c, MGC_EDT_PANEL_COLS};
        g[base + i * stride + c] = mgc_edt_window_min<SHORT>(line, n, i, s);
    }
    sync(); /* (the next panel of these workers rewrites the array) */
}

/* voxel v of a plane whose lines along the axis of the pass have n items, `stride` entries apart: dst[v] from the line in src */
template <int SHORT>
MGC_HD void mgc_edt_long_voxel(const double* src, double* dst, int64_t v, int64_t n, int64_t stride, double s)
{
    const int64_t i = (v / stride) % n;
    const MgcEdtLine line = {src + (v - i * stride), stride};
    dst[v] = mgc_edt_window_min<SHORT>(line, n, i, s);
}

/* Is voxel (z, y, x) of the object `plane` (any byte but 0) a border voxel at `connectivity` (1 .. ndim)?  It is of the object and one
 * of its neighbours -- the offsets in {-1, 0, 1}^ndim with at most `connectivity` non-zero entries, over the LAST ndim axes of (dz, dy,
 * dx) -- is background or outside the volume.  A 2-D handle has no z-neighbours; a 3-D handle of shape (1, Y, X) has them, all outside. */
MGC_HD bool mgc_edt_is_border(const uint8_t* plane, int64_t dz, int64_t dy, int64_t dx, int ndim, int connectivity, int64_t z, int64_t y, int64_t x)
{
    if (!plane[(z * dy + y) * dx + x]) return false;
    for (int c = 0; c < 27; ++c) {
        const int oz = c / 9 - 1, oy = (c / 3) % 3 - 1, ox = c % 3 - 1;
        const int nonzero = (oz != 0) + (oy != 0) + (ox != 0);
        if (nonzero == 0 || nonzero > connectivity) continue;
        if ((ndim < 3 && oz) || (ndim < 2 && oy)) continue;
        const int64_t nz = z + oz, ny = y + oy, nx = x + ox;
        if (nz < 0 || nz >= dz || ny < 0 || ny >= dy || nx < 0 || nx >= dx) return true;
        if (!plane[(nz * dy + ny) * dx + nx]) return true;
    }
    return false;
}

/* the class of a voxel of a against b: 0 = tp (both), 1 = fp (a only), 2 = fn (b only), 3 = tn (neither); b NULL counts as all zero */
MGC_HD int mgc_edt_overlap_class(const uint8_t* a, const uint8_t* b, int64_t v) { return (a[v] ? 0 : 2) + ((b && b[v]) ? 0 : 1); }

#endif /* MGC_EDT_H */
