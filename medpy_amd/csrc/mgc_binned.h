/*
 * mgc_binned.h -- the rule of the binned regional term (mgc_marker_histograms, mgc_add_tweights_binned, mgc_update_tweights_binned;
 * DESIGN 14), stated once: which bin a value of the feature image falls into, and the check of the arguments and of the two
 * tables, made before anything is written so that a refused call leaves the handle as it was (the approach of mgc_tweight_edit.h).
 * mgc_binned_bin is MGC_HD: the kernels of mgc_binned_ops.inl and host code compile the same lines.  Nothing here needs HIP:
 * mgc_kernels.hip includes it, and a stand-alone host program can (tests/hostsim/binned_main.cpp).
 */
#ifndef MGC_BINNED_H
#define MGC_BINNED_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "mgc_common.h"

#define MGC_BINNED_MAX_BINS 65536
/* up to this many bins a workgroup of k_marker_hist counts in LDS (two histograms of 32-bit counters: 32 KiB) and flushes what is
 * not zero; above it every count is a 64-bit integer add in device memory.  Mirrored in medpy_amd/_lib.py (BINNED_LDS_MAX). */
#define MGC_BINNED_LDS_MAX 4096

#define MGC_BINNED_OK 0
#define MGC_BINNED_INVALID 1 /* nbins, lo or width out of range; a table NULL; a table entry that is not finite */

/* floor((v - lo) / width) before the clamp: one f64 subtraction, one IEEE f64 division, one floor -- no reciprocal, nothing
 * contracted -- so that it is bit for bit numpy.floor((image.astype(float64) - lo) / width).  v is the value converted to double
 * (what mgc_load_as_double gives without take_abs; integers beyond 2^53 round to nearest, as NumPy's astype does). */
MGC_HD double mgc_binned_floor(double v, double lo, double width)
{
    const double d = v - lo;
    const double q = d / width;
    return floor(q);
}

/* the clamp of numpy.clip(., 0, nbins - 1), taken as an index.  NaN (refused by the callers before they bin) lands in bin 0: the
 * result is a valid index whatever comes in. */
MGC_HD int64_t mgc_binned_clamp(double f, int64_t nbins)
{
    if (!(f > 0.0)) return 0;
    if (f >= (double)(nbins - 1)) return nbins - 1;
    return (int64_t)f;
}

/* bin(v) = clamp(floor((double(v) - lo) / width), 0, nbins - 1) */
MGC_HD int64_t mgc_binned_bin(double v, double lo, double width, int64_t nbins) { return mgc_binned_clamp(mgc_binned_floor(v, lo, width), nbins); }

/* The limits of the binning: 1 <= nbins <= 65536, lo finite, width finite and > 0.  MGC_BINNED_OK, or MGC_BINNED_INVALID with a
 * sentence about the first offender in msg. */
static inline int mgc_binned_check_binning(int64_t nbins, double lo, double width, char* msg, size_t msg_len)
{
    if (nbins < 1 || nbins > MGC_BINNED_MAX_BINS) {
        snprintf(msg, msg_len, "nbins = %lld outside [1, %d]", (long long)nbins, MGC_BINNED_MAX_BINS);
        return MGC_BINNED_INVALID;
    }
    if (!isfinite(lo)) {
        snprintf(msg, msg_len, "lo = %g must be finite", lo);
        return MGC_BINNED_INVALID;
    }
    if (!isfinite(width) || !(width > 0.0)) {
        snprintf(msg, msg_len, "width = %g must be finite and > 0", width);
        return MGC_BINNED_INVALID;
    }
    return MGC_BINNED_OK;
}

/* The checks of the two table calls: the binning, then both tables given and every entry finite (negative entries are allowed, as
 * in mgc_add_tweights).  The FIRST offender is named: the lowest index, of one index the source entry; *which = 0 source, 1 sink
 * and *bad = its index (-1 where the binning or a NULL table offends).  Reads only. */
static inline int mgc_binned_check(int64_t nbins, double lo, double width, const double* source_table, const double* sink_table, int* which,
                                   int64_t* bad, char* msg, size_t msg_len)
{
    if (which) *which = 0;
    if (bad) *bad = -1;
    if (mgc_binned_check_binning(nbins, lo, width, msg, msg_len) != MGC_BINNED_OK) return MGC_BINNED_INVALID;
    if (!source_table || !sink_table) {
        if (which) *which = source_table ? 1 : 0;
        snprintf(msg, msg_len, "%s NULL", source_table ? "sink_table" : "source_table");
        return MGC_BINNED_INVALID;
    }
    for (int64_t b = 0; b < nbins; ++b) {
        const int w = !isfinite(source_table[b]) ? 0 : (!isfinite(sink_table[b]) ? 1 : -1);
        if (w < 0) continue;
        if (which) *which = w;
        if (bad) *bad = b;
        snprintf(msg, msg_len, "%s[%lld] = %g: table entries must be finite", w ? "sink_table" : "source_table", (long long)b, w ? sink_table[b] : source_table[b]);
        return MGC_BINNED_INVALID;
    }
    return MGC_BINNED_OK;
}

#endif /* MGC_BINNED_H */
