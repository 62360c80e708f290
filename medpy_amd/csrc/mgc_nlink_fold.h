/*
 * mgc_nlink_fold.h -- the per-arc rule of a warm update of the boundary term (mgc_update_boundary, DESIGN 10, "The boundary
 * term"): the capacity of an arc changes from c to c1 under a flow the last solve left on it.  Plain C++, no HIP: k_update_nlinks
 * (mgc_nlink_ops.inl) includes it, and a stand-alone host program can (tests/hostsim/nlink_fold_main.cpp).
 */
#ifndef MGC_NLINK_FOLD_H
#define MGC_NLINK_FOLD_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MGC_FOLD_HD __host__ __device__ __forceinline__
#else
#define MGC_FOLD_HD static inline
#endif

/* the same double, bit for bit (a capacity of NaN -- 0 / 0 of a linear term on a constant image -- equals itself here) */
MGC_FOLD_HD bool mgc_same_bits(double a, double b)
{
    uint64_t x, y;
    memcpy(&x, &a, sizeof(x));
    memcpy(&y, &b, sizeof(y));
    return x == y;
}

/* One arc, seen from its tail: c = capacity as built under the OLD arguments, c1 = under the NEW ones, *r = residual capacity.
 *   c1 == c (bitwise): nothing is touched, returns 0.
 *   otherwise  phi  = c - *r                    net flow out along the arc (signed: negative = flow came in along the reverse arc)
 *              phi1 = min(max(phi, -c1), c1)    the reverse arc has the same c1: the built-in terms are symmetric
 *              *r   = c1 - phi1                 in [0, 2 c1]
 *   and returns phi - phi1, the flow that no longer fits: the tail takes it back as (signed) excess.  The head evaluates the same rule
 *   from its own residual and gets the opposite amount.  *clamped: phi1 != phi.
 * A capacity that is not a number carries no flow (such an arc is not residual: k_build's masks) and gives none back. */
MGC_FOLD_HD double mgc_nlink_fold(double c, double c1, double* r, bool* clamped)
{
    *clamped = false;
    if (mgc_same_bits(c, c1)) return 0.0;
    double phi = c - *r;
    if (!(phi == phi)) phi = 0.0;
    if (!(c1 == c1)) { /* no capacity to speak of: whatever flowed goes back */
        *r = c1;
        *clamped = phi != 0.0;
        return phi;
    }
    double phi1 = phi;
    if (phi1 < -c1) phi1 = -c1;
    if (phi1 > c1) phi1 = c1;
    *r = c1 - phi1;
    *clamped = phi1 != phi;
    return phi - phi1;
}

/* The DIRECTED form (mgc_edit_nweights, DESIGN 10, "Edits of n-links by list"): the two arcs of a pair get capacities of their own.
 * One arc, seen from its tail: c_out / c_in = capacity as built of the arc and of its reverse BEFORE the edit, c_out1 / c_in1 = after
 * it, *r = the arc's residual capacity.
 *   both capacities unchanged (bitwise): nothing is touched, returns 0.
 *   otherwise  phi  = c_out - *r                       net flow out along the arc (negative: flow came in along the reverse arc)
 *              phi1 = min(max(phi, -c_in1), c_out1)    what the new pair can carry of it
 *              *r   = c_out1 - phi1                    in [0, c_out1 + c_in1]
 *   and returns phi - phi1 to the tail's signed excess.  The head evaluates the rule for the reverse arc from its own residual (its
 *   c_out is this c_in and so on) and gets the opposite amount.  *clamped: phi1 != phi.
 * With c_in == c_out and c_in1 == c_out1 this is mgc_nlink_fold(c_out, c_out1, r, clamped) bit for bit, the capacities that are not
 * numbers included; a reverse capacity that is not a number lets no flow come in. */
MGC_FOLD_HD double mgc_nlink_fold_directed(double c_out, double c_in, double c_out1, double c_in1, double* r, bool* clamped)
{
    *clamped = false;
    if (mgc_same_bits(c_out, c_out1) && mgc_same_bits(c_in, c_in1)) return 0.0;
    double phi = c_out - *r;
    if (!(phi == phi)) phi = 0.0;
    if (!(c_out1 == c_out1)) { /* no capacity to speak of: whatever flowed goes back */
        *r = c_out1;
        *clamped = phi != 0.0;
        return phi;
    }
    const double lo = c_in1 == c_in1 ? -c_in1 : 0.0;
    double phi1 = phi;
    if (phi1 < lo) phi1 = lo;
    if (phi1 > c_out1) phi1 = c_out1;
    *r = c_out1 - phi1;
    *clamped = phi1 != phi;
    return phi - phi1;
}

#endif /* MGC_NLINK_FOLD_H */
