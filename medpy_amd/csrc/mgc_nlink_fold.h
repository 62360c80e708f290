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

#endif /* MGC_NLINK_FOLD_H */
