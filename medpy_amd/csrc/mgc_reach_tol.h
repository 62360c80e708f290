/*
 * mgc_reach_tol.h -- when does a residual arc, or a residual t-link, count as OPEN at a rounding tolerance?  The one statement of the
 * rule behind mgc_cut_sets_tol, for the kernels (mgc_reach_tol_ops.inl) and for host code alike.
 *
 * A floating-point solve leaves residuals of a few ulp, or of DBL_MIN next to weights of order 1, that are 0.0 under another order
 * of the same additions.  Whether such an arc is open is an artefact of the route the solve took, so it is judged against the size of
 * the numbers it was computed from:
 *
 *   scale(v)  = the largest  rcap(u -> w) + rcap(w -> u)  over the arc pairs at v whose two ends are voxels of the volume
 *               (the pair's capacity as built, whatever flow it carries: the excess of v is a sum of flows of that size)
 *   arc u -> v    open at tol  iff  rcap > 0  and  rcap > tol * max(scale(u), scale(v))                     (oracle/cutcheck.c's rule)
 *   t-link of v   open at tol  iff  cap > tol * max(|tr0(v)|, scale(v)),  cap = excess(v) (source side) or sink(v) (sink side)
 *
 * tol = 0 is the exact rule: open iff the residual is > 0.
 */
#ifndef MGC_REACH_TOL_H
#define MGC_REACH_TOL_H

#include "mgc_common.h"

MGC_HD double mgc_tol_max(double a, double b) { return a > b ? a : b; }

/* what one arc pair contributes to the scale of its two ends */
MGC_HD double mgc_tol_pair(double there, double back) { return there + back; }

MGC_HD bool mgc_tol_arc_open(double rcap, double tol, double scale_u, double scale_v)
{
    return rcap > 0.0 && rcap > tol * mgc_tol_max(scale_u, scale_v);
}

/* cap: what the voxel still holds of its link (excess: from the source; sink: towards the sink); tr0: the merged t-link as built */
MGC_HD bool mgc_tol_tlink_open(double cap, double tol, double tr0, double scale)
{
    return cap > 0.0 && cap > tol * mgc_tol_max(tr0 < 0.0 ? -tr0 : tr0, scale);
}

#endif /* MGC_REACH_TOL_H */
