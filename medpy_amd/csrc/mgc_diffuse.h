/*
 * mgc_diffuse.h -- anisotropic diffusion (Perona-Malik / Tukey; mgc_diffuse_image, mgc_diffuse), stated once: the
 * conduction, the flux across one face, the update of one voxel, and the check of the arguments, made before anything is written.
 * The functions are MGC_HD: the kernel of mgc_diffuse_ops.inl and host code compile the same lines.  Nothing here needs HIP:
 * mgc_kernels.hip includes it, and a stand-alone host program can (tests/hostsim/diffusion_main.cpp).
 *
 * u is the image as float32 (numpy.array(img, dtype=float32): every dtype converted directly, rounded to nearest), axes
 * i = 0 .. n-1 in array order, extents N_i, n = 1 .. 3.  Constants, prepared on the host (mgc_ad_prepare):
 *   kappa   = f32(kappa)          kappa_s = f32(kappa * 2**0.5), the product in f64
 *   gamma   = f32(gamma)          s_i     = f32(spacing_i), 1 when none is given
 * One iteration, every operation an IEEE float32 operation rounded on its own (build with -ffp-contract=off; true division):
 *   d_i(p)   = u(p + e_i) - u(p)        if p_i < N_i - 1, else +0
 *   q        = d_i(p) / kappa           (option 3: d_i(p) / kappa_s)
 *   c        = f32(exp(-(q * q))) / s_i                                         option 1
 *            = (1 / (1 + q * q)) / s_i                                          option 2
 *            = (0.5 * (t * t)) / s_i, t = 1 - q * q, if |d_i(p)| <= kappa_s, else 0     option 3
 *   phi_i(p) = c * d_i(p)
 *   m_i(p)   = phi_i(p) - phi_i(p - e_i)  if p_i >= 1, else phi_i(p)
 *   u'(p)    = u(p) + gamma * ((m_0 + m_1) + m_2)      axes added first to last; two terms in 2-D, one in 1-D
 * Every voxel reads iteration k - 1 only: tiling, launch order and recomputation in halos cannot change a bit.  Options 2 and 3
 * use + - * / and comparisons only and equal medpy.filter.smoothing.anisotropic_diffusion (NumPy, float32) value for value.
 * Option 1's exp is (float)exp((double)x) here and on the device: a definition of ours, close to NumPy's float32 exp, not equal.
 * Two differences from the reference: kappa, gamma and the spacings go through float() first (the reference computes in float64
 * when handed NumPy float64 scalars); voxels that are not finite are neither refused nor specified.
 */
#ifndef MGC_DIFFUSE_H
#define MGC_DIFFUSE_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "mgc_common.h"

/* the brick of one workgroup of k_diffuse (z, y, x): mirrored in tests/diffusion_cases.py */
#define MGC_AD_BZ 8
#define MGC_AD_BY 8
#define MGC_AD_BX 64

#define MGC_AD_OK 0
#define MGC_AD_INVALID 1

/* the constants of a call; s[] by internal axis: 0 = z (array axis n - 3), 1 = y, 2 = x (the last array axis) */
struct MgcDiffuse {
    float kappa, kappa_s, gamma;
    float s[3];
    int option;
    int ndim;
};

/* option 1's exponential: f64 exp, rounded once */
MGC_HD float mgc_ad_exp(float x) { return (float)exp((double)x); }

/* phi = c(d) * d for the difference d across one face along an axis of spacing s */
MGC_HD float mgc_ad_flux(float d, float s, float kappa, float kappa_s, int option)
{
    float c;
    if (option == 1) {
        const float q = d / kappa;
        const float qq = q * q;
        c = mgc_ad_exp(-qq) / s;
    } else if (option == 2) {
        const float q = d / kappa;
        const float qq = q * q;
        const float den = 1.0f + qq;
        c = (1.0f / den) / s;
    } else {
        const float q = d / kappa_s;
        const float qq = q * q;
        const float t = 1.0f - qq;
        const float tt = t * t;
        c = fabsf(d) <= kappa_s ? (0.5f * tt) / s : 0.0f;
    }
    return c * d;
}

/* the forward difference along an axis: u1 = u(p + e_i); inside: p_i < N_i - 1 */
MGC_HD float mgc_ad_diff(float u0, float u1, bool inside) { return inside ? u1 - u0 : 0.0f; }

/* m_i = phi_i(p) - phi_i(p - e_i), or phi_i(p) on the low face of the volume */
MGC_HD float mgc_ad_div(float phi, float phi_lo, bool has_lo) { return has_lo ? phi - phi_lo : phi; }

/* u' from u and the three m (z, y, x = array axes first to last; a 2-D image has my and mx, a 1-D image mx) */
MGC_HD float mgc_ad_update(float u, float gamma, int ndim, float mz, float my, float mx)
{
    float sum;
    if (ndim >= 3) { sum = mz + my; sum = sum + mx; }
    else if (ndim == 2) sum = my + mx;
    else sum = mx;
    const float step = gamma * sum;
    return u + step;
}

/* One voxel from its seven values.  lo[i] / hi[i]: the neighbours at p - e_i / p + e_i (read only where has_lo[i] / has_hi[i]),
 * i by internal axis (0 = z, 1 = y, 2 = x).  What the kernel shares between neighbours this evaluates twice; the numbers are the
 * same. */
MGC_HD float mgc_ad_voxel(const MgcDiffuse& P, float u, const float lo[3], const float hi[3], const bool has_lo[3], const bool has_hi[3])
{
    float m[3];
    for (int i = 0; i < 3; ++i) {
        const float phi = mgc_ad_flux(mgc_ad_diff(u, hi[i], has_hi[i]), P.s[i], P.kappa, P.kappa_s, P.option);
        const float phi_lo = has_lo[i] ? mgc_ad_flux(mgc_ad_diff(lo[i], u, true), P.s[i], P.kappa, P.kappa_s, P.option) : 0.0f;
        m[i] = mgc_ad_div(phi, phi_lo, has_lo[i]);
    }
    return mgc_ad_update(u, P.gamma, P.ndim, m[0], m[1], m[2]);
}

/* The limits of a call: 1 <= ndim <= 3, extents >= 1, niter >= 0, option 1 .. 3, kappa finite and > 0, gamma finite, every
 * spacing finite and > 0.  MGC_AD_OK, or MGC_AD_INVALID with a sentence about the first offender in msg.  Reads only. */
static inline int mgc_ad_check(int ndim, const int64_t* shape, int niter, double kappa, double gamma, const double* spacing, int option, char* msg, size_t msg_len)
{
    if (ndim < 1 || ndim > 3) { snprintf(msg, msg_len, "ndim = %d outside [1, 3]", ndim); return MGC_AD_INVALID; }
    if (!shape) { snprintf(msg, msg_len, "shape NULL"); return MGC_AD_INVALID; }
    for (int i = 0; i < ndim; ++i)
        if (shape[i] < 1) { snprintf(msg, msg_len, "shape[%d] = %lld: every extent must be at least 1", i, (long long)shape[i]); return MGC_AD_INVALID; }
    if (niter < 0) { snprintf(msg, msg_len, "niter = %d must not be negative", niter); return MGC_AD_INVALID; }
    if (option < 1 || option > 3) { snprintf(msg, msg_len, "option = %d outside [1, 3]", option); return MGC_AD_INVALID; }
    if (!isfinite(kappa) || !(kappa > 0.0)) { snprintf(msg, msg_len, "kappa = %g must be finite and > 0", kappa); return MGC_AD_INVALID; }
    if (!isfinite(gamma)) { snprintf(msg, msg_len, "gamma = %g must be finite", gamma); return MGC_AD_INVALID; }
    if (spacing)
        for (int i = 0; i < ndim; ++i)
            if (!isfinite(spacing[i]) || !(spacing[i] > 0.0)) { snprintf(msg, msg_len, "spacing[%d] = %g: the spacing must be finite and positive", i, spacing[i]); return MGC_AD_INVALID; }
    return MGC_AD_OK;
}

/* the constants of a checked call, rounded to float32 as the definition says; dims (z, y, x) with leading extents of 1 */
static inline void mgc_ad_prepare(int ndim, const int64_t* shape, double kappa, double gamma, const double* spacing, int option, MgcDiffuse* P, int64_t dims[3])
{
    P->kappa = (float)kappa;
    P->kappa_s = (float)(kappa * 1.4142135623730951); /* 2 ** 0.5 in f64 */
    P->gamma = (float)gamma;
    P->option = option;
    P->ndim = ndim;
    for (int k = 0; k < 3; ++k) { P->s[k] = 1.0f; dims[k] = 1; }
    for (int i = 0; i < ndim; ++i) {
        dims[3 - ndim + i] = shape[i];
        if (spacing) P->s[3 - ndim + i] = (float)spacing[i];
    }
}

#endif /* MGC_DIFFUSE_H */
