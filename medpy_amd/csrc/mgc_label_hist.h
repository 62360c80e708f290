/*
 * mgc_label_hist.h -- the run merging of mgc_label_histograms, stated once.  k_label_hist gives a thread a GROUP of
 * MGC_LH_GROUP consecutive voxels along the fastest axis; neighbouring voxels mostly share label and bin, so the group is counted
 * run by run: one add of the run's length per maximal run of equal keys instead of one add per voxel.  mgc_label_hist_runs is
 * MGC_HD: the kernel of mgc_label_hist_ops.inl and host code compile the same lines (tests/hostsim/label_hist_main.cpp).  Nothing
 * here needs HIP.
 */
#ifndef MGC_LABEL_HIST_H
#define MGC_LABEL_HIST_H

#include <stdint.h>

#include "mgc_common.h"

#define MGC_LH_GROUP 16 /* voxels of a thread's group: one 16-byte load of the label plane */

/* the slot of a voxel in the block of 2 * nbins counters: the fg histogram first (label not zero), the bg histogram behind it */
MGC_HD uint32_t mgc_label_hist_key(bool fg, int64_t bin, int64_t nbins) { return (uint32_t)((fg ? 0 : nbins) + bin); }

/* add(key, run) once per maximal run of equal keys among key[0 .. count), in order; 0 <= count <= MGC_LH_GROUP (a group cut short
 * by the end of the volume has fewer).  The runs' lengths sum to count.  Every index into key is a constant once the loop is
 * unrolled, so the keys stay in registers on the device. */
template <class Add>
MGC_HD void mgc_label_hist_runs(const uint32_t (&key)[MGC_LH_GROUP], int count, Add&& add)
{
    uint32_t cur = 0u, run = 0u;
#pragma unroll
    for (int i = 0; i < MGC_LH_GROUP; ++i) {
        if (i >= count) break;
        if (run && key[i] == cur) {
            ++run;
        } else {
            if (run) add(cur, run);
            cur = key[i];
            run = 1u;
        }
    }
    if (run) add(cur, run);
}

#endif /* MGC_LABEL_HIST_H */
