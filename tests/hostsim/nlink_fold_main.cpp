/*
 * nlink_fold_main.cpp -- TEST ONLY.  The per-arc rule of a warm update of the boundary term (medpy_amd/csrc/mgc_nlink_fold.h) as a
 * stand-alone program, so that it can also be built with -fsanitize=address,undefined and run on the CPU.  Exit status 0 = every
 * property held; else the failed ones are printed (the first few cases each).
 */
#include <math.h>
#include <stdio.h>

#include <limits>
#include <random>

#include "../../medpy_amd/csrc/mgc_nlink_fold.h"

static int failures = 0;

static void expect(bool ok, const char* what, double c, double c1, double phi)
{
    if (ok) return;
    if (++failures <= 20) printf("FAILED: %s (c = %.17g, c' = %.17g, flow = %.17g)\n", what, c, c1, phi);
}

/* capacities of the boundary terms: from the floor sys.float_info.min up to the marker weight, log-uniform, the two ends included */
static double capacity(std::mt19937_64& rng)
{
    const double lo = log(1e-308), hi = log(65535.0);
    const int pick = (int)(rng() % 16);
    if (pick == 0) return 1e-308;
    if (pick == 1) return 65535.0;
    if (pick == 2) return 1.0;
    return exp(lo + (hi - lo) * std::uniform_real_distribution<double>(0.0, 1.0)(rng));
}

/* a flow the arc (capacity c) can carry: either sign, saturated either way, none, anything between */
static double flow_on(std::mt19937_64& rng, double c)
{
    switch (rng() % 6) {
    case 0: return c;
    case 1: return -c;
    case 2: return 0.0;
    default: return c * std::uniform_real_distribution<double>(-1.0, 1.0)(rng);
    }
}

int main()
{
    std::mt19937_64 rng(20240611);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 400000; ++k) {
        const double c = capacity(rng), phi = flow_on(rng, c);
        const double r0 = c - phi; /* what the solver holds: in [0, 2c] */
        bool clamped = true;
        /* unchanged capacity: the residual keeps its bits, nothing comes back */
        {
            double r = r0;
            const double back = mgc_nlink_fold(c, c, &r, &clamped);
            expect(mgc_same_bits(r, r0) && back == 0.0 && !clamped, "an unchanged capacity touches nothing", c, c, phi);
        }
        const double c1 = (k & 1) ? capacity(rng) : c * exp(std::uniform_real_distribution<double>(-3.0, 3.0)(rng));
        if (mgc_same_bits(c, c1) || !(c1 > 0.0) || !isfinite(c1)) continue;
        double r = r0;
        const double back = mgc_nlink_fold(c, c1, &r, &clamped);
        const double seen = c - r0; /* the flow as the rule sees it */
        expect(r >= 0.0 && r <= 2.0 * c1, "0 <= r' <= 2 c'", c, c1, phi);
        if (seen >= -c1 && seen <= c1) {
            expect(back == 0.0 && !clamped, "a flow inside the new bounds gives nothing back", c, c1, phi);
        } else {
            expect(clamped && back != 0.0 && (back > 0.0) == (seen > 0.0), "a flow outside the new bounds comes back with its sign", c, c1, phi);
            expect(r == (seen > 0.0 ? 0.0 : 2.0 * c1), "a clamped arc is saturated one way or the other", c, c1, phi);
        }
    }
    /* dyadic inputs: every operation of the rule is exact, so the two ends of a pair -- each from its own residual -- hand back equal
     * and opposite amounts and the pair keeps r'_ab + r'_ba == 2 c' */
    for (int k = 0; k < 400000; ++k) {
        const double c = (double)(1 + rng() % 4096) / 64.0, c1 = (double)(1 + rng() % 4096) / 64.0;
        const int64_t steps = (int64_t)(c * 64.0);
        double phi = (double)((int64_t)(rng() % (uint64_t)(2 * steps + 1)) - steps) / 64.0;
        if (rng() % 5 == 0) phi = (rng() & 1) ? c : -c;
        double rab = c - phi, rba = c + phi;
        expect(rab + rba == 2.0 * c, "(the case conserves the pair exactly)", c, c1, phi);
        bool ca, cb;
        const double back_a = mgc_nlink_fold(c, c1, &rab, &ca), back_b = mgc_nlink_fold(c, c1, &rba, &cb);
        expect(back_a == -back_b && ca == cb, "the two ends hand back equal and opposite amounts", c, c1, phi);
        expect(c == c1 || rab + rba == 2.0 * c1, "r'_ab + r'_ba == 2 c'", c, c1, phi);
        expect(rab >= 0.0 && rba >= 0.0, "no negative residual", c, c1, phi);
    }
    /* a capacity that is not a number (0 / 0 of a linear term on a constant image): not residual, carries nothing, gives nothing back */
    {
        bool clamped;
        double r = nan;
        expect(mgc_nlink_fold(nan, nan, &r, &clamped) == 0.0 && !clamped && r != r, "NaN -> NaN is an unchanged capacity", nan, nan, 0.0);
        r = nan;
        const double back = mgc_nlink_fold(nan, 0.5, &r, &clamped);
        expect(back == 0.0 && r == 0.5 && !clamped, "NaN -> c': the arc starts without flow", nan, 0.5, 0.0);
        r = 0.25;
        const double back2 = mgc_nlink_fold(0.5, nan, &r, &clamped);
        expect(back2 == 0.25 && r != r && clamped, "c -> NaN: the flow comes back, the arc is not residual", 0.5, nan, 0.25);
    }
    if (failures) printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
