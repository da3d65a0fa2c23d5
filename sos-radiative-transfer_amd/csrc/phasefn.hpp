// The phase functions of the azimuth builders and their ring rule, shared by epilogue.hip (k_phase_p0, k_phase_matrix and the
// Fourier modes) and view.hip (the same two at view cosines off the grid).
// Phase-function kinds: isotropic (phase:68), Rayleigh (phase:79), Henyey-Greenstein (phase:141) and a
// tabulated function with the reference's linear interpolation (phase:198-236; fwc:3,173 is its table).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sosrt.h"

namespace sosrt {

struct PhaseFn {
    int kind;
    double g;
    const double* tab_mu;
    const double* tab_p;
    int ntab;
    // p(cos Theta)
    __device__ __forceinline__ double operator()(double c) const {
        if (kind == SOSRT_PHASE_RAYLEIGH) return (3.0 / 4) * (1 + c * c);                    // phase:96
        if (kind == SOSRT_PHASE_HG) {                                                         // phase:158
            const double x = 1 + g * g - 2 * g * c;
            return (1 - g * g) / (x * sqrt(x));
        }
        if (kind == SOSRT_PHASE_TABLE) {                                                      // phase:198-236
            c = fmin(fmax(c, -1.0), 1.0);
            int lo = 0, hi = ntab;                                                            // searchsorted, side='left'
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab_mu[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo == 0) return tab_p[0];
            if (lo >= ntab) return tab_p[ntab - 1];
            const double ml = tab_mu[lo - 1], mh = tab_mu[lo], pl = tab_p[lo - 1], ph = tab_p[lo];
            return pl + (c - ml) / (mh - ml) * (ph - pl);
        }
        return 1.0;
    }
};

// trapz over phi = linspace(0, pi, nphi) of p(cos Theta+) + p(cos Theta-), cos Theta+- = -(a b +- sa sb cos phi)
__device__ __forceinline__ double ring(const PhaseFn& p, double cc, double ss, const double* __restrict__ cosphi,
                                       const double* __restrict__ wphi, int nphi) {
    double acc = 0;
    for (int q = 0; q < nphi; ++q) {
        const double x = ss * cosphi[q];
        acc += wphi[q] * (p(-(cc + x)) + p(-(cc - x)));
    }
    return acc;
}

}  // namespace sosrt
