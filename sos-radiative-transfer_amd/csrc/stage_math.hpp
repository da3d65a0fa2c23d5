// Arithmetic shared by the stage kernels of beam.hip, emission.hip, profile.hip and profile_view.hip: the profile kernels have
// the bits of the kernels they generalise only while the files evaluate these expressions alike, so they live in one place.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// phi(y) = (1 - e^{-y}) / y, phi(0) = 1: the mean of e^{-y s} over s in [0, 1].  expm1 keeps every bit next to y = 0, where a
// direction's attenuation and the beam's cancel (the closed forms of the coded first order switch to a limit form there).
__device__ __forceinline__ double phi1(double y) { return y == 0.0 ? 1.0 : -expm1(-y) / y; }

// The Planck radiance is linear in tau between two levels and attenuated exactly: with x = Delta / a, E = e^{-x}, A = (1 - E) / x
// the row the sweep arrives at weighs w0 = 1 - A and the row it leaves w1 = A - E (both 0 at x = 0).  Both differences cancel at
// small x; below 0.25 the alternating series
//     w0 = sum_{n>=1} (-1)^{n+1} x^n / (n+1)!,   w1 = sum_{n>=1} (-1)^{n+1} n x^n / (n+1)!
// is summed to 12 terms (the first term dropped is 0.25^13 / 14! = 2e-19): the rule of SOSRT_VIEW_QUAD_LINEAR (view.hip).
constexpr double kLinSeries = 0.25;
__device__ __forceinline__ void linear_weights(double x, double E, double& w0, double& w1) {
    if (x < kLinSeries) {
        constexpr double f[13] = {1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                                  1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0};
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int n = 12; n >= 1; --n) {                      // Horner, innermost term first
            s0 = f[n - 1] - x * s0;
            s1 = n * f[n - 1] - x * s1;
        }
        w0 = x * s0;
        w1 = x * s1;
    } else {
        const double a = (1 - E) / x;
        w0 = 1 - a;
        w1 = a - E;
    }
}

// zone of row t of a column (nz <= kMaxZones ascending first rows)
__device__ __forceinline__ int zone_of(const int* zr0, int nz, int t) {
    int z = 0;
    while (z + 1 < nz && t >= zr0[z + 1]) ++z;
    return z;
}

// emission coefficient of row t (zone z) of column b under per-level weights:
//   eps_t = 1 - (omega_atm w_atm,t f_atm + omega_aer w_aer,t f_aer)        (f of spec:149; clear zone: 1 - omega_atm w_atm,t)
// wat = omega_atm w_atm,t; wr_all[i] the row's aerosol weight, read in an aerosol zone only.  k_emission_profile (profile.hip)
// spells the same expression in its prologue: calling this there changed that kernel's register allocation, and its assembly
// is kept as DESIGN section 29 measured it
__device__ __forceinline__ double row_eps(const ColScalars& sc, int b, int z, double wat, double da, const double* __restrict__ wr_all,
                                          size_t i) {
    double eps = 1.0 - wat;
    if (sc.zmix[(size_t)b * kMaxZones + z]) {
        const double dr = sc.zdtr[(size_t)b * kMaxZones + z];
        const double wrt = sc.zwr[(size_t)b * kMaxZones + z] * wr_all[i];
        eps = 1.0 - (wat * (da / (da + dr)) + wrt * (dr / (da + dr)));
    }
    return eps;
}

}  // namespace sosrt
