// Planck band radiance on the device (DESIGN sections 19 and 31): the constants and the three device functions that bands.hip
// (the Planck stage) and brightness.hip (its inverse) both evaluate.  Moved here from bands.hip as they stood; the device code of
// bands.hip is the same instruction for instruction.  Internal linkage: every unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace sosrt {

namespace {

// CODATA 2018 (exact since the 2019 redefinition of the SI), the constants of sosrt/thermal.py
constexpr double kPlanckH = 6.62607015e-34;        // J s
constexpr double kLightC = 299792458.0;            // m / s
constexpr double kBoltzmannK = 1.380649e-23;       // J / K
constexpr double kPi = 3.14159265358979323846;
constexpr double kC2 = 100.0 * kPlanckH * kLightC / kBoltzmannK;             // x = kC2 nu / T, nu in cm^-1
constexpr double kRadiance = 2.0 * ((kBoltzmannK * kBoltzmannK) * (kBoltzmannK * kBoltzmannK)) /
                             ((kPlanckH * kPlanckH * kPlanckH) * (kLightC * kLightC));      // 2 k^4 / (h^3 c^2), W m^-2 sr^-1 K^-4
constexpr double kG0 = (kPi * kPi) * (kPi * kPi) / 15.0;                     // G(0) = pi^4 / 15
constexpr int kTailTerms = 30;

// S(x) = int_0^x t^3 / (e^t - 1) dt = sum c_k x^{k+3}, c_k = B_k / ((k+3) k!), the ten non-zero Bernoulli terms up to k = 16;
// for x < 1 (the next term is 4e-16 x^21)
__device__ __forceinline__ double planck_S(double x) {
    const double u = x * x;
    double p = -1.78404226122241216e-14;
    p = p * u + 7.87208031216745774e-13;
    p = p * u + -3.52279342579166215e-11;
    p = p * u + 1.60590438368216149e-09;
    p = p * u + -1.0 / 13305600.0;
    p = p * u + 1.0 / 272160.0;
    p = p * u + -1.0 / 5040.0;
    p = p * u + 1.0 / 60.0;
    p = p * x + -1.0 / 8.0;
    p = p * x + 1.0 / 3.0;
    return (x * u) * p;
}

// G(x) = int_x^inf t^3 / (e^t - 1) dt = sum_{n=1}^{30} e^{-n x} (x^3 / n + 3 x^2 / n^2 + 6 x / n^3 + 6 / n^4) for x >= 1: one exp,
// the powers e^{-n x} by repeated multiplication, the bracket as a Horner form in 1 / n (constants of the unrolled loop)
__device__ __forceinline__ double planck_G(double x) {
    const double e = exp(-x);
    const double x2 = x * x, a3 = x2 * x, a2 = 3.0 * x2, a1 = 6.0 * x;
    double p = 1.0, g = 0.0;
#pragma unroll
    for (int n = 1; n <= kTailTerms; ++n) {
        const double r = 1.0 / n;
        p *= e;
        g += p * (r * (a3 + r * (a2 + r * (a1 + r * 6.0))));
    }
    return g;
}

// band radiance of a black body at T between the wavenumbers lo < hi (cm^-1), W m^-2 sr^-1; the difference G(x_lo) - G(x_hi) in the
// form that does not cancel.  T <= 0 (and NaN) gives NaN.
__device__ __forceinline__ double planck_band(double T, double lo, double hi) {
    const double xl = (kC2 * lo) / T, xh = (kC2 * hi) / T;
    double d;
    if (xh < 1.0) d = planck_S(xh) - planck_S(xl);
    else if (xl >= 1.0) d = planck_G(xl) - planck_G(xh);
    else d = (kG0 - planck_S(xl)) - planck_G(xh);
    const double t2 = T * T;
    const double b = ((kRadiance * t2) * t2) * d;
    return T > 0.0 ? b : __builtin_nan("");
}

}  // namespace

}  // namespace sosrt
