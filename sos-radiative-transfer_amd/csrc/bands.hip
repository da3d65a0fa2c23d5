// Band integration (include/sosrt.h): Planck band radiances from temperatures, and the weighted sum over the
// spectral points of a batch.  Device code and its launchers; tests/bands_np.py is the NumPy model of both, written from the
// definitions in DESIGN and not from this file.
#include <hip/hip_runtime.h>

#include "bands.hpp"

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

// One workgroup per (band, column); lane i takes level i (i = L: the surface), in strides of the workgroup where L + 1 exceeds it.
// The raw values go to the outputs; with `normalise` the maximum is reduced in the wave, then across the waves through LDS in a
// fixed order, and every lane divides the values it wrote itself.
__global__ __launch_bounds__(kPlanckBlock) void k_planck_bands(int C, int L, const double* __restrict__ T_all,
                                                               const double* __restrict__ T_surface, BandEdges edges, int normalise,
                                                               double* planck, double* planck_surface, double* scale) {
    __shared__ double s_max[kPlanckBlock / 64];
    const int c = blockIdx.x, j = blockIdx.y;
    const double lo = edges.lo[j], hi = edges.hi[j];
    const size_t kc = (size_t)j * C + c;
    const double* T = T_all + (size_t)c * L;
    double* out = planck + kc * L;
    double m = 0.0;
    for (int i = threadIdx.x; i <= L; i += blockDim.x) {
        const double b = planck_band(i < L ? T[i] : T_surface[c], lo, hi);
        if (i < L) out[i] = b;
        else planck_surface[kc] = b;
        m = fmax(m, b);
    }
    if (!normalise) {
        if (scale && threadIdx.x == 0) scale[kc] = 1.0;
        return;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_max[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, s_max[w]);
    for (int i = threadIdx.x; i <= L; i += blockDim.x) {
        if (i < L) out[i] = out[i] / m;
        else planck_surface[kc] = planck_surface[kc] / m;
    }
    if (threadIdx.x == 0) scale[kc] = m;
}

// One lane per element i = c M + m of the output; the K loads of a lane are independent of its chain of fused multiply-adds, and
// consecutive lanes read consecutive doubles of x[k].  The product w s is rounded once, then acc = fma(w s, x, acc), k ascending:
// the result does not depend on the launch geometry, nor on how K is split over calls with `accumulate`.
__global__ __launch_bounds__(kReduceBlock) void k_band_reduce(size_t CM, int C, int M, int K, const double* __restrict__ weight,
                                                              const double* __restrict__ scale, const double* __restrict__ x,
                                                              double* out, int accumulate) {
    const size_t i = (size_t)blockIdx.x * kReduceBlock + threadIdx.x;
    if (i >= CM) return;
    const size_t c = i / (size_t)M;
    double acc = accumulate ? out[i] : 0.0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const size_t kc = (size_t)k * C + c;
        const double w = weight ? weight[kc] : 1.0, s = scale ? scale[kc] : 1.0;
        const double ws = w * s;
        acc = fma(ws, x[(size_t)k * CM + i], acc);
    }
    out[i] = acc;
}

}  // namespace

void launch_planck_bands(hipStream_t s, int C, int nk, int L, const double* T, const double* T_surface, const BandEdges& e,
                         int normalise, double* planck, double* planck_surface, double* scale) {
    const int waves = (L + 1 + 63) / 64;
    const int block = waves * 64 < kPlanckBlock ? waves * 64 : kPlanckBlock;
    k_planck_bands<<<dim3(C, nk), block, 0, s>>>(C, L, T, T_surface, e, normalise, planck, planck_surface, scale);
}

void launch_band_reduce(hipStream_t s, int C, int K, int M, const double* weight, const double* scale, const double* x, double* out,
                        int accumulate) {
    const size_t CM = (size_t)C * M;
    k_band_reduce<<<(unsigned)((CM + kReduceBlock - 1) / kReduceBlock), kReduceBlock, 0, s>>>(CM, C, M, K, weight, scale, x, out,
                                                                                             accumulate);
}

}  // namespace sosrt
