// Brightness temperature of a band-summed radiance (include/sosrt.h): per output element the temperature T at
// which f_c(T) = sum_k w[k][c] B_k(T) equals the radiance, B_k the band radiance of the Planck stage (planck_math.hpp).  Device
// code and its launcher; tests/band_view_np.py is the NumPy model, written from the definition in DESIGN and not from this file.
#include <hip/hip_runtime.h>

#include "brightness.hpp"
#include "planck_math.hpp"

namespace sosrt {

namespace {

constexpr double kBracketLo = 1.0, kBracketHi = 1e5;    // kelvin
constexpr double kStart = 250.0;
constexpr double kStop = 1e-9;                          // the accepted Newton step that ends the iteration, relative to T

// x^4 / (e^x - 1), the term of dB/dT at a band edge; 0 at x = 0 (its limit), and 0 where e^x overflows
__device__ __forceinline__ double slope_term(double x) {
    const double x2 = x * x;
    return x > 0.0 ? (x2 * x2) / expm1(x) : 0.0;
}

// f = sum_k w_k B_k(T) and df = sum_k w_k dB_k/dT, k ascending; dB/dT = 4 B / T + (2 k^4 / h^3 c^2) T^3 [x_lo^4 / (e^x_lo - 1) -
// x_hi^4 / (e^x_hi - 1)].  `w` points at the lane's column in the staged weights, stride `ncol`.
__device__ __forceinline__ void channel(double T, int K, int ncol, const double* w, const BandEdges& e, double& f, double& df) {
    const double t3 = (kRadiance * T) * (T * T);
    double a = 0.0, b = 0.0;
    for (int k = 0; k < K; ++k) {
        const double lo = e.lo[k], hi = e.hi[k], wk = w[k * ncol];
        const double B = planck_band(T, lo, hi);
        const double dB = 4.0 * B / T + t3 * (slope_term((kC2 * lo) / T) - slope_term((kC2 * hi) / T));
        a += wk * B;
        b += wk * dB;
    }
    f = a;
    df = b;
}

// One wave per workgroup, one lane per element i = c M + m.  The weights [K] of the columns the workgroup's 64 elements lie in
// (at most `ncol`) are staged in LDS first: lanes of one column then read one address (a broadcast), lanes of neighbouring columns
// neighbouring addresses.  The band edges come by value and are read through the scalar path (k is wave-uniform).  The lanes of
// the wave iterate while any of them is live; a lane that has stopped holds its value.
__global__ __launch_bounds__(kBrightnessBlock) void k_brightness(size_t CM, int C, int M, int K, int ncol, BandEdges edges,
                                                                 const double* __restrict__ weight,
                                                                 const double* __restrict__ radiance, double* T_out) {
    extern __shared__ double s_w[];                     // [K][ncol]
    const size_t i0 = (size_t)blockIdx.x * kBrightnessBlock;
    const size_t c0 = i0 / (size_t)M;
    for (int j = threadIdx.x; j < K * ncol; j += kBrightnessBlock) {
        const int k = j / ncol;
        const size_t c = c0 + (size_t)(j - k * ncol);
        s_w[j] = c < (size_t)C ? (weight ? weight[(size_t)k * C + c] : 1.0) : 0.0;
    }
    __syncthreads();
    const size_t i = i0 + threadIdx.x;
    const bool in = i < CM;
    const double* w = s_w + (in ? (int)(i / (size_t)M - c0) : 0);
    const double R = in ? radiance[i] : 0.0;
    // the element has a root: the radiance is finite and > 0, no weight of the column is negative (or NaN), not all are zero ..
    double wsum = 0.0;
    bool bad = false;
    for (int k = 0; k < K; ++k) {
        const double wk = w[k * ncol];
        bad |= !(wk >= 0.0);
        wsum += wk;
    }
    bool live = in && !bad && wsum > 0.0 && R > 0.0 && R < __builtin_inf();
    double a = kBracketLo, b = kBracketHi, f, df;
    // .. and the radiance lies strictly between the channel's values at the ends of the bracket
    if (live) {
        channel(a, K, ncol, w, edges, f, df);
        live = f < R;
    }
    if (live) {
        channel(b, K, ncol, w, edges, f, df);
        live = R < f;
    }
    // Newton on ln f in u = 1 / T (close to linear in the Wien regime), safeguarded by the bracket [a, b], which every evaluation
    // tightens; an iterate that is not finite or leaves the closed bracket is replaced by the bracket's geometric mean.  The first
    // accepted Newton step with |dT| <= 1e-9 T is applied and ends the iteration; what has not stopped after 40 is NaN.
    double T = kStart, result = __builtin_nan("");
    for (int it = 0; it < kBrightnessIterations && __any(live); ++it) {
        if (live) {
            channel(T, K, ncol, w, edges, f, df);
            if (f < R) a = T;
            else if (f > R) b = T;
            double Tn = 1.0 / (1.0 / T + (log(f / R) * f) / ((T * T) * df));
            const bool newton = Tn >= a && Tn <= b;       // (false for NaN; an infinity is outside the bracket)
            if (!newton) Tn = sqrt(a * b);
            const double step = fabs(Tn - T);
            T = Tn;
            if (newton && step <= kStop * T) {
                result = T;
                live = false;
            }
        }
    }
    if (in) T_out[i] = result;
}

}  // namespace

void launch_brightness_temperature(hipStream_t s, int C, int K, int M, const BandEdges& e, const double* weight,
                                   const double* radiance, double* T_out) {
    const size_t CM = (size_t)C * M;
    const int ncol = brightness_columns(C, M);
    k_brightness<<<(unsigned)((CM + kBrightnessBlock - 1) / kBrightnessBlock), kBrightnessBlock, (size_t)K * ncol * sizeof(double), s>>>(
        CM, C, M, K, ncol, e, weight, radiance, T_out);
}

}  // namespace sosrt
