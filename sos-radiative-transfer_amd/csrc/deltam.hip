// Delta-M scaling of a tabulated phase function, gfx950, fp64.
//
//   k_phase_moments_part    one workgroup per (chunk of 256 table intervals, table), one interval per thread: the four Gauss-Legendre
//                           nodes of the interval keep their P_{l-1}, P_l and weight * p in registers, the loop runs over l, and per l
//                           the wave's sum goes to LDS -- one accumulator per thread, whatever lmax.  The table is read once.
//   k_phase_moments_finish  one workgroup per table, one thread per l: the chunks' sums in ascending order, divided by the l = 0 sum.
//   k_delta_m_coef          c_l (2l + 1) of a table, once; f = chi[order].
//   k_delta_m_table         one abscissa per thread, the series in ascending l with the coefficients as wave-uniform loads.
//
// No floating-point atomics: every sum has an order that ntab and lmax fix, and table s of a batch is the work of the workgroups
// (., s) alone, so it has the bits of its single call.
#include "deltam.hpp"

namespace sosrt {

namespace {

// 4-node Gauss-Legendre on [-1, 1]: nodes ascending
__device__ constexpr double kGLx[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
__device__ constexpr double kGLw[4] = {0.34785484513745385, 0.6521451548625461, 0.6521451548625461, 0.34785484513745385};

// abscissa i of the table: the caller's, or np.linspace(-1, 1, ntab) as sosrt_phase_table_dev writes it (the product and the sum
// rounded one after the other, the last point set to 1)
__device__ __forceinline__ double abscissa(const double* __restrict__ tab_mu, int ntab, double step, int i) {
    if (tab_mu) return tab_mu[i];
    return i == ntab - 1 ? 1.0 : __dadd_rn(__dmul_rn((double)i, step), -1.0);
}

// P_{l+1} = a_l x P_l - b_l P_{l-1}, a_l = (2l + 1) / (l + 1), b_l = l / (l + 1): the one recurrence of both kernels, its
// constants formed once per workgroup
__device__ __forceinline__ void recurrence_tables(int lmax, double* s_a, double* s_b) {
    for (int l = threadIdx.x; l <= lmax; l += blockDim.x) {
        s_a[l] = (2.0 * l + 1.0) / (l + 1.0);
        s_b[l] = (double)l / (l + 1.0);
    }
    __syncthreads();
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kDeltaMBlock) void k_phase_moments_part(const double* __restrict__ tab_mu, const double* __restrict__ tab_p,
                                                                     int ntab, double step, int lmax, double* __restrict__ part) {
    constexpr int NW = kDeltaMBlock / 64;
    __shared__ double s_a[kDeltaMMaxOrder + 1], s_b[kDeltaMMaxOrder + 1], s_w[NW][kDeltaMMaxOrder + 1];
    const int tid = threadIdx.x, i = blockIdx.x * kDeltaMBlock + tid;
    const double* p = tab_p + (size_t)blockIdx.y * ntab;
    recurrence_tables(lmax, s_a, s_b);
    double x[4], q[4], P[4], Pm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = 0; q[k] = 0; P[k] = 1; Pm[k] = 0; }
    if (i < ntab - 1) {
        const double x0 = abscissa(tab_mu, ntab, step, i), x1 = abscissa(tab_mu, ntab, step, i + 1);
        const double p0 = p[i], p1 = p[i + 1];
        const double mid = 0.5 * (x0 + x1), half = 0.5 * (x1 - x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = mid + half * kGLx[k];
            q[k] = half * kGLw[k] * (p0 + (x[k] - x0) / (x1 - x0) * (p1 - p0));      // the builders' interpolant (phasefn.hpp)
        }
    }
    for (int l = 0; l <= lmax; ++l) {
        const double t = wave_sum(((q[0] * P[0] + q[1] * P[1]) + q[2] * P[2]) + q[3] * P[3]);
        if ((tid & 63) == 0) s_w[tid >> 6][l] = t;
        const double a = s_a[l], b = s_b[l];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double n = a * x[k] * P[k] - b * Pm[k];
            Pm[k] = P[k]; P[k] = n;
        }
    }
    __syncthreads();
    double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (lmax + 1);
    for (int l = tid; l <= lmax; l += kDeltaMBlock) o[l] = ((s_w[0][l] + s_w[1][l]) + s_w[2][l]) + s_w[3][l];
}

__global__ __launch_bounds__(kDeltaMBlock) void k_phase_moments_finish(const double* __restrict__ part, int chunks, int lmax,
                                                                       double* __restrict__ chi, double* __restrict__ norm) {
    const int s = blockIdx.x, l = threadIdx.x;
    if (l > lmax) return;
    const double* q = part + (size_t)s * chunks * (lmax + 1);
    double sum = 0, sum0 = 0;
    for (int c = 0; c < chunks; ++c) {
        sum += q[(size_t)c * (lmax + 1) + l];
        sum0 += q[(size_t)c * (lmax + 1)];
    }
    chi[(size_t)s * (lmax + 1) + l] = sum / sum0;
    if (l == 0 && norm) norm[s] = 0.5 * sum0;
}

__global__ __launch_bounds__(kDeltaMBlock) void k_delta_m_coef(const double* __restrict__ chi, int lmax, int order,
                                                               double* __restrict__ coef, double* __restrict__ f_out) {
    const int s = blockIdx.x, l = threadIdx.x;
    const double* c = chi + (size_t)s * (lmax + 1);
    const double f = c[order];
    if (l < order) coef[(size_t)s * order + l] = (2.0 * l + 1.0) * ((c[l] - f) / (1.0 - f));
    if (l == 0 && f_out) f_out[s] = f;
}

// (coef and the abscissae as __restrict__ arguments of their own: the stores to out leave them alone, which keeps the
// wave-uniform loads of the coefficients scalar)
__global__ __launch_bounds__(kDeltaMBlock) void k_delta_m_table(const double* __restrict__ coef, const double* __restrict__ tab_mu,
                                                                int ntab, double step, int order, double* __restrict__ out) {
    __shared__ double s_a[kDeltaMMaxOrder + 1], s_b[kDeltaMMaxOrder + 1];
    recurrence_tables(order - 1, s_a, s_b);
    const int i = blockIdx.x * kDeltaMBlock + threadIdx.x;
    if (i >= ntab) return;
    const double* c = coef + (size_t)blockIdx.y * order;
    const double x = abscissa(tab_mu, ntab, step, i);
    double acc = 0, P = 1, Pm = 0;
    for (int l = 0; l < order; ++l) {
        acc += c[l] * P;
        const double n = s_a[l] * x * P - s_b[l] * Pm;
        Pm = P; P = n;
    }
    out[(size_t)blockIdx.y * ntab + i] = acc;
}

}  // namespace

void launch_phase_moments(hipStream_t s, int S, const double* tab_mu, const double* tab_p, int ntab, int lmax, double* part,
                          double* chi, double* norm) {
    const int chunks = deltam_chunks(ntab);
    const double step = 2.0 / (ntab - 1);
    hipLaunchKernelGGL(k_phase_moments_part, dim3(chunks, S), dim3(kDeltaMBlock), 0, s, tab_mu, tab_p, ntab, step, lmax, part);
    hipLaunchKernelGGL(k_phase_moments_finish, dim3(S), dim3(kDeltaMBlock), 0, s, part, chunks, lmax, chi, norm);
}

void launch_phase_delta_m(hipStream_t s, int S, const double* chi, int lmax, int order, const double* tab_mu, int ntab,
                          double* coef, double* tab_out, double* f_out) {
    const double step = 2.0 / (ntab - 1);
    hipLaunchKernelGGL(k_delta_m_coef, dim3(S), dim3(kDeltaMBlock), 0, s, chi, lmax, order, coef, f_out);
    hipLaunchKernelGGL(k_delta_m_table, dim3((ntab + kDeltaMBlock - 1) / kDeltaMBlock, S), dim3(kDeltaMBlock), 0, s, coef, tab_mu, ntab,
                       step, order, tab_out);
}

}  // namespace sosrt
