// Band integration (include/sosrt.h): Planck band radiances from temperatures, and the weighted sum over the
// spectral points of a batch.  Device code and its launchers; tests/bands_np.py is the NumPy model of both, written from the
// definitions in DESIGN and not from this file.
#include <hip/hip_runtime.h>

#include "bands.hpp"
#include "planck_math.hpp"      // planck_S, planck_G, planck_band and their constants, shared with brightness.hip

namespace sosrt {

namespace {

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
