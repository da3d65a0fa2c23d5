// Band integration (include/sosrt.h): launchers of bands.hip.  Two stages beside the solve: Planck band
// radiances from temperatures, and the weighted sum of per-point arrays over the spectral points of a batch laid out point-major
// (b = k C + c).  Neither reads the handle's columns; both write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

namespace sosrt {

constexpr int kBandsPerLaunch = 64;    // band edges travel by value (1 KiB of the argument block); more bands take several launches
constexpr int kPlanckBlock = 256;      // lanes of a workgroup at most; more than 256 levels + 1 are walked in strides
constexpr int kReduceBlock = 256;

struct BandEdges {                     // cm^-1; entry j is band k0 + j of the launch
    double lo[kBandsPerLaunch];
    double hi[kBandsPerLaunch];
};

// planck [nk][C][L], planck_surface [nk][C], scale [nk][C] or null (normalise = 0): the nk <= kBandsPerLaunch bands of `e`
void launch_planck_bands(hipStream_t s, int C, int nk, int L, const double* T, const double* T_surface, const BandEdges& e,
                         int normalise, double* planck, double* planck_surface, double* scale);
// out [C][M] = (accumulate ? out : 0) + sum over k ascending of (w[k][c] s[k][c]) x[k][c][m], one fused multiply-add per k
void launch_band_reduce(hipStream_t s, int C, int K, int M, const double* weight, const double* scale, const double* x,
                        double* out, int accumulate);

}  // namespace sosrt
