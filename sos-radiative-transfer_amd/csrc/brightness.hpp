// Brightness temperature of a band-summed radiance (include/sosrt.h): launcher of brightness.hip.  The inverse
// of the Planck stage: per output element the temperature at which the weighted sum of K band radiances equals the radiance given.
// A stage beside the solve; it reads its inputs and writes its output only.
#pragma once
#include <hip/hip_runtime.h>

#include "bands.hpp"

namespace sosrt {

constexpr int kBrightnessBlock = 64;   // one wave per workgroup: its lanes iterate while any of them is live
constexpr int kBrightnessIterations = 40;

// columns whose weights a workgroup of kBrightnessBlock consecutive elements i = c M + m stages in LDS, at most
inline int brightness_columns(int C, int M) {
    const int span = (kBrightnessBlock - 1) / M + 2;
    const int n = span < kBrightnessBlock ? span : kBrightnessBlock;
    return n < C ? n : C;
}

// T_out [C][M] from radiance [C][M], weight [K][C] or null (ones), the K <= kBandsPerLaunch bands of `e`
void launch_brightness_temperature(hipStream_t s, int C, int K, int M, const BandEdges& e, const double* weight,
                                   const double* radiance, double* T_out);

}  // namespace sosrt
