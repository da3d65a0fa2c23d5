// Thermal emission (include/sosrt.h): launchers of emission.hip.  A stage beside the solve: the kernels read
// the columns' scalars and zone tables as sosrt_set_columns* uploaded them (ColScalars) and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

constexpr int kEmissionMaxL = 2048;    // two rows of L doubles in LDS (tau and the Planck profile), beside N surface values; one
                                       // workgroup per column, one lane per direction pair: sosrt_create's N <= 1024 is its size limit

// I0 [B][L][D]: the emitted field on the grid's directions; planck [B][L], planck_surface [B], emissivity [B] or null (1 - rho)
void launch_emission(hipStream_t s, const Grid& g, int B, ColScalars sc, int surface, const double* tau, const double* planck,
                     const double* planck_surface, const double* emissivity, double* I0);
// out [B][nlev_all][2V] (offset to the first level of lv): the same sweeps at the view cosines; specular or no surface
void launch_emission_view(hipStream_t s, int B, int V, int L, int nlev_all, ColScalars sc, int surface, const double* tau,
                          const double* planck, const double* planck_surface, const double* emissivity, const ViewMu& mu,
                          const ViewLevels& lv, double* out);
// launch_epilogue without the two beam terms
void launch_epilogue_emission(hipStream_t s, const Grid& g, const double* w, int B, ColScalars sc, const double* tau,
                              const double* I, const double* z_profile, const EpilogueOut& out);

}  // namespace sosrt
