// Per-level weights at view lanes (include/sosrt.h): launchers of profile_view.hip.  The weights are the
// handle's copies [B][L] of sosrt_set_row_weights_dev; the kernels read the columns' scalars and zone tables as
// sosrt_set_columns* uploaded them (ColScalars) and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_view.hpp"
#include "kernels.hpp"

namespace sosrt {

// out [nset][B][nlev_all][2V] (offset to the first level of lv): launch_view_first_order_beam (beam_view.hpp) with the weights
// in A and Rz, row by row.  Six rows of L doubles in LDS: L <= kProfileMaxL (profile.hpp)
void launch_view_first_order_profile(hipStream_t s, int L, int B, int V, int nset, int nlev_all, ColScalars sc, const double* tau,
                                     const double* sigma, const double* p0a, const double* p0r, const double* w_atm,
                                     const double* w_aer, const ViewMu& mu, const BeamViewLevels& lv, double* out);
// out [B][nlev_all][2V] (offset to the first level of lv): launch_emission_view (emission.hpp) with the weights in the emission
// coefficient, row by row; the levels of lv sorted by row, as the first-order kernel takes them
void launch_emission_view_profile(hipStream_t s, int B, int V, int L, int nlev_all, ColScalars sc, int surface, const double* tau,
                                  const double* planck, const double* planck_surface, const double* emissivity, const double* w_atm,
                                  const double* w_aer, const ViewMu& mu, const BeamViewLevels& lv, double* out);

}  // namespace sosrt
