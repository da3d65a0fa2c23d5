// Pseudo-spherical direct beam at view lanes (include/sosrt.h): launcher of beam_view.hip.  As the kernels of
// beam.hip it reads the columns' scalars and zone tables as sosrt_set_columns* uploaded them (ColScalars) and writes its output only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

// the requested levels of one launch, sorted by row: t ascending, idx the level's place in the caller's list
struct BeamViewLevels {
    int n;
    int t[kViewLevels];
    int idx[kViewLevels];
};

// out [nset][B][nlev_all][2V] (offset to the first level of lv): the first order on the beam path sigma [B][L] at the signed
// lanes (-mu[v], +mu[v]); p0a, p0r [nset][B][2V]
void launch_view_first_order_beam(hipStream_t s, int L, int B, int V, int nset, int nlev_all, ColScalars sc, const double* tau,
                                  const double* sigma, const double* p0a, const double* p0r, const ViewMu& mu,
                                  const BeamViewLevels& lv, double* out);

}  // namespace sosrt
