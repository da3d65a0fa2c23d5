// Per-level weights on the source function (include/sosrt.h): the first order and the thermal emission of a
// column whose rows carry the weights of sosrt_set_row_weights_dev (api_columns.hip).  Stages beside the solve: they read the
// columns of the last sosrt_set_columns*, the handle's weights, and write their outputs, nothing else.  Host code.
#include <hip/hip_runtime.h>

#include "handle.hpp"
#include "profile.hpp"

using namespace sosrt;

// what the entry points of the stage refuse alike, here and at view lanes (api_view.hip, api_profile_view.hip); every check comes
// before the launch, so a refused call writes nothing
int sosrt::profile_check(sosrt_handle* h, int B, const char* what) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "%s: the stage is for three-zone and zone-table columns, not the single slab (SOSRT_GEOM_SINGLE_SLAB)", what);
    if (B < 1 || B > h->B) return fail(SOSRT_E_INVALID, "%s: B=%d, the handle's current columns are %d (sosrt_set_columns)", what, B, h->B);
    if (h->L > kProfileMaxL) return fail(SOSRT_E_INVALID, "%s: L=%d, the stage takes at most %d layers", what, h->L, kProfileMaxL);
    if (!h->cols.rw_on) return fail(SOSRT_E_STATE, "%s: no per-level weights are set (sosrt_set_row_weights_dev)", what);
    return 0;
}

extern "C" {

int sosrt_first_order_profile_dev(sosrt_t* h, int B, const double* d_tau, const double* d_sigma, const double* d_P0_atm,
                                  const double* d_P0_aer, double* d_I1_out) {
    if (int e = profile_check(h, B, "sosrt_first_order_profile_dev")) return e;
    if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
        return fail(SOSRT_E_INVALID, "sosrt_first_order_profile_dev: the first order on a beam path is the coded one (SOSRT_FIRST_ORDER_CODED); "
                                     "the handle is set to SOSRT_FIRST_ORDER_README");
    if (!d_tau || !d_sigma || !d_P0_atm || !d_P0_aer || !d_I1_out)
        return fail(SOSRT_E_INVALID, "sosrt_first_order_profile_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_first_order_profile(h->stream, h->g, B, scalars_of(h), d_tau, d_sigma, d_P0_atm, d_P0_aer, h->cols.p0_zones,
                               h->cols.d_rwa.p, h->cols.d_rwr.p, d_I1_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_emission_profile_dev(sosrt_t* h, int B, const double* d_tau, const double* d_planck, const double* d_planck_surface,
                               const double* d_emissivity, double* d_I0_out) {
    if (int e = profile_check(h, B, "sosrt_emission_profile_dev")) return e;
    if (!d_tau || !d_planck || !d_planck_surface || !d_I0_out) return fail(SOSRT_E_INVALID, "sosrt_emission_profile_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_emission_profile(h->stream, h->g, B, scalars_of(h), h->surface, d_tau, d_planck, d_planck_surface, d_emissivity,
                            h->cols.d_rwa.p, h->cols.d_rwr.p, d_I0_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
