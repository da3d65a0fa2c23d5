// Per-level weights at view lanes (include/sosrt.h): the first term of the view radiance of a column whose
// rows carry the weights of sosrt_set_row_weights_dev -- the solar first order on a beam path and the thermal emission, at view
// cosines off the grid.  (The scattered term, sosrt_view_radiance_profile_dev, shares its body with sosrt_view_radiance_dev:
// api_view.hip.)  Stages beside the solve: they read the columns of the last sosrt_set_columns*, the handle's weights, and write
// their outputs, nothing else.  Host code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "handle.hpp"
#include "profile_view.hpp"

using namespace sosrt;

// the limits of the view stage (sosrt_view_radiance_dev), as sosrt_view_first_order_beam_dev and sosrt_emission_view_dev apply
// them; every check comes before the first launch, so a refused call writes nothing
// (phase_rows: the entry takes one p0 row per column, so it refuses phase sets as its model does)
static int view_limits_check(sosrt_handle* h, int V, const double* mu_view, int nlev, const int* levels, bool phase_rows,
                             const char* what) {
    if (V < 1 || V > SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "%s: V=%d view cosines: must be 1..%d", what, V, SOSRT_MAX_VIEWS);
    if (!mu_view) return fail(SOSRT_E_INVALID, "%s: null mu_view", what);
    for (int v = 0; v < V; ++v)
        if (!(std::isfinite(mu_view[v]) && mu_view[v] >= 0.01 && mu_view[v] <= 1))
            return fail(SOSRT_E_INVALID, "%s: mu_view[%d] = %g: a view cosine must be finite and in [0.01, 1]", what, v, mu_view[v]);
    if (nlev < 1 || !levels) return fail(SOSRT_E_INVALID, "%s: no levels", what);
    for (int i = 0; i < nlev; ++i)
        if (levels[i] < 0 || levels[i] >= h->L)
            return fail(SOSRT_E_INVALID, "%s: levels[%d] = %d is outside [0, %d)", what, i, levels[i], h->L);
    if (h->surface == SOSRT_SURFACE_LAMBERTIAN || h->surface == SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "%s: not available over a Lambertian surface (the handle's surface), as the view stage is not", what);
    if (phase_rows && (h->cols.max_set_used > 0 || h->cols.p0_zones > 0))
        return fail(SOSRT_E_INVALID, "%s: not available with several aerosol phase sets (sosrt_set_phase_sets, sosrt_set_aerosol_sets), "
                                     "as the view stage is not", what);
    if (phase_rows && h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "%s: not available with atmosphere phase sets (sosrt_set_atm_phase_sets, sosrt_set_atmosphere_sets), "
                                     "as the view stage is not", what);
    return 0;
}

// the levels [l0, l0 + kViewLevels) of a call sorted by row for the sweeps' cursor, idx their places in the caller's list
static BeamViewLevels sorted_levels(int nlev, const int* levels, int l0) {
    BeamViewLevels lv;
    lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
    int order[kViewLevels];
    for (int i = 0; i < lv.n; ++i) order[i] = i;
    std::stable_sort(order, order + lv.n, [&](int x, int y) { return levels[l0 + x] < levels[l0 + y]; });
    for (int i = 0; i < kViewLevels; ++i) {
        lv.t[i] = i < lv.n ? levels[l0 + order[i]] : -1;
        lv.idx[i] = i < lv.n ? order[i] : 0;
    }
    return lv;
}

static ViewMu signed_lanes(int V, const double* mu_view) {
    ViewMu vm;
    for (int j = 0; j < 2 * kMaxViews; ++j) vm.s[j] = 0;
    for (int v = 0; v < V; ++v) { vm.s[v] = -mu_view[v]; vm.s[V + v] = mu_view[v]; }
    return vm;
}

extern "C" {

int sosrt_view_first_order_profile_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_sigma,
                                       int nset, const double* d_p0rows_atm, const double* d_p0rows_aer, int nlev, const int* levels,
                                       double* d_first_out) {
    const char* what = "sosrt_view_first_order_profile_dev";
    if (int e = profile_check(h, B, what)) return e;
    if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
        return fail(SOSRT_E_INVALID, "%s: the first order on a beam path is the coded one (SOSRT_FIRST_ORDER_CODED); the handle is set to "
                                     "SOSRT_FIRST_ORDER_README", what);
    if (int e = view_limits_check(h, V, mu_view, nlev, levels, true, what)) return e;
    if (nset < 1) return fail(SOSRT_E_INVALID, "%s: nset=%d: at least one set of p0 rows", what, nset);
    if (!d_tau) return fail(SOSRT_E_INVALID, "%s: null d_tau", what);
    if (!d_sigma) return fail(SOSRT_E_INVALID, "%s: null d_sigma", what);
    if (!d_p0rows_atm || !d_p0rows_aer) return fail(SOSRT_E_INVALID, "%s: null d_p0rows_atm or d_p0rows_aer", what);
    if (!d_first_out) return fail(SOSRT_E_INVALID, "%s: null d_first_out", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    const ViewMu vm = signed_lanes(V, mu_view);
    for (int l0 = 0; l0 < nlev; l0 += kViewLevels) {
        launch_view_first_order_profile(h->stream, h->L, B, V, nset, nlev, scalars_of(h), d_tau, d_sigma, d_p0rows_atm, d_p0rows_aer,
                                        h->cols.d_rwa.p, h->cols.d_rwr.p, vm, sorted_levels(nlev, levels, l0),
                                        d_first_out + (size_t)l0 * 2 * V);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int sosrt_emission_view_profile_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_planck,
                                    const double* d_planck_surface, const double* d_emissivity, int nlev, const int* levels,
                                    double* d_out) {
    const char* what = "sosrt_emission_view_profile_dev";
    if (int e = profile_check(h, B, what)) return e;
    if (int e = view_limits_check(h, V, mu_view, nlev, levels, false, what)) return e;
    if (!d_tau || !d_planck || !d_planck_surface || !d_out) return fail(SOSRT_E_INVALID, "%s: null argument", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    const ViewMu vm = signed_lanes(V, mu_view);
    for (int l0 = 0; l0 < nlev; l0 += kViewLevels) {
        launch_emission_view_profile(h->stream, B, V, h->L, nlev, scalars_of(h), h->surface, d_tau, d_planck, d_planck_surface,
                                     d_emissivity, h->cols.d_rwa.p, h->cols.d_rwr.p, vm, sorted_levels(nlev, levels, l0),
                                     d_out + (size_t)l0 * 2 * V);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
