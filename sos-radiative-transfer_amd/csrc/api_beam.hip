// Pseudo-spherical direct beam (include/sosrt.h): the slant path of the beam, the first order on a beam
// path -- on the grid and at view lanes off it -- and the epilogue with its beam terms.  A stage beside the
// solve: it reads the columns of the last sosrt_set_columns* and writes its outputs, nothing else -- the handle's columns,
// resident field, order targets and phase state stay as they were.  Host code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "beam.hpp"
#include "beam_view.hpp"
#include "handle.hpp"

using namespace sosrt;

// what the entry points refuse alike; every check comes before the first launch, so a refused call writes nothing
static int beam_check(sosrt_handle* h, int B, const char* what) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "%s: the beam stage is for three-zone and zone-table columns; the single slab (SOSRT_GEOM_SINGLE_SLAB) "
                                     "has the plane closed form of I1_NumInt only", what);
    if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
        return fail(SOSRT_E_INVALID, "%s: the first order on a beam path is the coded one (SOSRT_FIRST_ORDER_CODED); the handle is set to "
                                     "SOSRT_FIRST_ORDER_README, whose isotropically reflected beam has no slant form", what);
    if (B < 1 || B > h->B) return fail(SOSRT_E_INVALID, "%s: B=%d, the handle's current columns are %d (sosrt_set_columns)", what, B, h->B);
    if (h->L > kBeamMaxL) return fail(SOSRT_E_INVALID, "%s: L=%d, the beam stage takes at most %d layers", what, h->L, kBeamMaxL);
    return 0;
}

// z [L] on the device: finite and strictly descending (read back: L doubles, after the stream's earlier work)
static int beam_check_z(sosrt_handle* h, const double* d_z, const char* what) {
    std::vector<double> z(h->L);
    HIPCHK(hipMemcpyAsync(z.data(), d_z, h->L * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int t = 0; t < h->L; ++t) {
        if (!std::isfinite(z[t])) return fail(SOSRT_E_INVALID, "%s: z[%d] = %g is not finite", what, t, z[t]);
        if (t && !(z[t] < z[t - 1]))
            return fail(SOSRT_E_INVALID, "%s: z must be strictly descending (z[%d] = %g, z[%d] = %g)", what, t - 1, z[t - 1], t, z[t]);
    }
    return 0;
}

extern "C" {

int sosrt_beam_slant_dev(sosrt_t* h, int B, const double* d_tau, const double* d_z, double earth_radius_km, const double* d_mu0,
                         double* d_sigma_out) {
    if (int e = beam_check(h, B, "sosrt_beam_slant_dev")) return e;
    if (!d_tau || !d_z || !d_sigma_out) return fail(SOSRT_E_INVALID, "sosrt_beam_slant_dev: null argument");
    if (!(std::isfinite(earth_radius_km) && earth_radius_km > 0))
        return fail(SOSRT_E_INVALID, "sosrt_beam_slant_dev: earth_radius_km = %g must be finite and > 0", earth_radius_km);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    if (int e = beam_check_z(h, d_z, "sosrt_beam_slant_dev")) return e;
    if (d_mu0) {
        // a caller's own cosines: each finite and in (0, 1] (the columns' own were checked when they were set)
        std::vector<double> m(B);
        HIPCHK(hipMemcpyAsync(m.data(), d_mu0, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int b = 0; b < B; ++b)
            if (!(std::isfinite(m[b]) && m[b] > 0 && m[b] <= 1))
                return fail(SOSRT_E_INVALID, "sosrt_beam_slant_dev: mu0[%d] = %g must be in (0, 1]", b, m[b]);
    }
    launch_beam_slant(h->stream, h->L, B, d_tau, d_z, earth_radius_km, d_mu0 ? d_mu0 : scalars_of(h).mu0, d_sigma_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_first_order_beam_dev(sosrt_t* h, int B, const double* d_tau, const double* d_sigma, const double* d_P0_atm,
                               const double* d_P0_aer, double* d_I1_out) {
    if (int e = beam_check(h, B, "sosrt_first_order_beam_dev")) return e;
    if (int e = no_row_weights(h, "sosrt_first_order_beam_dev")) return e;
    if (!d_tau || !d_sigma || !d_P0_atm || !d_P0_aer || !d_I1_out)
        return fail(SOSRT_E_INVALID, "sosrt_first_order_beam_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_first_order_beam(h->stream, h->g, B, scalars_of(h), d_tau, d_sigma, d_P0_atm, d_P0_aer, h->cols.p0_zones, d_I1_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_epilogue_beam_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, int beam_norm, const double* d_z_profile,
                            double* d_flux_down, double* d_flux_up, double* d_diffusivity, double* d_heating_rate,
                            double* d_net_toa, const double* d_sigma) {
    if (int e = beam_check(h, B, "sosrt_epilogue_beam_dev")) return e;
    if (!d_tau || !d_I || !d_sigma) return fail(SOSRT_E_INVALID, "sosrt_epilogue_beam_dev: null argument");
    if (d_heating_rate && !d_z_profile) return fail(SOSRT_E_INVALID, "sosrt_epilogue_beam_dev: the heating rate needs z_profile");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    EpilogueOut out{d_flux_down, d_flux_up, d_diffusivity, d_heating_rate, d_net_toa};
    launch_epilogue_beam(h->stream, h->g, h->grid.d_w, B, scalars_of(h), d_tau, d_sigma, d_I, beam_norm, d_z_profile, out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_view_first_order_beam_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_sigma,
                                    int nset, const double* d_p0rows_atm, const double* d_p0rows_aer, int nlev, const int* levels,
                                    double* d_first_out) {
    const char* what = "sosrt_view_first_order_beam_dev";
    if (int e = beam_check(h, B, what)) return e;
    if (int e = no_row_weights(h, what)) return e;
    // ---- the limits of sosrt_view_radiance_dev; every check comes before the first launch, so a refused call writes nothing ----
    if (V < 1 || V > SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "%s: V=%d view cosines: must be 1..%d", what, V, SOSRT_MAX_VIEWS);
    if (!mu_view) return fail(SOSRT_E_INVALID, "%s: null mu_view", what);
    for (int v = 0; v < V; ++v)
        if (!(std::isfinite(mu_view[v]) && mu_view[v] >= 0.01 && mu_view[v] <= 1))
            return fail(SOSRT_E_INVALID, "%s: mu_view[%d] = %g: a view cosine must be finite and in [0.01, 1]", what, v, mu_view[v]);
    if (nset < 1) return fail(SOSRT_E_INVALID, "%s: nset=%d: at least one set of p0 rows", what, nset);
    if (nlev < 1 || !levels) return fail(SOSRT_E_INVALID, "%s: no levels", what);
    for (int i = 0; i < nlev; ++i)
        if (levels[i] < 0 || levels[i] >= h->L)
            return fail(SOSRT_E_INVALID, "%s: levels[%d] = %d is outside [0, %d)", what, i, levels[i], h->L);
    if (h->surface == SOSRT_SURFACE_LAMBERTIAN || h->surface == SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "%s: the first order at view cosines is not available over a Lambertian surface (the handle's "
                                     "surface), as the view stage is not", what);
    if (h->cols.max_set_used > 0 || h->cols.p0_zones > 0)
        return fail(SOSRT_E_INVALID, "%s: not available with several aerosol phase sets (sosrt_set_phase_sets, sosrt_set_aerosol_sets): "
                                     "d_p0rows_aer is one row per column", what);
    if (h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "%s: not available with atmosphere phase sets (sosrt_set_atm_phase_sets, sosrt_set_atmosphere_sets): "
                                     "d_p0rows_atm is one row per column", what);
    if (!d_tau) return fail(SOSRT_E_INVALID, "%s: null d_tau", what);
    if (!d_sigma) return fail(SOSRT_E_INVALID, "%s: null d_sigma", what);
    if (!d_p0rows_atm || !d_p0rows_aer) return fail(SOSRT_E_INVALID, "%s: null d_p0rows_atm or d_p0rows_aer", what);
    if (!d_first_out) return fail(SOSRT_E_INVALID, "%s: null d_first_out", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    ViewMu vm;
    for (int j = 0; j < 2 * kMaxViews; ++j) vm.s[j] = 0;
    for (int v = 0; v < V; ++v) { vm.s[v] = -mu_view[v]; vm.s[V + v] = mu_view[v]; }
    // levels in chunks of kViewLevels, as the view stage takes them; within a chunk sorted by row for the sweeps' cursor
    for (int l0 = 0; l0 < nlev; l0 += kViewLevels) {
        BeamViewLevels lv;
        lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
        int order[kViewLevels];
        for (int i = 0; i < lv.n; ++i) order[i] = i;
        std::stable_sort(order, order + lv.n, [&](int x, int y) { return levels[l0 + x] < levels[l0 + y]; });
        for (int i = 0; i < kViewLevels; ++i) {
            lv.t[i] = i < lv.n ? levels[l0 + order[i]] : -1;
            lv.idx[i] = i < lv.n ? order[i] : 0;
        }
        launch_view_first_order_beam(h->stream, h->L, B, V, nset, nlev, scalars_of(h), d_tau, d_sigma, d_p0rows_atm, d_p0rows_aer,
                                     vm, lv, d_first_out + (size_t)l0 * 2 * V);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
