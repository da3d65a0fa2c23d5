// Thermal emission (include/sosrt.h): the emitted field on the grid's directions and at view cosines, and
// the epilogue without beam terms.  A stage beside the solve: it reads the columns of the last sosrt_set_columns* and writes its
// outputs, nothing else -- the handle's columns, resident field, order targets, phase state and first-order mode stay as they
// were.  Host code.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emission.hpp"
#include "handle.hpp"

using namespace sosrt;

// what the three entry points refuse alike; every check comes before the first launch, so a refused call writes nothing
static int emission_check(sosrt_handle* h, int B, const char* what) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "%s: the emission stage is for three-zone and zone-table columns; the single slab "
                                     "(SOSRT_GEOM_SINGLE_SLAB) has no zone table to take emission coefficients from", what);
    if (B < 1 || B > h->B) return fail(SOSRT_E_INVALID, "%s: B=%d, the handle's current columns are %d (sosrt_set_columns)", what, B, h->B);
    if (h->L > kEmissionMaxL) return fail(SOSRT_E_INVALID, "%s: L=%d, the emission stage takes at most %d layers", what, h->L, kEmissionMaxL);
    return 0;
}

extern "C" {

int sosrt_emission_dev(sosrt_t* h, int B, const double* d_tau, const double* d_planck, const double* d_planck_surface,
                       const double* d_emissivity, double* d_I0_out) {
    if (int e = emission_check(h, B, "sosrt_emission_dev")) return e;
    if (int e = no_row_weights(h, "sosrt_emission_dev")) return e;
    if (!d_tau || !d_planck || !d_planck_surface || !d_I0_out) return fail(SOSRT_E_INVALID, "sosrt_emission_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_emission(h->stream, h->g, B, scalars_of(h), h->surface, d_tau, d_planck, d_planck_surface, d_emissivity, d_I0_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_emission_view_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_planck,
                            const double* d_planck_surface, const double* d_emissivity, int nlev, const int* levels,
                            double* d_out) {
    if (int e = emission_check(h, B, "sosrt_emission_view_dev")) return e;
    if (int e = no_row_weights(h, "sosrt_emission_view_dev")) return e;
    if (V < 1 || V > SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: V=%d view cosines: must be 1..%d", V, SOSRT_MAX_VIEWS);
    if (!mu_view) return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: null mu_view");
    for (int v = 0; v < V; ++v)
        if (!(std::isfinite(mu_view[v]) && mu_view[v] >= 0.01 && mu_view[v] <= 1))
            return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: mu_view[%d] = %g: a view cosine must be finite and in [0.01, 1]", v, mu_view[v]);
    if (nlev < 1 || !levels) return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: no levels");
    for (int i = 0; i < nlev; ++i)
        if (levels[i] < 0 || levels[i] >= h->L)
            return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: levels[%d] = %d is outside [0, %d)", i, levels[i], h->L);
    if (h->surface == SOSRT_SURFACE_LAMBERTIAN || h->surface == SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: emission at view cosines is not available over a Lambertian surface: its "
                                     "ground value needs the grid's downward surface row, which a view lane does not carry");
    if (!d_tau || !d_planck || !d_planck_surface || !d_out) return fail(SOSRT_E_INVALID, "sosrt_emission_view_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    ViewMu vm;
    for (int j = 0; j < 2 * kMaxViews; ++j) vm.s[j] = 0;
    for (int v = 0; v < V; ++v) { vm.s[v] = -mu_view[v]; vm.s[V + v] = mu_view[v]; }
    for (int l0 = 0; l0 < nlev; l0 += kViewLevels) {
        ViewLevels lv;
        lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
        for (int i = 0; i < kViewLevels; ++i) lv.t[i] = i < lv.n ? levels[l0 + i] : -1;
        launch_emission_view(h->stream, B, V, h->L, nlev, scalars_of(h), h->surface, d_tau, d_planck, d_planck_surface,
                             d_emissivity, vm, lv, d_out + (size_t)l0 * 2 * V);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int sosrt_epilogue_emission_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, const double* d_z_profile,
                                double* d_flux_down, double* d_flux_up, double* d_diffusivity, double* d_heating_rate,
                                double* d_net_toa) {
    if (int e = emission_check(h, B, "sosrt_epilogue_emission_dev")) return e;
    if (!d_tau || !d_I) return fail(SOSRT_E_INVALID, "sosrt_epilogue_emission_dev: null argument");
    if (d_heating_rate && !d_z_profile) return fail(SOSRT_E_INVALID, "sosrt_epilogue_emission_dev: the heating rate needs z_profile");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    EpilogueOut out{d_flux_down, d_flux_up, d_diffusivity, d_heating_rate, d_net_toa};
    launch_epilogue_emission(h->stream, h->g, h->grid.d_w, B, scalars_of(h), d_tau, d_I, d_z_profile, out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
