// View radiance (include/sosrt.h): phase rows at view cosines off the grid, and the radiance of a resident
// field there by source-function integration.  A post-processing stage: it reads the columns of the last sosrt_set_columns* and
// writes its outputs and scratch of its own (handle.hpp, View), nothing else.  Host code.
#include <hip/hip_runtime.h>

#include <cmath>

#include "handle.hpp"

using namespace sosrt;

// columns a builder of the azimuth-resolved stage may be asked for: the current ones (before sosrt_set_columns, the handle's width)
static int view_batch_cap(const sosrt_handle* h) { return h->have_cols ? h->B : h->max_batch; }

static int view_phase_check(sosrt_handle* h, int kind, double g, int V2, const double* mu_signed, ViewMu* vm) {
    if (int e = phase_check(h, kind, g)) return e;
    if (V2 < 1 || V2 > 2 * SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "V2=%d exit cosines: must be 1..%d", V2, 2 * SOSRT_MAX_VIEWS);
    if (!mu_signed) return fail(SOSRT_E_INVALID, "null mu_signed");
    for (int j = 0; j < V2; ++j) {
        if (!(std::isfinite(mu_signed[j]) && std::fabs(mu_signed[j]) <= 1))
            return fail(SOSRT_E_INVALID, "mu_signed[%d] = %g is not a cosine in [-1, 1]", j, mu_signed[j]);
        vm->s[j] = mu_signed[j];
    }
    for (int j = V2; j < 2 * kMaxViews; ++j) vm->s[j] = 0;
    return 0;
}

extern "C" {

int sosrt_phase_rows_dev(sosrt_t* h, int kind, double g, int V2, const double* mu_signed, double* d_rows_out) {
    ViewMu vm;
    if (int e = view_phase_check(h, kind, g, V2, mu_signed, &vm)) return e;
    if (!d_rows_out) return fail(SOSRT_E_INVALID, "null output");
    HIPCHK(hipSetDevice(h->device));
    PhaseJob j = phase_job(h, kind, g);
    j.V2 = V2; j.out = d_rows_out;
    launch_phase_builder(h->stream, h->g, &vm, j);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0_rows_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, int V2, const double* mu_signed,
                            double* d_out) {
    ViewMu vm;
    if (int e = view_phase_check(h, kind, g, V2, mu_signed, &vm)) return e;
    if (B < 1 || !d_mu0 || !d_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    PhaseJob j = phase_job(h, kind, g);
    j.mu0 = d_mu0; j.B = B; j.V2 = V2; j.out = d_out;
    launch_phase_builder(h->stream, h->g, &vm, j);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"

// The body of sosrt_view_radiance_dev and of sosrt_view_radiance_profile_dev.  profile: the handle's
// per-level weights are required and multiply the stage's row coefficients behind launch_prepare, as apply_row_weights does for
// the solve's; the source kernel multiplies by the coefficients row by row, so nothing else changes.  Without it the weights
// are refused (the first order here is a closed form per zone) and no launch is added.
static int view_radiance_body(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_I_src,
                              const double* d_rows_atm, const double* d_rows_aer, const double* d_p0rows_atm,
                              const double* d_p0rows_aer, int quadrature, int nlev, const int* levels, double* d_scat_out,
                              double* d_first_out, bool profile) {
    if (profile) {
        if (int e = profile_check(h, B, "sosrt_view_radiance_profile_dev")) return e;
    } else {
        if (int e = need_gpu(h)) return e;
        if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
        if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
        if (int e = no_row_weights(h, "sosrt_view_radiance_dev")) return e;
    }
    // ---- what the stage refuses: every check comes before the first launch, so a refused call changes nothing ----
    if (B < 1 || B > h->B) return fail(SOSRT_E_INVALID, "B=%d: the handle's current columns are %d (sosrt_set_columns)", B, h->B);
    if (V < 1 || V > SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "V=%d view cosines: must be 1..%d", V, SOSRT_MAX_VIEWS);
    if (!mu_view) return fail(SOSRT_E_INVALID, "null mu_view");
    for (int v = 0; v < V; ++v)
        if (!(std::isfinite(mu_view[v]) && mu_view[v] >= 0.01 && mu_view[v] <= 1))
            return fail(SOSRT_E_INVALID, "mu_view[%d] = %g: a view cosine must be finite and in [0.01, 1]", v, mu_view[v]);
    if (quadrature != SOSRT_VIEW_QUAD_GRID && quadrature != SOSRT_VIEW_QUAD_LINEAR)
        return fail(SOSRT_E_INVALID, "unknown quadrature %d (SOSRT_VIEW_QUAD_GRID or SOSRT_VIEW_QUAD_LINEAR)", quadrature);
    if (nlev < 1 || !levels) return fail(SOSRT_E_INVALID, "no levels");
    for (int i = 0; i < nlev; ++i)
        if (levels[i] < 0 || levels[i] >= h->L) return fail(SOSRT_E_INVALID, "levels[%d] = %d is outside [0, %d)", i, levels[i], h->L);
    if (h->surface == SOSRT_SURFACE_LAMBERTIAN || h->surface == SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "view radiance is not available over a Lambertian surface: its boundary for the orders n >= 2 needs "
                                     "the sum over them of the grid's surface row, which the source field does not carry");
    if (h->cols.max_set_used > 0 || h->cols.p0_zones > 0)
        return fail(SOSRT_E_INVALID, "view radiance is not available with several aerosol phase sets (sosrt_set_phase_sets, sosrt_set_aerosol_sets)");
    if (h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "view radiance is not available with atmosphere phase sets (sosrt_set_atm_phase_sets, sosrt_set_atmosphere_sets)");
    if (!d_scat_out && !d_first_out) return fail(SOSRT_E_INVALID, "neither d_scat_out nor d_first_out: nothing to compute");
    if (!d_tau) return fail(SOSRT_E_INVALID, "null d_tau");
    const bool three = h->geom == SOSRT_GEOM_THREE_ZONE;
    if (d_first_out) {
        if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            return fail(SOSRT_E_INVALID, "the first order at view cosines is the coded one (SOSRT_FIRST_ORDER_CODED); the handle is set to SOSRT_FIRST_ORDER_README");
        if (!d_p0rows_atm || (three && !d_p0rows_aer)) return fail(SOSRT_E_INVALID, "d_first_out needs d_p0rows_atm and d_p0rows_aer");
    }
    if (d_scat_out && (!d_I_src || !d_rows_atm || (three && !d_rows_aer)))
        return fail(SOSRT_E_INVALID, "d_scat_out needs d_I_src, d_rows_atm and d_rows_aer");

    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    hipStream_t s = h->stream;
    const int L = h->L, D = h->D, V2 = 2 * V;
    auto& vw = h->view;
    for (auto& e : vw.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (int e = vw.d_desc.reserve(h->max_batch)) return e;
    if (int e = vw.d_rc.reserve((size_t)2 * h->max_batch * L)) return e;
    if (d_scat_out) {
        if (int e = vw.d_fold.reserve((size_t)view_source_kpad(D) * view_source_cols(V))) return e;
        if (int e = vw.d_S.reserve((size_t)B * L * V2)) return e;
    }
    ViewMu vm;
    for (int j = 0; j < 2 * kMaxViews; ++j) vm.s[j] = 0;
    for (int v = 0; v < V; ++v) { vm.s[v] = -mu_view[v]; vm.s[V + v] = mu_view[v]; }
    // the zone tables and the row coefficients (ca, cr) of the current columns on the caller's optical depths: the kernel the
    // solve prepares its own with, writing into this stage's buffers
    double* rca = vw.d_rc.p;
    double* rcr = rca + (size_t)h->max_batch * L;
    launch_prepare(s, h->g, B, h->geom, h->surface, scalars_of(h), d_tau, vw.d_desc.p, rca, rcr);
    HIPCHK(hipGetLastError());
    if (profile) {
        launch_row_weights_apply(s, (size_t)B * L, h->cols.d_rwa.p, h->cols.d_rwr.p, rca, rcr);
        HIPCHK(hipGetLastError());
    }
    vw.timed_scat = vw.timed_first = false;
    if (d_scat_out) {
        HIPCHK(hipEventRecord(vw.ev[0], s));
        launch_view_source(s, B * L, D, V, h->grid.d_w, d_rows_atm, three ? d_rows_aer : nullptr, d_I_src, rca, rcr, vw.d_fold.p,
                           vw.d_S.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(vw.ev[1], s));
    }
    for (int l0 = 0; l0 < nlev && d_scat_out; l0 += kViewLevels) {
        ViewLevels lv;
        lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
        for (int i = 0; i < kViewLevels; ++i) lv.t[i] = i < lv.n ? levels[l0 + i] : -1;
        launch_view_transport(s, B, V, L, quadrature, nlev, d_tau, vw.d_S.p, vw.d_desc.p, vm, lv, d_scat_out + (size_t)l0 * V2);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(vw.ev[2], s));
    vw.timed_scat = d_scat_out != nullptr;
    for (int l0 = 0; l0 < nlev && d_first_out; l0 += kViewLevels) {
        ViewLevels lv;
        lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
        for (int i = 0; i < kViewLevels; ++i) lv.t[i] = i < lv.n ? levels[l0 + i] : -1;
        launch_view_first_order(s, B, V, L, nlev, d_tau, d_p0rows_atm, three ? d_p0rows_aer : nullptr, vw.d_desc.p, vm, lv,
                                d_first_out + (size_t)l0 * V2);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(vw.ev[3], s));
    vw.timed_first = d_first_out != nullptr;
    return 0;
}

extern "C" {

int sosrt_view_radiance_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_I_src,
                            const double* d_rows_atm, const double* d_rows_aer, const double* d_p0rows_atm,
                            const double* d_p0rows_aer, int quadrature, int nlev, const int* levels, double* d_scat_out,
                            double* d_first_out) {
    return view_radiance_body(h, B, V, mu_view, d_tau, d_I_src, d_rows_atm, d_rows_aer, d_p0rows_atm, d_p0rows_aer, quadrature, nlev,
                              levels, d_scat_out, d_first_out, false);
}

int sosrt_view_radiance_profile_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_I_src,
                                    const double* d_rows_atm, const double* d_rows_aer, int quadrature, int nlev, const int* levels,
                                    double* d_scat_out) {
    // the scattered term only: the first term under weights is sosrt_view_first_order_profile_dev / sosrt_emission_view_profile_dev
    if (h && !d_scat_out) return fail(SOSRT_E_INVALID, "sosrt_view_radiance_profile_dev: null d_scat_out");
    return view_radiance_body(h, B, V, mu_view, d_tau, d_I_src, d_rows_atm, d_rows_aer, nullptr, nullptr, quadrature, nlev, levels,
                              d_scat_out, nullptr, true);
}

// ---------------------------------------------------------------------------------------------
// azimuth-resolved view radiance: mode rows and first-order phase values at the view lanes, the synthesis
// ---------------------------------------------------------------------------------------------
int sosrt_phase_rows_modes_dev(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, int V2,
                               const double* mu_signed, double* d_rows_out) {
    ViewMu vm;
    if (int e = view_phase_check(h, kind, g, V2, mu_signed, &vm)) return e;
    if (m_first < 1) return fail(SOSRT_E_INVALID, "mode rows: m_first = %d; mode 0 is sosrt_phase_rows_dev", m_first);
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (!d_rows_out) return fail(SOSRT_E_INVALID, "null output");
    HIPCHK(hipSetDevice(h->device));
    if (int e = modes_table(h, nphi, m_first, m_count)) return e;
    PhaseJob j = phase_job(h, kind, g, m_first, m_count, nphi);
    j.sign_odd = sign_odd; j.V2 = V2; j.out = d_rows_out;
    launch_phase_builder(h->stream, h->g, &vm, j);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0_rows_modes_dev(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* d_mu0,
                                  int V2, const double* mu_signed, double* d_out) {
    ViewMu vm;
    if (int e = view_phase_check(h, kind, g, V2, mu_signed, &vm)) return e;
    if (m_first < 1) return fail(SOSRT_E_INVALID, "mode rows: m_first = %d; mode 0 is sosrt_phase_p0_rows_dev", m_first);
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (B < 1 || !d_mu0 || !d_out) return fail(SOSRT_E_INVALID, "bad argument");
    if (B > view_batch_cap(h)) return fail(SOSRT_E_INVALID, "B=%d: the handle's current columns are %d", B, view_batch_cap(h));
    HIPCHK(hipSetDevice(h->device));
    if (int e = modes_table(h, nphi, m_first, m_count)) return e;
    PhaseJob j = phase_job(h, kind, g, m_first, m_count, nphi);
    j.mu0 = d_mu0; j.B = B; j.V2 = V2; j.out = d_out;
    launch_phase_builder(h->stream, h->g, &vm, j);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0_rows_azimuth_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, int V2, const double* mu_signed,
                                    int nphi_out, const double* d_phi, double* d_out) {
    ViewMu vm;
    if (int e = view_phase_check(h, kind, g, V2, mu_signed, &vm)) return e;
    if (B < 1 || !d_mu0 || !d_phi || !d_out) return fail(SOSRT_E_INVALID, "bad argument");
    if (nphi_out < 1) return fail(SOSRT_E_INVALID, "nphi_out = %d: at least one azimuth", nphi_out);
    if (B > view_batch_cap(h)) return fail(SOSRT_E_INVALID, "B=%d: the handle's current columns are %d", B, view_batch_cap(h));
    if ((long long)nphi_out * V2 > 0x7fffffffLL) return fail(SOSRT_E_INVALID, "nphi_out * V2 too large");
    HIPCHK(hipSetDevice(h->device));
    PhaseJob j = phase_job(h, kind, g);
    j.mu0 = d_mu0; j.B = B; j.V2 = V2; j.nphi_out = nphi_out; j.phi = d_phi; j.out = d_out;
    launch_phase_builder(h->stream, h->g, &vm, j);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_view_azimuth_accumulate_dev(sosrt_t* h, int B, int m, int nlev, int V2, const double* d_val, int nphi_out,
                                      const double* d_phi, double* d_out) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || nlev < 1 || !d_val || !d_phi || !d_out) return fail(SOSRT_E_INVALID, "view azimuth accumulate: bad argument (B=%d nlev=%d)", B, nlev);
    if (B > view_batch_cap(h)) return fail(SOSRT_E_INVALID, "B=%d: the handle's current columns are %d", B, view_batch_cap(h));
    if (m < 0 || m > SOSRT_MAX_MODES) return fail(SOSRT_E_INVALID, "view azimuth accumulate: mode %d is outside 0..SOSRT_MAX_MODES = %d", m, SOSRT_MAX_MODES);
    if (V2 < 1 || V2 > 2 * SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "V2=%d lanes: must be 1..%d", V2, 2 * SOSRT_MAX_VIEWS);
    if (nphi_out < 1) return fail(SOSRT_E_INVALID, "nphi_out = %d: at least one azimuth", nphi_out);
    const size_t n = (size_t)B * nlev * V2;
    if (n * (size_t)nphi_out > (size_t)0x7fffffff * 256) return fail(SOSRT_E_INVALID, "view azimuth accumulate: output too large");
    HIPCHK(hipSetDevice(h->device));
    launch_view_azimuth_accumulate(h->stream, n, m, d_val, nphi_out, d_phi, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_view_timing(sosrt_t* h, double* ms) {
    if (int e = need_gpu(h)) return e;
    if (!ms) return fail(SOSRT_E_INVALID, "null argument");
    auto& vw = h->view;
    ms[0] = ms[1] = ms[2] = 0;
    if (!vw.ev[3]) return fail(SOSRT_E_STATE, "sosrt_view_radiance_dev has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(vw.ev[3]));
    float t = 0;
    if (vw.timed_scat) {
        HIPCHK(hipEventElapsedTime(&t, vw.ev[0], vw.ev[1])); ms[0] = t;
        HIPCHK(hipEventElapsedTime(&t, vw.ev[1], vw.ev[2])); ms[1] = t;
    }
    if (vw.timed_first) { HIPCHK(hipEventElapsedTime(&t, vw.ev[2], vw.ev[3])); ms[2] = t; }
    return 0;
}

}  // extern "C"
