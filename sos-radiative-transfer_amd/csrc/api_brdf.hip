// BRDF ground (include/sosrt.h): the operator of a named BRDF, its beam row, the ground source of a field's
// surface row, the ground source's unscattered field and the sum over ground reflections; the Fourier modes of the first two
// (section 21); and their counterparts at view cosines off the grid with the ground's unscattered radiance at the view lanes
// (section 22).  Stages beside the solve: they read
// the grid and the columns of the last sosrt_set_columns* and write their outputs, nothing else -- the handle's columns,
// resident field, order targets, phase state and first-order mode stay as they were.  Host code.
#include <hip/hip_runtime.h>

#include <cmath>

#include "brdf.hpp"
#include "handle.hpp"

using namespace sosrt;

// what the entry points refuse alike; every check comes before the first launch, so a refused call writes nothing
// (per_column: the call takes a column count; the operator does not)
static int brdf_check(sosrt_handle* h, int B, bool per_column, const char* what) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "%s: the BRDF ground is for three-zone and zone-table columns; the single slab "
                                     "(SOSRT_GEOM_SINGLE_SLAB) has no ground", what);
    if (h->N < 4) return fail(SOSRT_E_INVALID, "%s: N=%d, the BRDF ground needs N >= 4", what, h->N);
    if (per_column && (B < 1 || B > h->B))
        return fail(SOSRT_E_INVALID, "%s: B=%d, the handle's current columns are %d (sosrt_set_columns)", what, B, h->B);
    return 0;
}

static int brdf_params(int kind, const double* params, int nparams, int nphi, BrdfParams& bp, const char* what) {
    if (nphi < 3 || nphi > SOSRT_BRDF_MAX_NPHI)
        return fail(SOSRT_E_INVALID, "%s: nphi=%d azimuth nodes: must be 3..%d", what, nphi, SOSRT_BRDF_MAX_NPHI);
    bp.kind = kind;
    bp.p[0] = bp.p[1] = bp.p[2] = 0;
    if (kind == SOSRT_BRDF_LAMBERTIAN) {
        if (nparams != 0) return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_LAMBERTIAN takes no parameters (nparams=%d)", what, nparams);
        return 0;
    }
    if (kind == SOSRT_BRDF_RPV) {
        if (nparams != 3) return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_RPV takes 3 parameters rho0, k, Theta (nparams=%d)", what, nparams);
        if (!params) return fail(SOSRT_E_INVALID, "%s: null params", what);
        if (!(params[0] > 0 && std::isfinite(params[0])) || !(params[1] > 0 && std::isfinite(params[1])) || !(std::fabs(params[2]) < 1))
            return fail(SOSRT_E_INVALID, "%s: RPV parameters rho0=%g, k=%g, Theta=%g: need rho0 > 0, k > 0, |Theta| < 1", what,
                        params[0], params[1], params[2]);
        for (int i = 0; i < 3; ++i) bp.p[i] = params[i];
        return 0;
    }
    if (kind == SOSRT_BRDF_ROSS_THICK || kind == SOSRT_BRDF_LI_SPARSE_R) {
        const char* name = kind == SOSRT_BRDF_ROSS_THICK ? "SOSRT_BRDF_ROSS_THICK" : "SOSRT_BRDF_LI_SPARSE_R";
        if (nparams != 1) return fail(SOSRT_E_INVALID, "%s: %s takes 1 parameter mu_floor (nparams=%d)", what, name, nparams);
        if (!params) return fail(SOSRT_E_INVALID, "%s: null params", what);
        if (!(std::isfinite(params[0]) && params[0] >= 0 && params[0] < 1))
            return fail(SOSRT_E_INVALID, "%s: %s mu_floor=%g: need 0 <= mu_floor < 1", what, name, params[0]);
        bp.p[0] = params[0];
        return 0;
    }
    if (kind == SOSRT_BRDF_COX_MUNK) {
        if (nparams != 3)
            return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_COX_MUNK takes 3 parameters sigma2, refractive_index, shadow (nparams=%d)", what,
                        nparams);
        if (!params) return fail(SOSRT_E_INVALID, "%s: null params", what);
        if (!(std::isfinite(params[0]) && params[0] > 0))
            return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_COX_MUNK sigma2=%g: need a finite slope variance > 0", what, params[0]);
        if (!(std::isfinite(params[1]) && params[1] > 1))
            return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_COX_MUNK refractive_index=%g: need a finite real index > 1", what, params[1]);
        if (!(params[2] == 0 || params[2] == 1))
            return fail(SOSRT_E_INVALID, "%s: SOSRT_BRDF_COX_MUNK shadow=%g: need exactly 0 or 1", what, params[2]);
        for (int i = 0; i < 3; ++i) bp.p[i] = params[i];
        return 0;
    }
    return fail(SOSRT_E_INVALID, "%s: unknown BRDF kind %d", what, kind);
}

// the number of operator terms of the two terms entry points (sosrt.h)
static int brdf_terms(int K, const char* what) {
    if (K < 1 || K > SOSRT_BRDF_MAX_TERMS)
        return fail(SOSRT_E_INVALID, "%s: K=%d operator terms: must be 1..%d (SOSRT_BRDF_MAX_TERMS)", what, K, SOSRT_BRDF_MAX_TERMS);
    return 0;
}

// the range of Fourier modes the mode builders take (sosrt.h)
static int brdf_mode_range(int m_first, int m_count, int nphi, const char* what) {
    const int m_max = SOSRT_MAX_MODES < nphi - 2 ? SOSRT_MAX_MODES : nphi - 2;
    if (m_first < 0 || m_count < 1 || m_first > m_max || m_count > m_max - m_first + 1)
        return fail(SOSRT_E_INVALID, "%s: modes m_first=%d, m_count=%d: need m_first >= 0, m_count >= 1 and the last mode <= "
                                     "min(SOSRT_MAX_MODES, nphi - 2) = %d", what, m_first, m_count, m_max);
    return 0;
}

// the view cosines of the entry points of section 22, as the view stage takes them (sosrt_view_radiance_dev)
static int brdf_view_mu(int V, const double* mu_view, ViewMu& vm, const char* what) {
    if (V < 1 || V > SOSRT_MAX_VIEWS) return fail(SOSRT_E_INVALID, "%s: V=%d view cosines: must be 1..%d", what, V, SOSRT_MAX_VIEWS);
    if (!mu_view) return fail(SOSRT_E_INVALID, "%s: null mu_view", what);
    for (int v = 0; v < V; ++v)
        if (!(std::isfinite(mu_view[v]) && mu_view[v] >= 0.01 && mu_view[v] <= 1))
            return fail(SOSRT_E_INVALID, "%s: mu_view[%d] = %g: a view cosine must be finite and in [0.01, 1]", what, v, mu_view[v]);
    for (int j = 0; j < 2 * kMaxViews; ++j) vm.s[j] = j < V ? mu_view[j] : 1.0;
    return 0;
}

// The one path of the six builders (launch_brdf_pairs), entry point `what`: the handle and, where the call is per column (`beam`:
// the second direction is d_mu0 [B], else the grid's downward nodes), B; the BRDF and its node count; the range of modes where the
// call has one (`modes`, else mode 0 alone: the azimuth mean); the view cosines where it has them (`views`, else the grid's upward
// nodes); the pointers.  In this order for every entry point, and all of it before the launch: a refused call writes nothing.
static int brdf_build(sosrt_handle* h, const char* what, bool beam, int B, bool views, int V, const double* mu_view, int kind,
                      const double* params, int nparams, int nphi, bool modes, int m_first, int m_count, int sign_odd,
                      const double* d_mu0, double* d_out) {
    if (int e = brdf_check(h, B, beam, what)) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, nphi, bp, what)) return e;
    if (modes)
        if (int e = brdf_mode_range(m_first, m_count, nphi, what)) return e;
    ViewMu vm = {};
    if (views)
        if (int e = brdf_view_mu(V, mu_view, vm, what)) return e;
    if ((beam && !d_mu0) || !d_out) return fail(SOSRT_E_INVALID, "%s: null argument", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_pairs(h->stream, h->g, vm, views ? V : 0, B, bp, nphi, modes ? m_first : 0, modes ? m_count : 1, sign_odd,
                      beam ? d_mu0 : nullptr, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

int sosrt_brdf_operator_dev(sosrt_t* h, int kind, const double* params, int nparams, int nphi, double* d_R_out) {
    return brdf_build(h, "sosrt_brdf_operator_dev", false, 0, false, 0, nullptr, kind, params, nparams, nphi, false, 0, 1, 0, nullptr,
                      d_R_out);
}

int sosrt_brdf_beam_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, int nphi, const double* d_mu0,
                        double* d_r0_out) {
    return brdf_build(h, "sosrt_brdf_beam_dev", true, B, false, 0, nullptr, kind, params, nparams, nphi, false, 0, 1, 0, d_mu0,
                      d_r0_out);
}

int sosrt_brdf_operator_modes_dev(sosrt_t* h, int kind, const double* params, int nparams, int nphi, int m_first, int m_count,
                                  int sign_odd, double* d_R_out) {
    return brdf_build(h, "sosrt_brdf_operator_modes_dev", false, 0, false, 0, nullptr, kind, params, nparams, nphi, true, m_first,
                      m_count, sign_odd, nullptr, d_R_out);
}

int sosrt_brdf_beam_modes_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, int nphi, int m_first, int m_count,
                              const double* d_mu0, double* d_r0_out) {
    return brdf_build(h, "sosrt_brdf_beam_modes_dev", true, B, false, 0, nullptr, kind, params, nparams, nphi, true, m_first, m_count,
                      0, d_mu0, d_r0_out);
}

int sosrt_brdf_view_rows_modes_dev(sosrt_t* h, int kind, const double* params, int nparams, int nphi, int m_first, int m_count,
                                   int sign_odd, int V, const double* mu_view, double* d_out) {
    return brdf_build(h, "sosrt_brdf_view_rows_modes_dev", false, 0, true, V, mu_view, kind, params, nparams, nphi, true, m_first,
                      m_count, sign_odd, nullptr, d_out);
}

int sosrt_brdf_view_beam_modes_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, int nphi, int m_first,
                                   int m_count, const double* d_mu0, int V, const double* mu_view, double* d_out) {
    return brdf_build(h, "sosrt_brdf_view_beam_modes_dev", true, B, true, V, mu_view, kind, params, nparams, nphi, true, m_first,
                      m_count, 0, d_mu0, d_out);
}

int sosrt_ground_source_dev(sosrt_t* h, int B, const double* d_I, const double* d_tau, const double* d_R, const double* d_r0,
                            const double* d_scale, double* d_S_out) {
    if (int e = brdf_check(h, B, true, "sosrt_ground_source_dev")) return e;
    if (!d_I || !d_tau || !d_R || !d_S_out) return fail(SOSRT_E_INVALID, "sosrt_ground_source_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_ground_source(h->stream, h->g, B, scalars_of(h), d_I, d_tau, d_R, d_r0, d_scale, d_S_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_ground_source_terms_dev(sosrt_t* h, int B, int K, const double* d_I, const double* d_tau, const double* d_R,
                                  const double* d_r0, const double* d_weight, double* d_S_out) {
    const char* what = "sosrt_ground_source_terms_dev";
    if (int e = brdf_check(h, B, true, what)) return e;
    if (int e = brdf_terms(K, what)) return e;
    if (!d_I || !d_tau || !d_R || !d_weight || !d_S_out) return fail(SOSRT_E_INVALID, "%s: null argument", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_ground_source_terms(h->stream, h->g, B, K, scalars_of(h), d_I, d_tau, d_R, d_r0, d_weight, d_S_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_ground_first_order_dev(sosrt_t* h, int B, const double* d_tau, const double* d_S, double* d_G_out, int* d_status) {
    if (int e = brdf_check(h, B, true, "sosrt_ground_first_order_dev")) return e;
    if (!d_tau || !d_S || !d_G_out) return fail(SOSRT_E_INVALID, "sosrt_ground_first_order_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_ground_first_order(h->stream, h->g, B, d_tau, d_S, d_G_out, d_status);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_bounce_accumulate_dev(sosrt_t* h, int B, const double* d_Ik, double* d_I_total, double* d_ratio_out) {
    if (int e = brdf_check(h, B, true, "sosrt_bounce_accumulate_dev")) return e;
    if (!d_Ik || !d_I_total || !d_ratio_out) return fail(SOSRT_E_INVALID, "sosrt_bounce_accumulate_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_bounce_accumulate(h->stream, h->g, B, d_Ik, d_I_total, d_ratio_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the ground's term at view lanes off the grid: what is not a builder of modes ----
int sosrt_brdf_view_beam_azimuth_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, const double* d_mu0, int V,
                                     const double* mu_view, int nphi_out, const double* d_phi, double* d_out) {
    const char* what = "sosrt_brdf_view_beam_azimuth_dev";
    if (int e = brdf_check(h, B, true, what)) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, 3, bp, what)) return e;        // (no quadrature: any valid node count)
    ViewMu vm;
    if (int e = brdf_view_mu(V, mu_view, vm, what)) return e;
    if (nphi_out < 1) return fail(SOSRT_E_INVALID, "%s: nphi_out = %d: at least one azimuth", what, nphi_out);
    if ((long long)nphi_out * B * V > 0x7fffffffLL * 256) return fail(SOSRT_E_INVALID, "%s: output too large", what);
    if (!d_mu0 || !d_phi || !d_out) return fail(SOSRT_E_INVALID, "%s: null argument", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_view_beam_azimuth(h->stream, B, vm, V, bp, d_mu0, nphi_out, d_phi, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// the one path of sosrt_view_ground_dev (d_weight is its d_scale, nullable) and sosrt_view_ground_terms_dev (`terms`, with K)
static int view_ground(sosrt_handle* h, const char* what, int B, bool terms, int K, int V, const double* mu_view, const double* d_tau,
                       const double* d_I, const double* d_Rv, const double* d_r0v, const double* d_weight, int nlev,
                       const int* levels, int accumulate, double* d_S_out, double* d_out) {
    if (int e = brdf_check(h, B, true, what)) return e;
    if (terms)
        if (int e = brdf_terms(K, what)) return e;
    ViewMu vm;
    if (int e = brdf_view_mu(V, mu_view, vm, what)) return e;
    if (nlev < 1 || !levels) return fail(SOSRT_E_INVALID, "%s: no levels", what);
    for (int i = 0; i < nlev; ++i)
        if (levels[i] < 0 || levels[i] >= h->L)
            return fail(SOSRT_E_INVALID, "%s: levels[%d] = %d is outside [0, %d)", what, i, levels[i], h->L);
    if ((d_I == nullptr) != (d_Rv == nullptr))
        return fail(SOSRT_E_INVALID, "%s: d_I and d_Rv go together (both NULL: the beam-only call)", what);
    if (!d_I && !d_r0v) return fail(SOSRT_E_INVALID, "%s: neither a field with its rows nor beam rows: no source", what);
    if (!d_tau || !d_out || (terms && !d_weight)) return fail(SOSRT_E_INVALID, "%s: null argument", what);
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    for (int l0 = 0; l0 < nlev; l0 += kViewLevels) {
        ViewLevels lv;
        lv.n = nlev - l0 < kViewLevels ? nlev - l0 : kViewLevels;
        for (int i = 0; i < kViewLevels; ++i) lv.t[i] = i < lv.n ? levels[l0 + i] : 0;
        if (terms)
            launch_view_ground_terms(h->stream, h->g, B, K, V, vm, scalars_of(h), d_I, d_tau, d_Rv, d_r0v, d_weight, nlev, lv,
                                     accumulate != 0, d_S_out, d_out + (size_t)l0 * 2 * V);
        else
            launch_view_ground(h->stream, h->g, B, V, vm, scalars_of(h), d_I, d_tau, d_Rv, d_r0v, d_weight, nlev, lv,
                               accumulate != 0, d_S_out, d_out + (size_t)l0 * 2 * V);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int sosrt_view_ground_dev(sosrt_t* h, int B, int V, const double* mu_view, const double* d_tau, const double* d_I,
                          const double* d_Rv, const double* d_r0v, const double* d_scale, int nlev, const int* levels,
                          int accumulate, double* d_S_out, double* d_out) {
    return view_ground(h, "sosrt_view_ground_dev", B, false, 0, V, mu_view, d_tau, d_I, d_Rv, d_r0v, d_scale, nlev, levels, accumulate,
                       d_S_out, d_out);
}

int sosrt_view_ground_terms_dev(sosrt_t* h, int B, int K, int V, const double* mu_view, const double* d_tau, const double* d_I,
                                const double* d_Rv, const double* d_r0v, const double* d_weight, int nlev, const int* levels,
                                int accumulate, double* d_S_out, double* d_out) {
    return view_ground(h, "sosrt_view_ground_terms_dev", B, true, K, V, mu_view, d_tau, d_I, d_Rv, d_r0v, d_weight, nlev,
                       levels, accumulate, d_S_out, d_out);
}

}  // extern "C"
