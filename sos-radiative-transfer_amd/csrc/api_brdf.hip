// BRDF ground (include/sosrt.h): the operator of a named BRDF, its beam row, the ground source of a field's
// surface row, the ground source's unscattered field and the sum over ground reflections.  Stages beside the solve: they read
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
    return fail(SOSRT_E_INVALID, "%s: unknown BRDF kind %d", what, kind);
}

extern "C" {

int sosrt_brdf_operator_dev(sosrt_t* h, int kind, const double* params, int nparams, int nphi, double* d_R_out) {
    if (int e = brdf_check(h, 0, false, "sosrt_brdf_operator_dev")) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, nphi, bp, "sosrt_brdf_operator_dev")) return e;
    if (!d_R_out) return fail(SOSRT_E_INVALID, "sosrt_brdf_operator_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_operator(h->stream, h->g, bp, nphi, d_R_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_brdf_beam_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, int nphi, const double* d_mu0,
                        double* d_r0_out) {
    if (int e = brdf_check(h, B, true, "sosrt_brdf_beam_dev")) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, nphi, bp, "sosrt_brdf_beam_dev")) return e;
    if (!d_mu0 || !d_r0_out) return fail(SOSRT_E_INVALID, "sosrt_brdf_beam_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_beam(h->stream, h->g, B, bp, nphi, d_mu0, d_r0_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// the range of Fourier modes the two mode builders take (sosrt.h)
static int brdf_mode_range(int m_first, int m_count, int nphi, const char* what) {
    const int m_max = SOSRT_MAX_MODES < nphi - 2 ? SOSRT_MAX_MODES : nphi - 2;
    if (m_first < 0 || m_count < 1 || m_first > m_max || m_count > m_max - m_first + 1)
        return fail(SOSRT_E_INVALID, "%s: modes m_first=%d, m_count=%d: need m_first >= 0, m_count >= 1 and the last mode <= "
                                     "min(SOSRT_MAX_MODES, nphi - 2) = %d", what, m_first, m_count, m_max);
    return 0;
}

int sosrt_brdf_operator_modes_dev(sosrt_t* h, int kind, const double* params, int nparams, int nphi, int m_first, int m_count,
                                  int sign_odd, double* d_R_out) {
    if (int e = brdf_check(h, 0, false, "sosrt_brdf_operator_modes_dev")) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, nphi, bp, "sosrt_brdf_operator_modes_dev")) return e;
    if (int e = brdf_mode_range(m_first, m_count, nphi, "sosrt_brdf_operator_modes_dev")) return e;
    if (!d_R_out) return fail(SOSRT_E_INVALID, "sosrt_brdf_operator_modes_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_operator_modes(h->stream, h->g, bp, nphi, m_first, m_count, sign_odd, d_R_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_brdf_beam_modes_dev(sosrt_t* h, int B, int kind, const double* params, int nparams, int nphi, int m_first, int m_count,
                              const double* d_mu0, double* d_r0_out) {
    if (int e = brdf_check(h, B, true, "sosrt_brdf_beam_modes_dev")) return e;
    BrdfParams bp;
    if (int e = brdf_params(kind, params, nparams, nphi, bp, "sosrt_brdf_beam_modes_dev")) return e;
    if (int e = brdf_mode_range(m_first, m_count, nphi, "sosrt_brdf_beam_modes_dev")) return e;
    if (!d_mu0 || !d_r0_out) return fail(SOSRT_E_INVALID, "sosrt_brdf_beam_modes_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_brdf_beam_modes(h->stream, h->g, B, bp, nphi, m_first, m_count, d_mu0, d_r0_out);
    HIPCHK(hipGetLastError());
    return 0;
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

}  // extern "C"
