// Delta-M scaling: the entry points of the Legendre moments of a tabulated phase function and of its
// truncated table.  Host code; the kernels are in deltam.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "deltam.hpp"
#include "handle.hpp"

using namespace sosrt;

static_assert(kDeltaMMaxTab == SOSRT_DELTAM_MAX_NTAB && kDeltaMMaxOrder == SOSRT_DELTAM_MAX_LMAX, "the kernels' bounds are the header's caps");

namespace {

int tables_check(sosrt_handle* h, const char* what, int S, int ntab, int lmax) {
    if (int e = need_gpu(h)) return e;
    if (S < 1 || S > 65535) return fail(SOSRT_E_INVALID, "%s: S must be 1..65535 tables (got %d)", what, S);
    if (ntab < 2 || ntab > SOSRT_DELTAM_MAX_NTAB)
        return fail(SOSRT_E_INVALID, "%s: ntab must be 2..SOSRT_DELTAM_MAX_NTAB = %d (got %d)", what, SOSRT_DELTAM_MAX_NTAB, ntab);
    if (lmax < 1 || lmax > SOSRT_DELTAM_MAX_LMAX)
        return fail(SOSRT_E_INVALID, "%s: lmax must be 1..SOSRT_DELTAM_MAX_LMAX = %d (got %d)", what, SOSRT_DELTAM_MAX_LMAX, lmax);
    return 0;
}

int ascending_check(const char* what, const double* tab_mu, int ntab) {
    for (int i = 1; tab_mu && i < ntab; ++i)
        if (!(tab_mu[i] > tab_mu[i - 1])) return fail(SOSRT_E_INVALID, "%s: tab_mu must be strictly ascending (index %d)", what, i);
    return 0;
}

// the workspace of both calls; a larger one waits for the stream, which may still read the old
int workspace(sosrt_handle* h, size_t n) {
    if (n > h->pf.d_deltam.cap) HIPCHK(hipStreamSynchronize(h->stream));
    return h->pf.d_deltam.reserve(n);
}

// what delta-M refuses of the moments chi [S][lmax + 1] (host): non-finite values, and a truncated fraction f = chi[order] that
// leaves nothing to scale
int moments_check(int S, const double* chi, int lmax, int order) {
    for (int s = 0; s < S; ++s) {
        const double* c = chi + (size_t)s * (lmax + 1);
        for (int l = 0; l <= lmax; ++l)
            if (!std::isfinite(c[l])) return fail(SOSRT_E_INVALID, "delta-M: table %d: moment %d is not finite", s, l);
        if (!(std::fabs(c[order]) < 1 - 1e-6))
            return fail(SOSRT_E_INVALID, "delta-M: table %d: f = chi[%d] = %.17g, |f| must be < 1 - 1e-6", s, order, c[order]);
    }
    return 0;
}

int delta_m_order_check(int lmax, int order) {
    if (order < 1 || order > lmax) return fail(SOSRT_E_INVALID, "delta-M: order must be 1..lmax = %d (got %d)", lmax, order);
    return 0;
}

int delta_m_launch(sosrt_handle* h, int S, const double* d_chi, int lmax, int order, const double* d_tab_mu, int ntab,
                   double* d_tab_out, double* d_f_out) {
    if (int e = workspace(h, (size_t)S * order)) return e;
    launch_phase_delta_m(h->stream, S, d_chi, lmax, order, d_tab_mu, ntab, h->pf.d_deltam.p, d_tab_out, d_f_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// runs body(d) with n doubles of device scratch, drains the stream and frees the scratch, whatever body returns
template <typename F>
int with_scratch(sosrt_handle* h, size_t n, F&& body) {
    double* d = nullptr;
    if (int e = dalloc(&d, n)) return e;
    const int rc = body(d);
    (void)hipStreamSynchronize(h->stream);
    hipFree(d);
    return rc;
}

}  // namespace

extern "C" {

int sosrt_phase_moments_dev(sosrt_t* h, int S, const double* d_tab_mu, const double* d_tab_p, int ntab, int lmax,
                            double* d_chi_out, double* d_norm_out) {
    if (int e = tables_check(h, "phase moments", S, ntab, lmax)) return e;
    if (!d_tab_p || !d_chi_out) return fail(SOSRT_E_INVALID, "phase moments: null argument");
    HIPCHK(hipSetDevice(h->device));
    if (int e = workspace(h, deltam_moments_workspace(S, ntab, lmax))) return e;
    launch_phase_moments(h->stream, S, d_tab_mu, d_tab_p, ntab, lmax, h->pf.d_deltam.p, d_chi_out, d_norm_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_moments(sosrt_t* h, int S, const double* tab_mu, const double* tab_p, int ntab, int lmax, double* chi_out,
                        double* norm_out) {
    if (int e = tables_check(h, "phase moments", S, ntab, lmax)) return e;
    if (!tab_p || !chi_out) return fail(SOSRT_E_INVALID, "phase moments: null argument");
    if (int e = ascending_check("phase moments", tab_mu, ntab)) return e;
    HIPCHK(hipSetDevice(h->device));
    const size_t np = (size_t)S * ntab, nc = (size_t)S * (lmax + 1);
    return with_scratch(h, np + ntab + nc + S, [&](double* d) -> int {
        hipStream_t s = h->stream;
        double *d_p = d, *d_mu = d + np, *d_chi = d_mu + ntab, *d_norm = d_chi + nc;
        HIPCHK(hipMemcpyAsync(d_p, tab_p, np * sizeof(double), hipMemcpyHostToDevice, s));
        if (tab_mu) HIPCHK(hipMemcpyAsync(d_mu, tab_mu, ntab * sizeof(double), hipMemcpyHostToDevice, s));
        if (int e = sosrt_phase_moments_dev(h, S, tab_mu ? d_mu : nullptr, d_p, ntab, lmax, d_chi, d_norm)) return e;
        HIPCHK(hipMemcpyAsync(chi_out, d_chi, nc * sizeof(double), hipMemcpyDeviceToHost, s));
        if (norm_out) HIPCHK(hipMemcpyAsync(norm_out, d_norm, S * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

int sosrt_phase_delta_m_dev(sosrt_t* h, int S, const double* d_chi, int lmax, int order, const double* d_tab_mu, int ntab,
                            double* d_tab_out, double* d_f_out) {
    if (int e = tables_check(h, "delta-M", S, ntab, lmax)) return e;
    if (int e = delta_m_order_check(lmax, order)) return e;
    if (!d_chi || !d_tab_out) return fail(SOSRT_E_INVALID, "delta-M: null argument");
    HIPCHK(hipSetDevice(h->device));
    // the refusals need the moments on the host: S (lmax + 1) doubles, the one wait of this entry
    std::vector<double> chi((size_t)S * (lmax + 1));
    HIPCHK(hipMemcpyAsync(chi.data(), d_chi, chi.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (int e = moments_check(S, chi.data(), lmax, order)) return e;
    return delta_m_launch(h, S, d_chi, lmax, order, d_tab_mu, ntab, d_tab_out, d_f_out);
}

int sosrt_phase_delta_m(sosrt_t* h, int S, const double* chi, int lmax, int order, const double* tab_mu, int ntab, double* tab_out,
                        double* f_out) {
    if (int e = tables_check(h, "delta-M", S, ntab, lmax)) return e;
    if (int e = delta_m_order_check(lmax, order)) return e;
    if (!chi || !tab_out) return fail(SOSRT_E_INVALID, "delta-M: null argument");
    if (int e = ascending_check("delta-M", tab_mu, ntab)) return e;
    if (int e = moments_check(S, chi, lmax, order)) return e;
    HIPCHK(hipSetDevice(h->device));
    const size_t np = (size_t)S * ntab, nc = (size_t)S * (lmax + 1);
    return with_scratch(h, np + ntab + nc + S, [&](double* d) -> int {
        hipStream_t s = h->stream;
        double *d_out = d, *d_mu = d + np, *d_chi = d_mu + ntab, *d_f = d_chi + nc;
        HIPCHK(hipMemcpyAsync(d_chi, chi, nc * sizeof(double), hipMemcpyHostToDevice, s));
        if (tab_mu) HIPCHK(hipMemcpyAsync(d_mu, tab_mu, ntab * sizeof(double), hipMemcpyHostToDevice, s));
        if (int e = delta_m_launch(h, S, d_chi, lmax, order, tab_mu ? d_mu : nullptr, ntab, d_out, d_f)) return e;
        HIPCHK(hipMemcpyAsync(tab_out, d_out, np * sizeof(double), hipMemcpyDeviceToHost, s));
        if (f_out) HIPCHK(hipMemcpyAsync(f_out, d_f, S * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

int sosrt_phase_p0_normaliser_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, double* d_Z_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (B < 1 || !d_mu0 || !d_Z_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    PhaseJob j = phase_job(h, kind, g);
    j.mu0 = d_mu0; j.B = B; j.out = d_Z_out;
    launch_phase_p0_normaliser(h->stream, h->g, j);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
