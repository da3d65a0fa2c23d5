// Phase functions on the device: the table of SOSRT_PHASE_TABLE, Lorenz-Mie tables, the builders of P0 and
// of the phase matrix, their Fourier modes in azimuth, order targets and the azimuth synthesis.  Host code;
// the builders' kernels are in phase.hip, the Mie and synthesis kernels in epilogue.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.hpp"

using namespace sosrt;

namespace {

// np.linspace(a, b, n): i * step + a with the last point set to b (no contraction of the product and the sum)
void mie_linspace(double a, double b, int n, double* out) {
    if (n == 1) { out[0] = a; return; }
    const double step = (b - a) / (n - 1);
    for (int i = 0; i < n; ++i) {
        volatile double t = i * step;
        out[i] = t + a;
    }
    out[n - 1] = b;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
// phase functions on the device
// ---------------------------------------------------------------------------------------------
int sosrt_phase_table(sosrt_t* h, const double* tab_mu, const double* tab_p, int ntab) {
    if (int e = need_gpu(h)) return e;
    if (!tab_mu || !tab_p || ntab < 2) return fail(SOSRT_E_INVALID, "a table needs at least two points");
    for (int i = 1; i < ntab; ++i)
        if (!(tab_mu[i] > tab_mu[i - 1])) return fail(SOSRT_E_INVALID, "tab_mu must be strictly ascending (index %d)", i);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->pf.d_tab) { hipFree(h->pf.d_tab); h->pf.d_tab = nullptr; h->pf.ntab = 0; }
    if (int e = dalloc(&h->pf.d_tab, 2 * (size_t)ntab)) return e;
    HIPCHK(hipMemcpy(h->pf.d_tab, tab_mu, ntab * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->pf.d_tab + ntab, tab_p, ntab * sizeof(double), hipMemcpyHostToDevice));
    h->pf.ntab = ntab;
    return 0;
}

int sosrt_phase_table_dev(sosrt_t* h, const double* d_tab_mu, const double* d_tab_p, int ntab) {
    if (int e = need_gpu(h)) return e;
    if (!d_tab_p || ntab < 2) return fail(SOSRT_E_INVALID, "a table needs at least two points");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (h->pf.ntab != ntab || !h->pf.d_tab) {                      // (a table of the same length is overwritten in stream order)
        HIPCHK(hipStreamSynchronize(s));
        if (h->pf.d_tab) { hipFree(h->pf.d_tab); h->pf.d_tab = nullptr; h->pf.ntab = 0; }
        if (int e = dalloc(&h->pf.d_tab, 2 * (size_t)ntab)) return e;
        h->pf.ntab = ntab;
    }
    if (d_tab_mu) {
        HIPCHK(hipMemcpyAsync(h->pf.d_tab, d_tab_mu, ntab * sizeof(double), hipMemcpyDeviceToDevice, s));
    } else {
        std::vector<double> mu(ntab);
        mie_linspace(-1.0, 1.0, ntab, mu.data());
        HIPCHK(hipMemcpyAsync(h->pf.d_tab, mu.data(), ntab * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                     // (mu leaves scope)
    }
    HIPCHK(hipMemcpyAsync(h->pf.d_tab + ntab, d_tab_p, ntab * sizeof(double), hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Lorenz-Mie tables on the device
// ---------------------------------------------------------------------------------------------
namespace {

struct MiePlan {
    int S = 0, R = 0, ntab = 0, n_cap = 0;
    size_t o_x, o_radii, o_mu, o_tn, o_mre, o_mim, o_rm, o_sig, o_nmax, o_nstart, in_bytes;   // staged by the host
    size_t o_ab, o_qw, o_part, o_p, o_bulk, bytes;                                              // written by the kernels
};

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// Terms of the series and start of the downward recurrence, as mie.mie_coefficients counts them
int mie_counts(double m_re, double m_im, double x, int* nmax, int* nstart) {
    if (!(x > 0) || !std::isfinite(x) || !std::isfinite(m_re) || !std::isfinite(m_im) || (m_re == 0 && m_im == 0))
        return fail(SOSRT_E_INVALID, "Mie: the size parameter must be positive and finite and the refractive index non-zero (x = %g, m = %g%+gi)", x, m_re, m_im);
    const double amx = std::hypot(m_re * x, m_im * x);
    if (x > SOSRT_MIE_MAX_X || amx > SOSRT_MIE_MAX_MX)
        return fail(SOSRT_E_INVALID, "Mie: x = %g, |m x| = %g are beyond the caps SOSRT_MIE_MAX_X = %g, SOSRT_MIE_MAX_MX = %g", x,
                    amx, (double)SOSRT_MIE_MAX_X, (double)SOSRT_MIE_MAX_MX);
    *nmax = (int)std::nearbyint(x + 4.0 * std::pow(x, 1.0 / 3.0) + 2.0);
    *nstart = (int)(std::max((double)*nmax, amx) + 16);
    return 0;
}

// Lays the call out, grows the arena and the staging buffer, and waits until the staging buffer may be refilled
int mie_prepare(sosrt_handle* h, MiePlan& p, bool tables) {
    const size_t n = (size_t)p.S * p.R;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    p.o_x = take(n * 8); p.o_radii = take((size_t)p.R * 8); p.o_mu = take((size_t)p.ntab * 8); p.o_tn = take(((size_t)p.n_cap + 1) * 8);
    p.o_mre = take((size_t)p.S * 8); p.o_mim = take((size_t)p.S * 8); p.o_rm = take((size_t)p.S * 8); p.o_sig = take((size_t)p.S * 8);
    p.o_nmax = take(n * 4); p.o_nstart = take(n * 4);
    p.in_bytes = o;
    p.o_ab = take(n * p.n_cap * 4 * 8); p.o_qw = take(n * kMieQ * 8);
    p.o_part = take(tables ? (size_t)p.S * mie_chunks(p.R) * p.ntab * 8 : 0);
    p.o_p = take(tables ? (size_t)p.S * p.ntab * 8 : 0); p.o_bulk = take((size_t)p.S * 3 * 8);
    p.bytes = o;
    if (p.bytes > (size_t)SOSRT_MIE_MAX_WORKSPACE)
        return fail(SOSRT_E_INVALID, "Mie: the call needs %zu bytes of workspace, more than SOSRT_MIE_MAX_WORKSPACE = %zu: split it", p.bytes,
                    (size_t)SOSRT_MIE_MAX_WORKSPACE);
    HIPCHK(hipSetDevice(h->device));
    if (!h->pf.mie_ev) {
        HIPCHK(hipEventCreateWithFlags(&h->pf.mie_ev, hipEventDisableTiming));
        for (auto& e : h->pf.mie_t) HIPCHK(hipEventCreate(&e));
    }
    if (p.bytes > h->pf.d_mie.cap) HIPCHK(hipStreamSynchronize(h->stream));
    if (int e = h->pf.d_mie.reserve(p.bytes)) return e;
    HIPCHK(hipEventSynchronize(h->pf.mie_ev));                  // (never recorded: returns at once)
    return h->pf.h_mie.reserve(p.in_bytes);
}

// stages the inputs, copies them and launches the coefficient kernel (with `tables`, the other two as well)
int mie_run(sosrt_handle* h, const MiePlan& p, bool tables) {
    hipStream_t s = h->stream;
    double* tn = (double*)(h->pf.h_mie.p + p.o_tn);
    tn[0] = 0;
    for (int n = 1; n <= p.n_cap; ++n) tn[n] = (n + 1.0) / n;
    HIPCHK(hipMemcpyAsync(h->pf.d_mie.p, h->pf.h_mie.p, p.in_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->pf.mie_ev, s));
    char* d = h->pf.d_mie.p;
    auto D = [&](size_t off) { return (double*)(d + off); };
    const int n = p.S * p.R;
    HIPCHK(hipEventRecord(h->pf.mie_t[0], s));
    launch_mie_coefficients(s, n, p.R, p.n_cap, D(p.o_x), (const int*)(d + p.o_nmax), (const int*)(d + p.o_nstart), D(p.o_mre),
                            D(p.o_mim), tables ? D(p.o_radii) : nullptr, D(p.o_rm), D(p.o_sig), D(p.o_ab), D(p.o_qw));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->pf.mie_t[1], s));
    if (tables) {
        launch_mie_angles(s, p.S, p.R, p.ntab, p.n_cap, D(p.o_mu), D(p.o_ab), (const int*)(d + p.o_nmax), D(p.o_tn), D(p.o_qw),
                          D(p.o_part));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->pf.mie_t[2], s));
        launch_mie_integrate(s, p.S, p.R, p.ntab, D(p.o_part), D(p.o_radii), D(p.o_qw), D(p.o_p), D(p.o_bulk));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->pf.mie_t[3], s));
    }
    h->pf.mie_timed = tables;
    return 0;
}

int mie_ensembles(sosrt_handle* h, int S, const double* wl, const double* m_re, const double* m_im, const double* r_m,
                  const double* sig, int nb_radius, double r_min, double r_max, int ntab, double* p_out, double* bulk_out,
                  bool dev) {
    if (int e = need_gpu(h)) return e;
    if (S < 1 || !wl || !m_re || !m_im || !p_out) return fail(SOSRT_E_INVALID, "Mie: need S >= 1, wl, m_re, m_im and p_out");
    if (ntab < 2) return fail(SOSRT_E_INVALID, "Mie: a table needs at least two points (ntab = %d)", ntab);
    if (nb_radius < 1) return fail(SOSRT_E_INVALID, "Mie: nb_radius must be >= 1 (got %d)", nb_radius);
    if (!(r_min > 0) || !std::isfinite(r_min)) return fail(SOSRT_E_INVALID, "Mie: r_min must be positive (got %g)", r_min);
    if (nb_radius > 1 && (!(r_max > r_min) || !std::isfinite(r_max))) return fail(SOSRT_E_INVALID, "Mie: need r_max > r_min (got %g, %g)", r_max, r_min);
    if (nb_radius > 1 && (!r_m || !sig)) return fail(SOSRT_E_INVALID, "Mie: an ensemble needs r_m and sig");
    if ((long long)S * nb_radius > (1 << 24)) return fail(SOSRT_E_INVALID, "Mie: S * nb_radius too large");
    if (S > 65535) return fail(SOSRT_E_INVALID, "Mie: at most 65535 ensembles in a call");
    for (int s = 0; s < S; ++s) {
        if (!(wl[s] > 0) || !std::isfinite(wl[s])) return fail(SOSRT_E_INVALID, "Mie: ensemble %d: the wavelength must be positive (got %g)", s, wl[s]);
        if (nb_radius > 1 && (!(sig[s] > 1) || !std::isfinite(sig[s]))) return fail(SOSRT_E_INVALID, "Mie: ensemble %d: sig must be > 1 (got %g)", s, sig[s]);
        if (nb_radius > 1 && (!(r_m[s] > 0) || !std::isfinite(r_m[s]))) return fail(SOSRT_E_INVALID, "Mie: ensemble %d: r_m must be positive (got %g)", s, r_m[s]);
    }
    const int R = nb_radius;
    std::vector<double> radii(R), x((size_t)S * R);
    std::vector<int> nmax((size_t)S * R), nstart((size_t)S * R);
    mie_linspace(r_min, r_max, R, radii.data());
    MiePlan p;
    p.S = S; p.R = R; p.ntab = ntab;
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < R; ++i) {
            const size_t k = (size_t)s * R + i;
            x[k] = 2 * M_PI * radii[i] / wl[s];              // (2 pi r) / wl, as mie.log_normal_bulk_phase writes it
            if (int e = mie_counts(m_re[s], m_im[s], x[k], &nmax[k], &nstart[k])) return e;
            p.n_cap = std::max(p.n_cap, nmax[k]);
        }
    if (int e = mie_prepare(h, p, true)) return e;
    char* hm = h->pf.h_mie.p;
    memcpy(hm + p.o_x, x.data(), x.size() * 8);
    memcpy(hm + p.o_radii, radii.data(), radii.size() * 8);
    mie_linspace(-1.0, 1.0, ntab, (double*)(hm + p.o_mu));
    memcpy(hm + p.o_mre, m_re, (size_t)S * 8);
    memcpy(hm + p.o_mim, m_im, (size_t)S * 8);
    for (int s = 0; s < S; ++s) {
        ((double*)(hm + p.o_rm))[s] = R > 1 ? r_m[s] : 1.0;
        ((double*)(hm + p.o_sig))[s] = R > 1 ? sig[s] : 2.0;
    }
    memcpy(hm + p.o_nmax, nmax.data(), nmax.size() * 4);
    memcpy(hm + p.o_nstart, nstart.data(), nstart.size() * 4);
    if (int e = mie_run(h, p, true)) return e;
    hipStream_t st = h->stream;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(p_out, h->pf.d_mie.p + p.o_p, (size_t)S * ntab * 8, kind, st));
    if (bulk_out) HIPCHK(hipMemcpyAsync(bulk_out, h->pf.d_mie.p + p.o_bulk, (size_t)S * 3 * 8, kind, st));
    if (!dev) HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int sosrt_mie_ensembles(sosrt_t* h, int S, const double* wl, const double* m_re, const double* m_im, const double* r_m,
                        const double* sig, int nb_radius, double r_min, double r_max, int ntab, double* p_out, double* bulk_out) {
    return mie_ensembles(h, S, wl, m_re, m_im, r_m, sig, nb_radius, r_min, r_max, ntab, p_out, bulk_out, false);
}

int sosrt_mie_ensembles_dev(sosrt_t* h, int S, const double* wl, const double* m_re, const double* m_im, const double* r_m,
                            const double* sig, int nb_radius, double r_min, double r_max, int ntab, double* d_p_out,
                            double* d_bulk_out) {
    return mie_ensembles(h, S, wl, m_re, m_im, r_m, sig, nb_radius, r_min, r_max, ntab, d_p_out, d_bulk_out, true);
}

int sosrt_mie_efficiencies(sosrt_t* h, int K, const double* m_re, const double* m_im, const double* x, double* out) {
    if (int e = need_gpu(h)) return e;
    if (K < 1 || K > (1 << 24) || !m_re || !m_im || !x || !out) return fail(SOSRT_E_INVALID, "Mie: need 1 <= K <= 2^24, m_re, m_im, x and out");
    std::vector<int> nmax(K), nstart(K);
    MiePlan p;
    p.S = K; p.R = 1; p.ntab = 0;
    for (int k = 0; k < K; ++k) {
        if (int e = mie_counts(m_re[k], m_im[k], x[k], &nmax[k], &nstart[k])) return e;
        p.n_cap = std::max(p.n_cap, nmax[k]);
    }
    if (int e = mie_prepare(h, p, false)) return e;
    char* hm = h->pf.h_mie.p;
    memcpy(hm + p.o_x, x, (size_t)K * 8);
    memcpy(hm + p.o_mre, m_re, (size_t)K * 8);
    memcpy(hm + p.o_mim, m_im, (size_t)K * 8);
    memcpy(hm + p.o_nmax, nmax.data(), (size_t)K * 4);
    memcpy(hm + p.o_nstart, nstart.data(), (size_t)K * 4);
    if (int e = mie_run(h, p, false)) return e;
    hipStream_t st = h->stream;
    std::vector<double> q((size_t)K * kMieQ);
    HIPCHK(hipMemcpyAsync(q.data(), h->pf.d_mie.p + p.o_qw, q.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) memcpy(out + 4 * (size_t)k, q.data() + (size_t)k * kMieQ, 4 * sizeof(double));
    return 0;
}

int sosrt_mie_timing(sosrt_t* h, double* ms) {
    if (int e = need_gpu(h)) return e;
    if (!ms) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->pf.mie_timed) return fail(SOSRT_E_STATE, "sosrt_mie_ensembles has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->pf.mie_t[3]));
    for (int k = 0; k < 3; ++k) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, h->pf.mie_t[k], h->pf.mie_t[k + 1]));
        ms[k] = t;
    }
    return 0;
}

}  // extern "C"

int sosrt::phase_check(sosrt_handle* h, int kind, double g) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (kind < SOSRT_PHASE_ISO || kind > SOSRT_PHASE_TABLE) return fail(SOSRT_E_INVALID, "unknown phase-function kind %d", kind);
    if (kind == SOSRT_PHASE_TABLE && !h->pf.d_tab) return fail(SOSRT_E_STATE, "sosrt_phase_table has not been called");
    if (kind == SOSRT_PHASE_HG && !(std::fabs(g) < 1)) return fail(SOSRT_E_INVALID, "|g| must be < 1 (got %g)", g);
    return 0;
}

PhaseFn sosrt::phase_fn(const sosrt_handle* h, int kind, double g) {
    PhaseFn p{};
    p.kind = kind; p.g = g;
    p.tab_mu = h->pf.d_tab; p.tab_p = h->pf.d_tab ? h->pf.d_tab + h->pf.ntab : nullptr; p.ntab = h->pf.ntab;
    return p;
}

PhaseJob sosrt::phase_job(const sosrt_handle* h, int kind, double g, int mf, int mc, int nphi) {
    PhaseJob j{};
    j.p = phase_fn(h, kind, g);
    j.w = h->grid.d_w;
    j.cosphi = mc ? h->pf.d_modetab.p : h->grid.d_phi;
    j.wq = mc ? h->pf.d_modetab.p + nphi : h->grid.d_phi + kNPhi;
    j.nphi = mc ? nphi : kNPhi;
    j.m_first = mf; j.m_count = mc;
    return j;
}

namespace {

// A host-pointer entry around its device entry: n doubles of output (and `extra` more of scratch behind them) are allocated, dev
// fills them on the handle's stream, they are copied out, the stream is synchronised and the buffer freed
template <typename F>
int to_host(sosrt_handle* h, size_t n, size_t extra, double* out, F&& dev) {
    hipStream_t s = h->stream;
    double* d = nullptr;
    if (int e = dalloc(&d, n + extra)) return e;
    auto body = [&]() -> int {
        if (int e = dev(d)) return e;
        HIPCHK(hipMemcpyAsync(out, d, n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    (void)hipStreamSynchronize(s);
    hipFree(d);
    return rc;
}

// Modes [m_first, m_first + m_count) of the matrix (d_mu0 == nullptr, out [m_count][D][D]) or of P0 (out [m_count][B][D]): mode 0
// is the 25-node builder's output, bit for bit; the modes m >= 1 of the request come from the mode builder on nphi nodes
int build_modes(sosrt_handle* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, int B, const double* d_mu0,
                double* d_out) {
    const int mf = m_first > 0 ? m_first : 1, mc = m_first > 0 ? m_count : m_count - 1;   // modes m >= 1 of the request
    PhaseJob j = phase_job(h, kind, g);
    j.mu0 = d_mu0; j.B = B; j.out = d_out;
    if (m_first == 0) launch_phase_builder(h->stream, h->g, nullptr, j);
    if (mc > 0) {
        if (int e = modes_table(h, nphi, mf, mc)) return e;
        j = phase_job(h, kind, g, mf, mc, nphi);
        j.sign_odd = sign_odd; j.mu0 = d_mu0; j.B = B;
        j.out = d_out + (size_t)(m_count - mc) * (d_mu0 ? B : h->D) * h->D;
        launch_phase_builder(h->stream, h->g, nullptr, j);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int sosrt_phase_p0_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, double* d_P0_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (B < 1 || !d_mu0 || !d_P0_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return build_modes(h, kind, g, 0, 1, 0, 0, B, d_mu0, d_P0_out);
}

int sosrt_phase_p0(sosrt_t* h, int B, int kind, double g, const double* mu0, double* P0_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (B < 1 || B > h->max_batch || !mu0 || !P0_out) return fail(SOSRT_E_INVALID, "bad argument (B must be 1..max_batch)");
    for (int b = 0; b < B; ++b)
        if (!(mu0[b] > 0 && mu0[b] <= 1)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be in (0, 1]", b);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->fld.d_ratio, mu0, B * sizeof(double), hipMemcpyHostToDevice, s));
    if (int e = sosrt_phase_p0_dev(h, B, kind, g, h->fld.d_ratio, h->fld.d_P0a)) return e;
    HIPCHK(hipMemcpyAsync(P0_out, h->fld.d_P0a, (size_t)B * h->D * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int sosrt_phase_matrix_dev(sosrt_t* h, int kind, double g, double* d_P_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (!d_P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return build_modes(h, kind, g, 0, 1, 0, 0, 0, nullptr, d_P_out);
}

int sosrt_phase_matrix(sosrt_t* h, int kind, double g, double* P_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (!P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return to_host(h, (size_t)h->D * h->D, 0, P_out, [&](double* dP) { return sosrt_phase_matrix_dev(h, kind, g, dP); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Fourier modes in azimuth
// ---------------------------------------------------------------------------------------------
int sosrt::modes_check(sosrt_handle* h, int kind, double g, int m_first, int m_count, int nphi) {
    if (int e = phase_check(h, kind, g)) return e;
    if (m_first < 0 || m_count < 1) return fail(SOSRT_E_INVALID, "modes: need m_first >= 0 and m_count >= 1 (got %d, %d)", m_first, m_count);
    const int m_last = m_first + m_count - 1;
    if (m_last > SOSRT_MAX_MODES) return fail(SOSRT_E_INVALID, "modes: the highest mode is %d, at most SOSRT_MAX_MODES = %d", m_last, SOSRT_MAX_MODES);
    if (m_last >= 1 && m_last > nphi - 2)
        return fail(SOSRT_E_INVALID, "modes: mode %d needs nphi >= %d (a trapezoid rule of nphi points on [0, pi] aliases higher modes; got %d)",
                    m_last, m_last + 2, nphi);
    return 0;
}

// uploads cos(phi_q) and the weights of modes [mf, mf + mc) (row 0: the m = 0 ring) for phi = linspace(0, pi, nphi);
// synchronises the handle's stream first: an earlier builder may still read the buffer
int sosrt::modes_table(sosrt_handle* h, int nphi, int mf, int mc) {
    const size_t need = (size_t)(2 + mc) * nphi;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (int e = h->pf.d_modetab.reserve(need)) return e;
    std::vector<double> phi(nphi), t(need);
    const double pi = 3.141592653589793, step = pi / (nphi - 1);
    for (int q = 0; q < nphi; ++q) phi[q] = q * step;          // np.linspace(0, pi, nphi)
    phi[nphi - 1] = pi;
    for (int q = 0; q < nphi; ++q) {
        const double w = ((q > 0 ? phi[q] - phi[q - 1] : 0.0) + (q + 1 < nphi ? phi[q + 1] - phi[q] : 0.0)) / 2;
        t[q] = std::cos(phi[q]);
        t[nphi + q] = w;
        for (int j = 1; j <= mc; ++j) t[(size_t)(1 + j) * nphi + q] = w * std::cos((mf + j - 1) * phi[q]);
    }
    HIPCHK(hipMemcpy(h->pf.d_modetab.p, t.data(), need * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

extern "C" {

int sosrt_phase_modes_dev(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, double* d_P_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (!d_P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return build_modes(h, kind, g, m_first, m_count, nphi, sign_odd, 0, nullptr, d_P_out);
}

int sosrt_phase_modes(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, double* P_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (!P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return to_host(h, (size_t)m_count * h->D * h->D, 0, P_out,
                   [&](double* dP) { return sosrt_phase_modes_dev(h, kind, g, m_first, m_count, nphi, 0, dP); });
}

int sosrt_phase_p0_modes_dev(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* d_mu0,
                             double* d_P0_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (B < 1 || !d_mu0 || !d_P0_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return build_modes(h, kind, g, m_first, m_count, nphi, 0, B, d_mu0, d_P0_out);
}

int sosrt_phase_p0_modes(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* mu0,
                         double* P0_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (B < 1 || B > h->max_batch || !mu0 || !P0_out) return fail(SOSRT_E_INVALID, "bad argument (B must be 1..max_batch)");
    for (int b = 0; b < B; ++b)
        if (!(mu0[b] > 0 && mu0[b] <= 1)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be in (0, 1]", b);
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)m_count * B * h->D;
    return to_host(h, n, B, P0_out, [&](double* dP) -> int {
        HIPCHK(hipMemcpyAsync(dP + n, mu0, B * sizeof(double), hipMemcpyHostToDevice, h->stream));
        return sosrt_phase_p0_modes_dev(h, B, kind, g, m_first, m_count, nphi, dP + n, dP);
    });
}

int sosrt_set_order_targets(sosrt_t* h, const int* d_targets) {
    if (int e = need_gpu(h)) return e;
    h->d_targets = d_targets;
    return 0;
}

int sosrt_azimuth_accumulate_dev(sosrt_t* h, int B, int m, const double* d_Im, int nlev, const int* d_levels, int nphi_out,
                                 const double* d_phi, double* d_out) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || m < 0 || nlev < 1 || nphi_out < 1 || !d_Im || !d_levels || !d_phi || !d_out)
        return fail(SOSRT_E_INVALID, "azimuth accumulate: bad argument (B=%d m=%d nlev=%d nphi_out=%d)", B, m, nlev, nphi_out);
    if ((long long)B * nlev > 0x7fffffffLL) return fail(SOSRT_E_INVALID, "azimuth accumulate: B * nlev too large");
    HIPCHK(hipSetDevice(h->device));
    launch_azimuth_accumulate(h->stream, h->g, B, m, d_Im, nlev, d_levels, nphi_out, d_phi, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_azimuth_synthesize_dev(sosrt_t* h, int B, int M, const double* d_I0, const double* d_Im, int nlev, const int* d_levels,
                                 int nphi_out, const double* d_phi, double* d_out) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || M < 0 || M > SOSRT_MAX_MODES || nlev < 1 || nphi_out < 1 || !d_I0 || (M > 0 && !d_Im) || !d_levels || !d_phi || !d_out)
        return fail(SOSRT_E_INVALID, "azimuth synthesize: bad argument (B=%d M=%d nlev=%d nphi_out=%d; M is at most SOSRT_MAX_MODES = %d)",
                    B, M, nlev, nphi_out, SOSRT_MAX_MODES);
    if ((long long)B * nlev > 0x7fffffffLL) return fail(SOSRT_E_INVALID, "azimuth synthesize: B * nlev too large");
    HIPCHK(hipSetDevice(h->device));
    launch_azimuth_synthesize(h->stream, h->g, B, M, d_I0, d_Im, nlev, d_levels, nphi_out, d_phi, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
