// BRDF ground, gfx950: the stages of the series in ground reflections that runs around the order loop.
//
//   k_brdf_operator        R(i, j) = 2 w_j |mu_j| rho_bar(mu_i, |mu_j|): one lane per pair, the azimuth nodes in a loop; every
//                          (pair, node) is evaluated once, the cosines of a chunk of nodes come from LDS.
//   k_brdf_beam            r0[b][i] = rho_bar(mu_i, mu0[b]): one lane per (column, upward lane), the same loop.
//   k_brdf_operator_modes   the Fourier modes m of R in azimuth, R^m(i, j) = 2 w_j |mu_j| rho^m(mu_i, |mu_j|), the same
//   k_brdf_beam_modes      layout and loop: rho at a (pair, node) feeds the register accumulators of up to 8 modes per launch, the
//                          nodes' weights times cos(m phi) come from LDS; mode 0 has the bits of the two kernels above.
//   k_ground_source        S = scale (R I_surface + r0 e^{-tau*/mu0}): one workgroup per column, the surface row in LDS, one lane
//                          per upward lane i, fused multiply-adds over j ascending (R is stored with the lanes i of one j contiguous).
//   k_ground_first_order   the unscattered upward field of S with the mu -> 0+ blend of the order loop's upward sweep on every
//                          row: one workgroup per column, one wave per row, the row in LDS for the blend's search.
//   k_bounce_accumulate    total += Ik and the column's ratio of the two fields on the TOA-up and surface-down lanes.
//   k_brdf_view_rows_modes the same modes at view cosines off the grid, 2 w_j |mu_j| rho^m(mu_view_v, |mu_j|) and
//   k_brdf_view_beam_modes rho^m(mu_view_v, mu0_b): the layout and loop of the two mode kernels, their bits at a node.
//   k_brdf_view_beam_azimuth rho(mu_view_v, mu0_b, phi) at an azimuth itself, no quadrature.
//   k_view_ground          the ground's unscattered radiance at the view lanes: k_ground_source's chain with the view rows, one
//                          exp per (level, lane); downward lanes +0; written or accumulated.
//
// The kernels read the grid, the columns' mu0 (ColScalars) and their arguments, and write nothing but their outputs.
#include "brdf.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

constexpr int kPhiChunk = 256;         // azimuth nodes whose cosines a workgroup holds in LDS at a time
constexpr double kPi = 3.14159265358979323846;
constexpr int kModesPerLaunch = 8;     // Fourier modes whose accumulators a lane of the mode kernels holds in registers

// one direction of a pair: cosine, sine, tangent
struct Dir {
    double c, s, t;
};
__device__ __forceinline__ Dir make_dir(double c) {
    Dir d;
    d.c = c;
    d.s = sqrt(fmax(0.0, 1.0 - c * c));
    d.t = d.s / c;
    return d;
}

// rho(a, b, phi) of SOSRT_BRDF_RPV (sosrt.h); every term is symmetric in (a, b) as written.  hav = 1 - cos phi = 2 sin^2(phi / 2).
__device__ __forceinline__ double rpv(const BrdfParams& bp, const Dir& a, const Dir& b, double minnaert, double cphi, double hav) {
    const double rho0 = bp.p[0], th = bp.p[2];
    const double cosg = a.c * b.c + a.s * b.s * cphi;
    const double den = 1.0 + 2.0 * th * cosg + th * th;
    const double F = (1.0 - th * th) / (den * sqrt(den));
    // tan^2 a + tan^2 b - 2 tan a tan b cos phi vanishes at the hot spot (a = b, phi = 0); as written it cancels there, rounds
    // below 0, and its square root carries the square root of the rounding.  (tan a - tan b)^2 + 2 tan a tan b (1 - cos phi) is
    // the same number as a sum of two non-negative terms (the clamp stays for a NaN-free square root whatever the inputs).
    const double dt = a.t - b.t;
    const double G = sqrt(fmax(0.0, dt * dt + 2.0 * (a.t * b.t) * hav));
    return rho0 * minnaert * F * (1.0 + (1.0 - rho0) / (1.0 + G));
}

// (1 / pi) int_0^pi rho dphi by the trapezoid rule on nphi nodes; s_cos: 2 kPhiChunk doubles of the workgroup (cos phi and
// 1 - cos phi of a chunk of nodes).  Every thread of the workgroup calls this (the chunk loop holds barriers); `live` says
// whether the lane has a pair.
__device__ __forceinline__ double azimuth_mean(const BrdfParams& bp, bool live, double ca, double cb, int nphi, double* s_cos) {
    double* s_hav = s_cos + kPhiChunk;
    const Dir a = make_dir(ca), b = make_dir(cb);
    const double minnaert = bp.kind == SOSRT_BRDF_RPV ? pow(a.c * b.c * (a.c + b.c), bp.p[1] - 1.0) : 1.0;
    const double h = 1.0 / (nphi - 1);
    double acc = 0;
    for (int q0 = 0; q0 < nphi; q0 += kPhiChunk) {
        const int nq = min(kPhiChunk, nphi - q0);
        __syncthreads();
        for (int q = threadIdx.x; q < nq; q += blockDim.x) {
            const double phi = kPi * (q0 + q) * h, sh = sin(0.5 * phi);
            s_cos[q] = q0 + q == nphi - 1 ? -1.0 : cos(phi);
            s_hav[q] = q0 + q == nphi - 1 ? 2.0 : 2.0 * sh * sh;
        }
        __syncthreads();
        if (live) {
            for (int q = 0; q < nq; ++q) {
                const double v = bp.kind == SOSRT_BRDF_RPV ? rpv(bp, a, b, minnaert, s_cos[q], s_hav[q]) : 1.0;
                const double w = (q0 + q == 0 || q0 + q == nphi - 1) ? 0.5 * h : h;
                acc = fma(w, v, acc);
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_brdf_operator(Grid g, BrdfParams bp, int nphi, double* __restrict__ R) {
    __shared__ double s_cos[2 * kPhiChunk];
    const int N = g.N, M = N - 1;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < (long long)M * M;
    const int j = live ? (int)(idx / M) : 0, i = live ? (int)(idx - (long long)j * M) : 0;
    const double a = g.mu[N + 1 + i], b = -g.mu[j];
    const double rb = azimuth_mean(bp, live, a, b, nphi, s_cos);
    if (live) {
        // trapezoid weight of node j among mu[0 .. N-2]
        const double w = j == 0 ? (g.mu[1] - g.mu[0]) / 2 : j == M - 1 ? (g.mu[M - 1] - g.mu[M - 2]) / 2 : (g.mu[j + 1] - g.mu[j - 1]) / 2;
        R[idx] = 2.0 * w * b * rb;
    }
}

__global__ __launch_bounds__(256) void k_brdf_beam(Grid g, int B, BrdfParams bp, int nphi, const double* __restrict__ mu0,
                                                   double* __restrict__ r0) {
    __shared__ double s_cos[2 * kPhiChunk];
    const int N = g.N, M = N - 1;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < (long long)B * M;
    const int b = live ? (int)(idx / M) : 0, i = live ? (int)(idx - (long long)b * M) : 0;
    const double rb = azimuth_mean(bp, live, g.mu[N + 1 + i], mu0[b], nphi, s_cos);
    if (live) r0[idx] = rb;
}

// ---- Fourier modes of the BRDF in azimuth ----
// cos(m phi_q) on the nphi nodes phi_q = pi q / (nphi - 1): the integer product m q reduced modulo the 2 (nphi - 1) nodes of the
// full circle and folded onto [0, pi], so that m = 0 gives 1, node nphi - 1 gives (-1)^m and a quarter turn gives 0, all exactly.
__device__ __forceinline__ double mode_cos(int m, int q, int nphi, double h) {
    const int half = nphi - 1, period = 2 * half;
    int r = (int)(((long long)m * q) % period);
    if (r > half) r = period - r;
    if (r == 0) return 1.0;
    if (r == half) return -1.0;
    if (2 * r == half) return 0.0;
    return cos(kPi * r * h);
}

// rho^m(a, b) = (1 / pi) int_0^pi rho cos(m phi) dphi for the modes m0 .. m0 + nm - 1 (nm <= kModesPerLaunch) by the trapezoid
// rule of azimuth_mean: rho at a (pair, node) is evaluated once and feeds the accumulators of all modes, which stay in registers
// (the loops over k have a constant trip count and are unrolled; a mode k >= nm has weight 0).  s_cos: (2 + kModesPerLaunch)
// kPhiChunk doubles of the workgroup: cos phi, 1 - cos phi and per mode the weight of the node times cos(m phi) for a chunk of
// nodes.  With m = 0 the weight times 1 is the weight, so mode 0 has the bits of azimuth_mean.  Every thread of the workgroup
// calls this.
template <int NM>
__device__ __forceinline__ void azimuth_modes(const BrdfParams& bp, bool live, double ca, double cb, int nphi, int m0, int nm,
                                              double* s_cos, double (&acc)[NM]) {
    double* s_hav = s_cos + kPhiChunk;
    double* s_wc = s_cos + 2 * kPhiChunk;                    // [NM][kPhiChunk]
    const Dir a = make_dir(ca), b = make_dir(cb);
    const double minnaert = bp.kind == SOSRT_BRDF_RPV ? pow(a.c * b.c * (a.c + b.c), bp.p[1] - 1.0) : 1.0;
    const double h = 1.0 / (nphi - 1);
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0;
    for (int q0 = 0; q0 < nphi; q0 += kPhiChunk) {
        const int nq = min(kPhiChunk, nphi - q0);
        __syncthreads();
        for (int q = threadIdx.x; q < nq; q += blockDim.x) {
            const double phi = kPi * (q0 + q) * h, sh = sin(0.5 * phi);
            s_cos[q] = q0 + q == nphi - 1 ? -1.0 : cos(phi);
            s_hav[q] = q0 + q == nphi - 1 ? 2.0 : 2.0 * sh * sh;
            const double w = (q0 + q == 0 || q0 + q == nphi - 1) ? 0.5 * h : h;
#pragma unroll
            for (int k = 0; k < NM; ++k) s_wc[k * kPhiChunk + q] = k < nm ? w * mode_cos(m0 + k, q0 + q, nphi, h) : 0.0;
        }
        __syncthreads();
        if (live) {
            for (int q = 0; q < nq; ++q) {
                const double v = bp.kind == SOSRT_BRDF_RPV ? rpv(bp, a, b, minnaert, s_cos[q], s_hav[q]) : 1.0;
#pragma unroll
                for (int k = 0; k < NM; ++k) acc[k] = fma(s_wc[k * kPhiChunk + q], v, acc[k]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_brdf_operator_modes(Grid g, BrdfParams bp, int nphi, int m0, int nm, int sign_odd,
                                                             double* __restrict__ R) {
    __shared__ double s_cos[(2 + kModesPerLaunch) * kPhiChunk];
    const int N = g.N, M = N - 1;
    const long long pairs = (long long)M * M;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < pairs;
    const int j = live ? (int)(idx / M) : 0, i = live ? (int)(idx - (long long)j * M) : 0;
    const double a = g.mu[N + 1 + i], b = -g.mu[j];
    double rb[kModesPerLaunch];
    azimuth_modes<kModesPerLaunch>(bp, live, a, b, nphi, m0, nm, s_cos, rb);
    if (live) {
        const double w = j == 0 ? (g.mu[1] - g.mu[0]) / 2 : j == M - 1 ? (g.mu[M - 1] - g.mu[M - 2]) / 2 : (g.mu[j + 1] - g.mu[j - 1]) / 2;
#pragma unroll
        for (int k = 0; k < kModesPerLaunch; ++k)
            if (k < nm) {
                const double v = 2.0 * w * b * rb[k];
                R[(size_t)k * pairs + idx] = (sign_odd && ((m0 + k) & 1)) ? -v : v;
            }
    }
}

__global__ __launch_bounds__(256) void k_brdf_beam_modes(Grid g, int B, BrdfParams bp, int nphi, int m0, int nm,
                                                         const double* __restrict__ mu0, double* __restrict__ r0) {
    __shared__ double s_cos[(2 + kModesPerLaunch) * kPhiChunk];
    const int N = g.N, M = N - 1;
    const long long n = (long long)B * M;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    const int b = live ? (int)(idx / M) : 0, i = live ? (int)(idx - (long long)b * M) : 0;
    double rb[kModesPerLaunch];
    azimuth_modes<kModesPerLaunch>(bp, live, g.mu[N + 1 + i], mu0[b], nphi, m0, nm, s_cos, rb);
    if (live) {
#pragma unroll
        for (int k = 0; k < kModesPerLaunch; ++k)
            if (k < nm) r0[(size_t)k * n + idx] = rb[k];
    }
}

__global__ __launch_bounds__(1024) void k_ground_source(Grid g, int B, ColScalars sc, const double* __restrict__ I_all,
                                                        const double* __restrict__ tau_all, const double* __restrict__ R,
                                                        const double* __restrict__ r0, const double* __restrict__ scale,
                                                        double* __restrict__ S_all) {
    const int L = g.L, N = g.N, D = g.D, M = N - 1;
    const int b = blockIdx.x, i = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double s_I[];                          // [N-1] the downward surface row
    const double* row = I_all + ((size_t)b * L + (L - 1)) * D;
    for (int j = i; j < M; j += blockDim.x) s_I[j] = row[j];
    __syncthreads();
    if (i >= M) return;
    double acc = 0;
    for (int j = 0; j < M; ++j) acc = fma(R[(size_t)j * M + i], s_I[j], acc);
    if (r0) acc += r0[(size_t)b * M + i] * exp(-tau_all[(size_t)b * L + (L - 1)] / sc.mu0[b]);
    S_all[(size_t)b * M + i] = scale ? scale[b] * acc : acc;
}

constexpr int kGfoWaves = 4;

__global__ __launch_bounds__(64 * kGfoWaves) void k_ground_first_order(Grid g, int B, const double* __restrict__ tau_all,
                                                                       const double* __restrict__ S_all,
                                                                       double* __restrict__ G_all, int* __restrict__ status) {
    const int L = g.L, N = g.N, D = g.D;
    const int b = blockIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    extern __shared__ double sm[];
    double* s_S = sm;                                        // [N]: s_S[u] is the source of lane N+u (u = 0: the mu = 0 node, 0)
    double* s_row = sm + N + (size_t)wave * N;               // [N] the wave's row, lanes N .. 2N-1
    __shared__ int s_err;
    if (threadIdx.x == 0) s_err = 0;
    for (int u = threadIdx.x; u < N; u += blockDim.x) s_S[u] = u == 0 ? 0.0 : S_all[(size_t)b * (N - 1) + (u - 1)];
    const double* tau = tau_all + (size_t)b * L;
    const double tauL = tau[L - 1];
    double* Gc = G_all + (size_t)b * L * D;
    for (int t0 = 0; t0 < L; t0 += kGfoWaves) {              // (the same trips for every wave: the barriers are uniform)
        const int t = t0 + wave;
        const bool active = t < L;
        __syncthreads();
        if (active) {
            const double dt = tauL - tau[t];
            for (int u = lane; u < N; u += 64) s_row[u] = u == 0 ? 0.0 : s_S[u] * exp(-dt / g.mu[N + u]);
        }
        __syncthreads();
        if (!active) continue;
        // spec:402-409 on lanes k = N + u: the first u >= 1 whose second difference is <= 1e-4; the last u that can be tested
        // is N-3 (it reads u + 2 = N-1, lane 2N-1)
        int kf = -1;
        for (int base = 1; base <= N - 3; base += 64) {
            const int u = base + lane;
            bool pass = false;
            if (u <= N - 3) pass = !(fabs((s_row[u] - s_row[u + 1]) - (s_row[u + 1] - s_row[u + 2])) > 0.0001);
            const unsigned long long mask = __ballot(pass);
            if (mask) { kf = base + __ffsll((long long)mask) - 1; break; }
        }
        int kk = 0;
        double xk = 0, muk = 1;
        if (kf < 0) {
            if (lane == 0) s_err = 1;                        // the search ran off the row: unblended, IndexError of the reference
        } else {
            kk = kf + 1;                                     // <= N-2
            xk = s_row[kk];
            muk = g.mu[N + kk];
        }
        double* Gr = Gc + (size_t)t * D;
        for (int m = lane; m < D; m += 64) {
            double v = 0.0;
            if (m >= N) {
                const int u = m - N;
                v = s_row[u];
                if (u >= 1 && u < kk) {
                    const double w = g.mu[m] / muk;
                    v = (1 - w) * s_row[0] + w * xk;         // lane N as it stands: 0
                }
            }
            Gr[m] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && status) status[b] = s_err ? SOSRT_COL_INDEXERROR : SOSRT_COL_OK;
}

__device__ __forceinline__ double wmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_bounce_accumulate(Grid g, int B, const double* __restrict__ Ik_all,
                                                           double* __restrict__ tot_all, double* __restrict__ ratio) {
    const int L = g.L, N = g.N, D = g.D;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    const size_t n = (size_t)L * D;
    const double* Ik = Ik_all + (size_t)b * n;
    double* tot = tot_all + (size_t)b * n;
    for (size_t e = tid; e < n; e += blockDim.x) tot[e] += Ik[e];
    __syncthreads();                                         // (the two rows below were written by other lanes)
    // max |Ik|, max |total| on the upward lanes of row 0 and on the downward lanes of row L-1
    double mk[2] = {0, 0}, mt[2] = {0, 0};
    for (int m = tid; m < N; m += blockDim.x) {
        const size_t e0 = (size_t)N + m, e1 = (size_t)(L - 1) * D + m;
        mk[0] = fmax(mk[0], fabs(Ik[e0])); mt[0] = fmax(mt[0], fabs(tot[e0]));
        mk[1] = fmax(mk[1], fabs(Ik[e1])); mt[1] = fmax(mt[1], fabs(tot[e1]));
    }
    __shared__ double s_red[4][4];
    const double v[4] = {wmax(mk[0]), wmax(mt[0]), wmax(mk[1]), wmax(mt[1])};
    if ((tid & 63) == 0)
        for (int k = 0; k < 4; ++k) s_red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid == 0) {
        double r[4];
        for (int k = 0; k < 4; ++k) {
            r[k] = s_red[0][k];
            for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r[k] = s_red[w][k] > r[k] ? s_red[w][k] : r[k];
        }
        const double top = r[1] > 0 ? r[0] / r[1] : 0.0, sfc = r[3] > 0 ? r[2] / r[3] : 0.0;
        ratio[b] = sfc > top ? sfc : top;
    }
}

// ---- the ground's term at view lanes off the grid ----
// The rows of the operator modes at view cosines in place of the upward nodes: (j, v) in place of (j, i), everything else as
// k_brdf_operator_modes, so that at a view cosine equal to the node mu[N+1+i] the output has the bits of that kernel's column i.
__global__ __launch_bounds__(256) void k_brdf_view_rows_modes(Grid g, ViewMu vm, int V, BrdfParams bp, int nphi, int m0, int nm,
                                                              int sign_odd, double* __restrict__ R) {
    __shared__ double s_cos[(2 + kModesPerLaunch) * kPhiChunk];
    const int M = g.N - 1;
    const long long pairs = (long long)M * V;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < pairs;
    const int j = live ? (int)(idx / V) : 0, v = live ? (int)(idx - (long long)j * V) : 0;
    const double a = vm.s[v], b = -g.mu[j];
    double rb[kModesPerLaunch];
    azimuth_modes<kModesPerLaunch>(bp, live, a, b, nphi, m0, nm, s_cos, rb);
    if (live) {
        const double w = j == 0 ? (g.mu[1] - g.mu[0]) / 2 : j == M - 1 ? (g.mu[M - 1] - g.mu[M - 2]) / 2 : (g.mu[j + 1] - g.mu[j - 1]) / 2;
#pragma unroll
        for (int k = 0; k < kModesPerLaunch; ++k)
            if (k < nm) {
                const double x = 2.0 * w * b * rb[k];
                R[(size_t)k * pairs + idx] = (sign_odd && ((m0 + k) & 1)) ? -x : x;
            }
    }
}

__global__ __launch_bounds__(256) void k_brdf_view_beam_modes(int B, ViewMu vm, int V, BrdfParams bp, int nphi, int m0, int nm,
                                                              const double* __restrict__ mu0, double* __restrict__ r0) {
    __shared__ double s_cos[(2 + kModesPerLaunch) * kPhiChunk];
    const long long n = (long long)B * V;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    const int b = live ? (int)(idx / V) : 0, v = live ? (int)(idx - (long long)b * V) : 0;
    double rb[kModesPerLaunch];
    azimuth_modes<kModesPerLaunch>(bp, live, vm.s[v], mu0[b], nphi, m0, nm, s_cos, rb);
    if (live) {
#pragma unroll
        for (int k = 0; k < kModesPerLaunch; ++k)
            if (k < nm) r0[(size_t)k * n + idx] = rb[k];
    }
}

// rho(mu_view_v, mu0_b, phi_q) at the azimuth itself, no quadrature: one lane per (q, b, v)
__global__ __launch_bounds__(256) void k_brdf_view_beam_azimuth(int B, ViewMu vm, int V, BrdfParams bp, const double* __restrict__ mu0,
                                                                int nphi_out, const double* __restrict__ phi, double* __restrict__ out) {
    const long long n = (long long)B * V;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * nphi_out) return;
    const int q = (int)(idx / n);
    const long long e = idx - (long long)q * n;
    const int b = (int)(e / V), v = (int)(e - (long long)b * V);
    double r = 1.0;
    if (bp.kind == SOSRT_BRDF_RPV) {
        const Dir da = make_dir(vm.s[v]), db = make_dir(mu0[b]);
        const double minnaert = pow(da.c * db.c * (da.c + db.c), bp.p[1] - 1.0);
        const double sh = sin(0.5 * phi[q]);
        r = rpv(bp, da, db, minnaert, cos(phi[q]), 2.0 * sh * sh);
    }
    out[idx] = r;
}

// The ground's unscattered radiance at the view lanes: S^view of k_ground_source's chain with the rows at the view cosines
// ((j, v) in place of (j, i)), then one exp per (level, lane).  One workgroup per column, one lane per v; out [B][nlev_all][2V],
// `out` offset to the first level of lv.
__global__ __launch_bounds__(kMaxViews) void k_view_ground(Grid g, int B, int V, ViewMu vm, ColScalars sc,
                                                           const double* __restrict__ I_all, const double* __restrict__ tau_all,
                                                           const double* __restrict__ Rv, const double* __restrict__ r0v,
                                                           const double* __restrict__ scale, int nlev_all, ViewLevels lv,
                                                           int accumulate, double* __restrict__ S_out, double* __restrict__ out) {
    const int L = g.L, D = g.D, M = g.N - 1;
    const int b = blockIdx.x, v = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double s_I[];                          // [N-1] the downward surface row
    if (I_all) {
        const double* row = I_all + ((size_t)b * L + (L - 1)) * D;
        for (int j = v; j < M; j += blockDim.x) s_I[j] = row[j];
    }
    __syncthreads();
    if (v >= V) return;
    const double* tau = tau_all + (size_t)b * L;
    double acc = 0;
    if (I_all)
        for (int j = 0; j < M; ++j) acc = fma(Rv[(size_t)j * V + v], s_I[j], acc);
    if (r0v) acc += r0v[(size_t)b * V + v] * exp(-tau[L - 1] / sc.mu0[b]);
    const double S = scale ? scale[b] * acc : acc;
    if (S_out) S_out[(size_t)b * V + v] = S;
    const double tauL = tau[L - 1], mv = vm.s[v];
    for (int l = 0; l < lv.n; ++l) {
        const double dt = tauL - tau[lv.t[l]];
        const double x = S * exp(-dt / mv);
        double* o = out + ((size_t)b * nlev_all + l) * (2 * V);
        if (accumulate) {
            o[V + v] += x;
        } else {
            o[v] = 0.0;
            o[V + v] = x;
        }
    }
}

}  // namespace

void launch_brdf_view_rows_modes(hipStream_t s, const Grid& g, const ViewMu& vm, int V, BrdfParams bp, int nphi, int m_first,
                                 int m_count, int sign_odd, double* R) {
    const long long pairs = (long long)(g.N - 1) * V;
    for (int m = 0; m < m_count; m += kModesPerLaunch)
        hipLaunchKernelGGL(k_brdf_view_rows_modes, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, g, vm, V, bp, nphi,
                           m_first + m, min(kModesPerLaunch, m_count - m), sign_odd, R + (size_t)m * pairs);
}

void launch_brdf_view_beam_modes(hipStream_t s, int B, const ViewMu& vm, int V, BrdfParams bp, int nphi, int m_first, int m_count,
                                 const double* mu0, double* r0) {
    const long long n = (long long)B * V;
    for (int m = 0; m < m_count; m += kModesPerLaunch)
        hipLaunchKernelGGL(k_brdf_view_beam_modes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, B, vm, V, bp, nphi,
                           m_first + m, min(kModesPerLaunch, m_count - m), mu0, r0 + (size_t)m * n);
}

void launch_brdf_view_beam_azimuth(hipStream_t s, int B, const ViewMu& vm, int V, BrdfParams bp, const double* mu0, int nphi_out,
                                   const double* phi, double* out) {
    const long long n = (long long)B * V * nphi_out;
    hipLaunchKernelGGL(k_brdf_view_beam_azimuth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, B, vm, V, bp, mu0, nphi_out,
                       phi, out);
}

void launch_view_ground(hipStream_t s, const Grid& g, int B, int V, const ViewMu& vm, ColScalars sc, const double* I,
                        const double* tau, const double* Rv, const double* r0v, const double* scale, int nlev_all,
                        const ViewLevels& lv, int accumulate, double* S_out, double* out) {
    hipLaunchKernelGGL(k_view_ground, dim3((unsigned)B), dim3(kMaxViews), (size_t)(g.N - 1) * sizeof(double), s, g, B, V, vm, sc,
                       I, tau, Rv, r0v, scale, nlev_all, lv, accumulate, S_out, out);
}

void launch_brdf_operator(hipStream_t s, const Grid& g, BrdfParams bp, int nphi, double* R) {
    const long long pairs = (long long)(g.N - 1) * (g.N - 1);
    hipLaunchKernelGGL(k_brdf_operator, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, g, bp, nphi, R);
}

void launch_brdf_beam(hipStream_t s, const Grid& g, int B, BrdfParams bp, int nphi, const double* mu0, double* r0) {
    const long long n = (long long)B * (g.N - 1);
    hipLaunchKernelGGL(k_brdf_beam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, B, bp, nphi, mu0, r0);
}

void launch_brdf_operator_modes(hipStream_t s, const Grid& g, BrdfParams bp, int nphi, int m_first, int m_count, int sign_odd,
                                double* R) {
    const long long pairs = (long long)(g.N - 1) * (g.N - 1);
    for (int m = 0; m < m_count; m += kModesPerLaunch)
        hipLaunchKernelGGL(k_brdf_operator_modes, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, g, bp, nphi, m_first + m,
                           min(kModesPerLaunch, m_count - m), sign_odd, R + (size_t)m * pairs);
}

void launch_brdf_beam_modes(hipStream_t s, const Grid& g, int B, BrdfParams bp, int nphi, int m_first, int m_count, const double* mu0,
                            double* r0) {
    const long long n = (long long)B * (g.N - 1);
    for (int m = 0; m < m_count; m += kModesPerLaunch)
        hipLaunchKernelGGL(k_brdf_beam_modes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, B, bp, nphi, m_first + m,
                           min(kModesPerLaunch, m_count - m), mu0, r0 + (size_t)m * n);
}

void launch_ground_source(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* I, const double* tau, const double* R,
                          const double* r0, const double* scale, double* S) {
    const int threads = (g.N - 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(k_ground_source, dim3((unsigned)B), dim3(threads), (size_t)(g.N - 1) * sizeof(double), s, g, B, sc, I, tau,
                       R, r0, scale, S);
}

void launch_ground_first_order(hipStream_t s, const Grid& g, int B, const double* tau, const double* S, double* G, int* status) {
    const size_t shm = (size_t)(1 + kGfoWaves) * g.N * sizeof(double);
    hipLaunchKernelGGL(k_ground_first_order, dim3((unsigned)B), dim3(64 * kGfoWaves), shm, s, g, B, tau, S, G, status);
}

void launch_bounce_accumulate(hipStream_t s, const Grid& g, int B, const double* Ik, double* total, double* ratio) {
    hipLaunchKernelGGL(k_bounce_accumulate, dim3((unsigned)B), dim3(256), 0, s, g, B, Ik, total, ratio);
}

}  // namespace sosrt
