// BRDF ground, gfx950: the stages of the series in ground reflections that runs around the order loop.
//
//   k_brdf_pairs<NM>       every builder of the named BRDF's Fourier modes in azimuth, rho^m(a, b) = (1 / pi) int_0^pi rho(a, b, phi)
//                          cos(m phi) dphi on the trapezoid nodes: one lane per pair (a, b), the azimuth nodes in a loop, rho at a
//                          (pair, node) evaluated once and fed to the register accumulators of NM modes, the nodes' cosines and
//                          weights times cos(m phi) from LDS.  a: the grid's upward nodes mu_i (sections 20, 21) or view cosines
//                          off the grid (section 22).  b: the grid's downward nodes, stored as the operator 2 w_j |mu_j| rho^m(a,
//                          |mu_j|) with the optional (-1)^m, or the columns' mu0, stored as the beam row rho^m(a, mu0_b).  NM = 1
//                          for a launch of one mode (the azimuth mean rho_bar is mode 0), NM = 8 otherwise; a mode's bits are the
//                          same in both, and the same at a view cosine that is a node as at the node.
//                          The BRDF's kind is a template argument: the dispatch on it is made once, at the launch, and a kind's
//                          node loop holds that kind's arithmetic alone.
//   k_ground_source        S = scale (R I_surface + r0 e^{-tau*/mu0}) (ground_chain): one workgroup per column, the surface row in
//                          LDS, one lane per upward lane i, fused multiply-adds over j ascending (R is stored with the lanes i of
//                          one j contiguous).
//   k_ground_source_terms  S = sum_k weight[b][k] (R_k I_surface + r0_k e^{-tau*/mu0}) (ground_terms): the same layout, the surface
//                          row staged once for the K operators, which every column shares.
//   k_ground_first_order   the unscattered upward field of S with the mu -> 0+ blend of the order loop's upward sweep on every
//                          row: one workgroup per column, one wave per row, the row in LDS for the blend's search.
//   k_bounce_accumulate    total += Ik and the column's ratio of the two fields on the TOA-up and surface-down lanes.
//   k_brdf_view_beam_azimuth rho(mu_view_v, mu0_b, phi) at an azimuth itself, no quadrature.
//   k_view_ground          (section 22) the ground's unscattered radiance at the view lanes: ground_chain with the rows at the view
//                          cosines, one exp per (level, lane); downward lanes +0; written or accumulated.
//   k_view_ground_terms    k_view_ground with ground_terms in place of ground_chain.
//
// The kernels read the grid, the columns' mu0 (ColScalars) and their arguments, and write nothing but their outputs.
#include "brdf.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

constexpr int kPhiChunk = 256;         // azimuth nodes whose cosines a workgroup holds in LDS at a time
constexpr double kPi = 3.14159265358979323846;
constexpr int kModesPerLaunch = 8;     // Fourier modes whose accumulators a lane of the mode kernels holds in registers
constexpr int kSumChunks = 16;         // chunks of nodes (4096 nodes) a lane sums before it folds the partial sum into the total

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

// The two kernels of the Ross-Li model (sosrt.h), at directions already floored (pair_setup).  cos xi of the phase angle is
// clamped for acos; both are symmetric in (a, b) as written.
__device__ __forceinline__ double cos_xi(const Dir& a, const Dir& b, double cphi) {
    return fmin(1.0, fmax(-1.0, a.c * b.c + a.s * b.s * cphi));
}
// SOSRT_BRDF_ROSS_THICK: ((pi/2 - xi) cos xi + sin xi) / (a + b) - pi/4; inv_sum = 1 / (a + b)
__device__ __forceinline__ double ross_thick(const Dir& a, const Dir& b, double inv_sum, double cphi) {
    const double cx = cos_xi(a, b, cphi), xi = acos(cx);
    return ((0.5 * kPi - xi) * cx + sin(xi)) * inv_sum - 0.25 * kPi;
}
// SOSRT_BRDF_LI_SPARSE_R with h/b = 2, b/r = 1: O - sec + (1 + cos xi) / (2 a b), O = (t - sin t cos t) sec / pi, cos t = 2
// sqrt(D^2 + (tan a tan b sin phi)^2) / sec; sec = 1/a + 1/b.  D^2 in RPV's non-cancelling form, and sin^2 phi = hav (2 - hav)
// from the same input, a product of two non-negative numbers.
__device__ __forceinline__ double li_sparse_r(const Dir& a, const Dir& b, double sec, double cphi, double hav) {
    const double cx = cos_xi(a, b, cphi);
    const double dt = a.t - b.t, tt = a.t * b.t;
    const double D2 = fmax(0.0, dt * dt + 2.0 * tt * hav);
    const double ct = fmin(1.0, fmax(-1.0, 2.0 * sqrt(D2 + (tt * tt) * (hav * (2.0 - hav))) / sec));
    const double t = acos(ct);
    const double O = (t - sin(t) * ct) * sec / kPi;
    return O - sec + 0.5 * (1.0 + cx) / (a.c * b.c);
}

// SOSRT_BRDF_COX_MUNK (sosrt.h): the sun glint of an isotropic Gaussian slope distribution of variance
// sigma2 = p[0] over water of real index p[1].  Smith's Lambda of one direction, for the shadowing 1 / (1 + Lambda(a) + Lambda(b)):
// cot = c / s; at c = 1 (the grid's last node) cot is infinite and Lambda = 0.
__device__ __forceinline__ double smith_lambda(const Dir& d, double sigma2) {
    if (!(d.s > 0.0)) return 0.0;
    const double cot = d.c / d.s;
    return 0.5 * (sqrt(sigma2 / kPi) * exp(-(cot * cot) / sigma2) / cot - erfc(cot / sqrt(sigma2)));
}
// What the glint of a pair does not owe to the azimuth: S / (4 sigma2 a b), S = 1 / (1 + Lambda(a) + Lambda(b)) where p[2], else 1.
__device__ __forceinline__ double cox_munk_pre(const BrdfParams& bp, const Dir& a, const Dir& b) {
    const double sigma2 = bp.p[0];
    const double S = bp.p[2] != 0.0 ? 1.0 / (1.0 + smith_lambda(a, sigma2) + smith_lambda(b, sigma2)) : 1.0;
    return S / (4.0 * sigma2 * a.c * b.c);
}
// rho(a, b, phi) = F(cos chi) exp(-t2 / sigma2) (1 + t2)^2 pre.  With h2 = |horizontal part of a + b|^2, t2 = h2 / (a + b)^2 is
// tan^2 of the facet's tilt and cos^2 chi = |a + b|^2 / 4 = (h2 + (a + b)^2) / 4 of the angle of incidence on it.  hvc = 1 + cos
// phi = 2 cos^2(phi / 2): h2 = (s_a - s_b)^2 + 2 s_a s_b hvc is a sum of two non-negative terms, and so is cos^2 chi -- 1 + cos xi formed
// by subtraction (cos xi = a b - s_a s_b (1 - hav)) would cancel toward grazing specular geometry.  phi = pi is the specular direction,
// where the glint peaks and hvc -> 0: hvc comes as a square of its own (2 - hav, one minus a number next to 1, carries 2e-16
// ABSOLUTE, which at a = 0.05, b = 0.05004 one node from phi = pi is 3e-12 of hvc and of the exponent t2 / sigma2 = 1.1 there).
// F = (r_s^2 + r_p^2) / 2 is the unpolarised Fresnel reflectance.  Symmetric in (a, b) as written.  What depends on the pair alone
// (1 / (a + b)^2, 1 / sigma2, n^2) leaves the node loop; a node costs one exp, two sqrt and the two Fresnel divisions.
__device__ __forceinline__ double cox_munk(const BrdfParams& bp, const Dir& a, const Dir& b, double pre, double hvc) {
    const double n2 = bp.p[1] * bp.p[1], inv_sigma2 = 1.0 / bp.p[0];
    const double sum = a.c + b.c, sum2 = sum * sum, inv_sum2 = 1.0 / sum2;
    const double ds = a.s - b.s;
    const double h2 = ds * ds + 2.0 * (a.s * b.s) * hvc;
    const double t2 = h2 * inv_sum2;
    const double c2 = 0.25 * (h2 + sum2);
    const double c = sqrt(c2), g = sqrt(n2 - 1.0 + c2);
    const double rs = (c - g) / (c + g), rp = (n2 * c - g) / (n2 * c + g);
    const double F = 0.5 * (rs * rs + rp * rp);
    const double q = 1.0 + t2;
    return F * exp(-t2 * inv_sigma2) * (q * q) * pre;
}

// What a pair (a, b) computes once, before its azimuth nodes: the two directions (the Ross-Li kernels': floored at p[0]) and one
// number `pre` of the kind's: RPV's Minnaert factor, 1 / (a + b) of Ross-Thick, sec of Li-Sparse, Cox-Munk's S / (4 sigma2 a b).
template <int KIND>
__device__ __forceinline__ void pair_setup(const BrdfParams& bp, double ca, double cb, Dir& a, Dir& b, double& pre) {
    if constexpr (KIND == SOSRT_BRDF_ROSS_THICK || KIND == SOSRT_BRDF_LI_SPARSE_R) {
        a = make_dir(fmax(ca, bp.p[0]));
        b = make_dir(fmax(cb, bp.p[0]));
        pre = KIND == SOSRT_BRDF_ROSS_THICK ? 1.0 / (a.c + b.c) : 1.0 / a.c + 1.0 / b.c;
    } else if constexpr (KIND == SOSRT_BRDF_COX_MUNK) {
        a = make_dir(ca);
        b = make_dir(cb);
        pre = cox_munk_pre(bp, a, b);
    } else {
        a = make_dir(ca);
        b = make_dir(cb);
        pre = KIND == SOSRT_BRDF_RPV ? pow(a.c * b.c * (a.c + b.c), bp.p[1] - 1.0) : 1.0;
    }
}
// rho(a, b, phi) of kind KIND
template <int KIND>
__device__ __forceinline__ double brdf_value(const BrdfParams& bp, const Dir& a, const Dir& b, double pre, double cphi, double hav,
                                             double hvc) {
    if constexpr (KIND == SOSRT_BRDF_RPV) return rpv(bp, a, b, pre, cphi, hav);
    else if constexpr (KIND == SOSRT_BRDF_ROSS_THICK) return ross_thick(a, b, pre, cphi);
    else if constexpr (KIND == SOSRT_BRDF_LI_SPARSE_R) return li_sparse_r(a, b, pre, cphi, hav);
    else if constexpr (KIND == SOSRT_BRDF_COX_MUNK) return cox_munk(bp, a, b, pre, hvc);
    else return 1.0;
}

// ---- the BRDF's Fourier modes in azimuth (DESIGN sections 20 to 22; mode 0 is the azimuth mean) ----
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

// rho^m(a, b) = (1 / pi) int_0^pi rho cos(m phi) dphi for the modes m0 .. m0 + nm - 1 (nm <= NM) by the trapezoid rule on nphi
// nodes: rho at a (pair, node) is evaluated once and feeds the accumulators of all modes, which stay in registers (the loops
// over k have a constant trip count and are unrolled; a mode k >= nm carries weight 0 into an accumulator of its own, so a
// mode's bits do not depend on NM).  s_cos: (3 + NM) kPhiChunk doubles of the workgroup: cos phi, 1 - cos phi, 1 + cos phi (from
// the node's distance to pi: 2 sin^2 of half of it) and per mode the weight of the node times cos(m phi) for a chunk of nodes.
// With m = 0 the weight times 1 is the weight: mode 0 is the plain trapezoid sum, the azimuth mean.  Every thread of the
// workgroup calls this (the chunk loop holds barriers); `live` says whether the lane has a pair.
// The sum runs in blocks of kSumChunks chunks, each block into a partial sum of its own that is then added to the total: the
// terms of mode 0 have one sign and vary slowly from node to node, so the roundings of one running sum do not average out but add
// up, to 1.2e-12 of the sum at 65537 nodes (measured; 9e-13 for a pair with b = 1, whose terms are all equal); over 4096 terms
// they stay below 3e-14.  Up to 4096 nodes there is one block and the total IS its partial sum: the bits of the single running sum.
template <int NM, int KIND>
__device__ __forceinline__ void azimuth_modes(const BrdfParams& bp, bool live, double ca, double cb, int nphi, int m0, int nm,
                                              double* s_cos, double (&acc)[NM]) {
    double* s_hav = s_cos + kPhiChunk;
    double* s_hvc = s_cos + 2 * kPhiChunk;
    double* s_wc = s_cos + 3 * kPhiChunk;                    // [NM][kPhiChunk]
    Dir a, b;
    double pre;
    pair_setup<KIND>(bp, ca, cb, a, b, pre);
    const double h = 1.0 / (nphi - 1);
    double part[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = part[k] = 0;
    for (int q0 = 0; q0 < nphi; q0 += kPhiChunk) {
        const int nq = min(kPhiChunk, nphi - q0);
        __syncthreads();
        for (int q = threadIdx.x; q < nq; q += blockDim.x) {
            const double phi = kPi * (q0 + q) * h, sh = sin(0.5 * phi);
            s_cos[q] = q0 + q == nphi - 1 ? -1.0 : cos(phi);
            s_hav[q] = q0 + q == nphi - 1 ? 2.0 : 2.0 * sh * sh;
            const double ch = sin(0.5 * (kPi * (nphi - 1 - (q0 + q)) * h));
            s_hvc[q] = 2.0 * ch * ch;
            const double w = (q0 + q == 0 || q0 + q == nphi - 1) ? 0.5 * h : h;
#pragma unroll
            for (int k = 0; k < NM; ++k) s_wc[k * kPhiChunk + q] = k < nm ? w * mode_cos(m0 + k, q0 + q, nphi, h) : 0.0;
        }
        __syncthreads();
        if (live) {
            for (int q = 0; q < nq; ++q) {
                const double v = brdf_value<KIND>(bp, a, b, pre, s_cos[q], s_hav[q], s_hvc[q]);
#pragma unroll
                for (int k = 0; k < NM; ++k) part[k] = fma(s_wc[k * kPhiChunk + q], v, part[k]);
            }
        }
        const int chunk = q0 / kPhiChunk;
        if (chunk % kSumChunks == kSumChunks - 1 || q0 + kPhiChunk >= nphi) {      // (the same for every lane)
#pragma unroll
            for (int k = 0; k < NM; ++k) {
                acc[k] = chunk < kSumChunks ? part[k] : acc[k] + part[k];
                part[k] = 0;
            }
        }
    }
}

// trapezoid weight of node j among mu[0 .. N-2], the grid's downward nodes
__device__ __forceinline__ double flux_weight(const Grid& g, int j) {
    const int M = g.N - 1;
    return j == 0 ? (g.mu[1] - g.mu[0]) / 2 : j == M - 1 ? (g.mu[M - 1] - g.mu[M - 2]) / 2 : (g.mu[j + 1] - g.mu[j - 1]) / 2;
}

// The modes m0 .. m0 + nm - 1 (nm <= NM) of every pair (first, second) of directions, out [nm][nSecond][nFirst].  First: the
// view cosines vm.s[0 .. V-1], or with V = 0 the grid's upward nodes mu[N+1 ..].  Second: the columns' mu0[0 .. B-1], stored as
// rho^m itself, or with mu0 = nullptr the grid's downward nodes |mu_j|, stored as 2 w_j |mu_j| rho^m, mode m as (-1)^m of it
// where sign_odd.  A lane past the pairs stays for the barriers of the node loop.  KIND: bp.kind, the launch's choice.
template <int NM, int KIND>
__global__ __launch_bounds__(256) void k_brdf_pairs(Grid g, ViewMu vm, int V, int B, BrdfParams bp, int nphi, int m0, int nm,
                                                    int sign_odd, const double* __restrict__ mu0, double* __restrict__ out) {
    __shared__ double s_cos[(3 + NM) * kPhiChunk];
    const int N = g.N, M = N - 1;
    const int nFirst = V ? V : M;
    const long long n = (long long)(mu0 ? B : M) * nFirst;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    const int second = live ? (int)(idx / nFirst) : 0, first = live ? (int)(idx - (long long)second * nFirst) : 0;
    const double a = V ? vm.s[first] : g.mu[N + 1 + first], b = mu0 ? mu0[second] : -g.mu[second];
    double rb[NM];
    azimuth_modes<NM, KIND>(bp, live, a, b, nphi, m0, nm, s_cos, rb);
    if (live) {
        const double w = mu0 ? 0.0 : flux_weight(g, second);
#pragma unroll
        for (int k = 0; k < NM; ++k)
            if (k < nm) {
                double x = rb[k];
                if (!mu0) {
                    x = 2.0 * w * b * x;
                    if (sign_odd && ((m0 + k) & 1)) x = -x;
                }
                out[(size_t)k * n + idx] = x;
            }
    }
}

// S of one lane = scale (sum_j R[j n + lane] s_I[j] + r0 exp(-tauL / mu0)): the sum over the M entries of the surface row by
// fused multiply-adds with j ascending, then the beam term (its exp evaluated only where r0, the lane's beam row, is given),
// the scale last.  R (no field, no sum), r0 and scale (the column's) are nullable.
__device__ __forceinline__ double ground_chain(const double* __restrict__ R, int n, int lane, const double* s_I, int M,
                                               const double* __restrict__ r0, double tauL, double mu0,
                                               const double* __restrict__ scale) {
    double acc = 0;
    if (R)
        for (int j = 0; j < M; ++j) acc = fma(R[(size_t)j * n + lane], s_I[j], acc);
    if (r0) acc += *r0 * exp(-tauL / mu0);
    return scale ? *scale * acc : acc;
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
    S_all[(size_t)b * M + i] = ground_chain(R, M, i, s_I, M, r0 ? r0 + (size_t)b * M + i : nullptr, tau_all[(size_t)b * L + (L - 1)],
                                            sc.mu0[b], scale ? scale + b : nullptr);
}

// S of one lane over K operator terms = sum_k weight[k] c_k, c_k the ground_chain of term k without a scale (its operator R + k
// strideR, its beam row r0[k strideR0]): acc = +0, then acc = fma(weight[k], c_k, acc) with k ascending.  With K = 1 that is
// round(weight c), the bits of ground_chain with scale = weight; a term of weight 0 leaves acc as it is; all weights 0 give +0.
__device__ __forceinline__ double ground_terms(int K, const double* __restrict__ R, size_t strideR, int n, int lane, const double* s_I,
                                               int M, const double* __restrict__ r0, size_t strideR0, double tauL, double mu0,
                                               const double* __restrict__ weight) {
    double acc = 0;
    for (int k = 0; k < K; ++k) {
        const double c = ground_chain(R ? R + k * strideR : nullptr, n, lane, s_I, M, r0 ? r0 + k * strideR0 : nullptr, tauL, mu0,
                                      nullptr);
        acc = fma(weight[k], c, acc);
    }
    return acc;
}

// k_ground_source over K terms: R [K][N-1][N-1], r0 [K][B][N-1] (nullable), weight [B][K].  The surface row is staged once; the
// K operators are the same for every column (L2 serves them after the first), each read with the lanes i of one j contiguous.
__global__ __launch_bounds__(1024) void k_ground_source_terms(Grid g, int B, int K, ColScalars sc, const double* __restrict__ I_all,
                                                              const double* __restrict__ tau_all, const double* __restrict__ R,
                                                              const double* __restrict__ r0, const double* __restrict__ weight,
                                                              double* __restrict__ S_all) {
    const int L = g.L, N = g.N, D = g.D, M = N - 1;
    const int b = blockIdx.x, i = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double s_I[];                          // [N-1] the downward surface row
    const double* row = I_all + ((size_t)b * L + (L - 1)) * D;
    for (int j = i; j < M; j += blockDim.x) s_I[j] = row[j];
    __syncthreads();
    if (i >= M) return;
    S_all[(size_t)b * M + i] = ground_terms(K, R, (size_t)M * M, M, i, s_I, M, r0 ? r0 + (size_t)b * M + i : nullptr, (size_t)B * M,
                                            tau_all[(size_t)b * L + (L - 1)], sc.mu0[b], weight + (size_t)b * K);
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
// rho(ca, cb, phi) of a Ross-Li kernel or of Cox-Munk at an azimuth itself, with the inputs of the node loop: cos phi, 2 sin^2(phi / 2)
// and 2 cos^2(phi / 2)
template <int KIND>
__device__ __forceinline__ double value_at(const BrdfParams& bp, double ca, double cb, double phi) {
    Dir a, b;
    double pre;
    pair_setup<KIND>(bp, ca, cb, a, b, pre);
    const double sh = sin(0.5 * phi), ch = cos(0.5 * phi);
    return brdf_value<KIND>(bp, a, b, pre, cos(phi), 2.0 * sh * sh, 2.0 * ch * ch);
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
    } else if (bp.kind == SOSRT_BRDF_ROSS_THICK) {
        r = value_at<SOSRT_BRDF_ROSS_THICK>(bp, vm.s[v], mu0[b], phi[q]);
    } else if (bp.kind == SOSRT_BRDF_LI_SPARSE_R) {
        r = value_at<SOSRT_BRDF_LI_SPARSE_R>(bp, vm.s[v], mu0[b], phi[q]);
    } else if (bp.kind == SOSRT_BRDF_COX_MUNK) {
        r = value_at<SOSRT_BRDF_COX_MUNK>(bp, vm.s[v], mu0[b], phi[q]);
    }
    out[idx] = r;
}

// k_view_ground over K terms (ground_terms): Rv [K][N-1][V], r0v [K][B][V], weight [B][K]
__global__ __launch_bounds__(kMaxViews) void k_view_ground_terms(Grid g, int B, int K, int V, ViewMu vm, ColScalars sc,
                                                                 const double* __restrict__ I_all, const double* __restrict__ tau_all,
                                                                 const double* __restrict__ Rv, const double* __restrict__ r0v,
                                                                 const double* __restrict__ weight, int nlev_all, ViewLevels lv,
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
    const double S = ground_terms(K, I_all ? Rv : nullptr, (size_t)M * V, V, v, s_I, M, r0v ? r0v + (size_t)b * V + v : nullptr,
                                  (size_t)B * V, tau[L - 1], sc.mu0[b], weight + (size_t)b * K);
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

// The ground's unscattered radiance at the view lanes: S^view of k_ground_source's ground_chain with the rows at the view cosines
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
    const double S = ground_chain(I_all ? Rv : nullptr, V, v, s_I, M, r0v ? r0v + (size_t)b * V + v : nullptr, tau[L - 1], sc.mu0[b],
                                  scale ? scale + b : nullptr);
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

void launch_brdf_pairs(hipStream_t s, const Grid& g, const ViewMu& vm, int V, int B, BrdfParams bp, int nphi, int m_first,
                       int m_count, int sign_odd, const double* mu0, double* out) {
    const long long n = (long long)(mu0 ? B : g.N - 1) * (V ? V : g.N - 1);
    const dim3 blocks((unsigned)((n + 255) / 256));
    // [kind][one mode or up to kModesPerLaunch]; api_brdf.hip lets no other kind through
    static constexpr decltype(&k_brdf_pairs<1, 0>) kernels[5][2] = {
        {k_brdf_pairs<1, SOSRT_BRDF_LAMBERTIAN>, k_brdf_pairs<kModesPerLaunch, SOSRT_BRDF_LAMBERTIAN>},
        {k_brdf_pairs<1, SOSRT_BRDF_RPV>, k_brdf_pairs<kModesPerLaunch, SOSRT_BRDF_RPV>},
        {k_brdf_pairs<1, SOSRT_BRDF_ROSS_THICK>, k_brdf_pairs<kModesPerLaunch, SOSRT_BRDF_ROSS_THICK>},
        {k_brdf_pairs<1, SOSRT_BRDF_LI_SPARSE_R>, k_brdf_pairs<kModesPerLaunch, SOSRT_BRDF_LI_SPARSE_R>},
        {k_brdf_pairs<1, SOSRT_BRDF_COX_MUNK>, k_brdf_pairs<kModesPerLaunch, SOSRT_BRDF_COX_MUNK>},
    };
    for (int m = 0; m < m_count; m += kModesPerLaunch) {
        const int nm = min(kModesPerLaunch, m_count - m);
        const auto kernel = kernels[bp.kind][nm == 1 ? 0 : 1];
        hipLaunchKernelGGL(kernel, blocks, dim3(256), 0, s, g, vm, V, B, bp, nphi, m_first + m, nm, sign_odd, mu0,
                           out + (size_t)m * n);
    }
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

void launch_ground_source(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* I, const double* tau, const double* R,
                          const double* r0, const double* scale, double* S) {
    const int threads = (g.N - 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(k_ground_source, dim3((unsigned)B), dim3(threads), (size_t)(g.N - 1) * sizeof(double), s, g, B, sc, I, tau,
                       R, r0, scale, S);
}

void launch_ground_source_terms(hipStream_t s, const Grid& g, int B, int K, ColScalars sc, const double* I, const double* tau,
                                const double* R, const double* r0, const double* weight, double* S) {
    const int threads = (g.N - 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(k_ground_source_terms, dim3((unsigned)B), dim3(threads), (size_t)(g.N - 1) * sizeof(double), s, g, B, K, sc, I,
                       tau, R, r0, weight, S);
}

void launch_view_ground_terms(hipStream_t s, const Grid& g, int B, int K, int V, const ViewMu& vm, ColScalars sc, const double* I,
                              const double* tau, const double* Rv, const double* r0v, const double* weight, int nlev_all,
                              const ViewLevels& lv, int accumulate, double* S_out, double* out) {
    hipLaunchKernelGGL(k_view_ground_terms, dim3((unsigned)B), dim3(kMaxViews), (size_t)(g.N - 1) * sizeof(double), s, g, B, K, V, vm,
                       sc, I, tau, Rv, r0v, weight, nlev_all, lv, accumulate, S_out, out);
}

void launch_ground_first_order(hipStream_t s, const Grid& g, int B, const double* tau, const double* S, double* G, int* status) {
    const size_t shm = (size_t)(1 + kGfoWaves) * g.N * sizeof(double);
    hipLaunchKernelGGL(k_ground_first_order, dim3((unsigned)B), dim3(64 * kGfoWaves), shm, s, g, B, tau, S, G, status);
}

void launch_bounce_accumulate(hipStream_t s, const Grid& g, int B, const double* Ik, double* total, double* ratio) {
    hipLaunchKernelGGL(k_bounce_accumulate, dim3((unsigned)B), dim3(256), 0, s, g, B, Ik, total, ratio);
}

}  // namespace sosrt
