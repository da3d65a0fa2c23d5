// View radiance: the radiance of a solved field at view cosines that are not nodes of the direction grid,
// by integrating the field's source function along the line of sight at the view cosine itself.  gfx950.
//
//   k_view_fold       W[k][c] = w_k rows[c][2N-1-k]: the rows folded as the contraction's matrices are (I1_In:73, spec:321);
//                     the atmosphere's rows in the columns c < CP/2, the aerosol's from CP/2 on, zero padding.
//   k_view_source     S[b][t][j] = ca(b,t) sum_k W_atm[k][j] Isrc[b][t][k] + cr(b,t) sum_k W_aer[k][j] Isrc[b][t][k]: a
//                     [B L x 2N] . [2N x 4V] fp64 product on v_fma_f64.  A workgroup owns 64 rows of the field and ALL output
//                     columns, so a row of Isrc is read once whatever V is; both operands are streamed by 16-deep k-chunks through
//                     LDS (the folded rows no longer fit LDS at N = 501), the next chunk's loads in flight while the current one
//                     is multiplied.
//   k_view_transport  one lane per (column, |mu|): the downward sweep of -mu, the surface value, the upward sweep of +mu;
//                     one exponential per (row, lane) per sweep; GRID (the grid's trapezoid arithmetic, without the mu -> 0
//                     treatments) and LINEAR (exact attenuation of a piecewise-linear source) are one loop with two weight
//                     formulas.  Every lane reads the zone table of its own column.
//   k_view_first_order
//                     the closed-form first order (spec:104-292, I1_In:13-58) at the lanes s_j and the requested levels only:
//                     the chain through the zone-boundary rows, O(zones) exponentials per level.
// The rows of the phase matrix, of P0 and of their Fourier modes at the view cosines come from the builders of phase.hip, with
// the stored matrix's own normalisers: at a node the row is the matrix's row.
#include "kernels.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

// ---------------------------------------------------------------------------------------------
// source at the view lanes
// ---------------------------------------------------------------------------------------------
constexpr int VS_BM = 64;          // rows of the field per workgroup
constexpr int VS_KC = 16;          // k-chunk
constexpr int VS_LDA = VS_BM + 2;  // row stride of the transposed chunk of the field (even: a lane's four rows are two 16-byte reads)

// W [Dp][CP]: column c < CP/2 is lane j = c of the atmosphere's rows, column CP/2 + j lane j of the aerosol's
__global__ __launch_bounds__(256) void k_view_fold(int D, int Dp, int V2, int CP, const double* __restrict__ w,
                                                   const double* __restrict__ rows_atm, const double* __restrict__ rows_aer,
                                                   double* __restrict__ W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Dp * CP) return;
    const int k = i / CP, c = i - k * CP, half = CP / 2;
    const int j = c < half ? c : c - half;
    const double* rows = c < half ? rows_atm : rows_aer;
    W[i] = (k < D && j < V2 && rows) ? w[k] * rows[(size_t)j * D + (D - 1 - k)] : 0.0;
}

// Thread (tx, ty) of the 16 x 16 workgroup owns rows 4 ty .. 4 ty + 3 of the tile and the columns tx + 16 i, i < CPT: a wave
// reads 16 consecutive doubles of a chunk row of W (no bank conflict, broadcast over ty) and four addresses of the field's
// chunk (broadcast over tx).  CPT = 4, 8, 16 serves V <= 16, 32, 64.
template <int CPT>
__global__ __launch_bounds__(256) void k_view_source(int nrows, int D, int Dp, int V2, const double* __restrict__ A,
                                                     const double* __restrict__ W, const double* __restrict__ ca,
                                                     const double* __restrict__ cr, double* __restrict__ S) {
    constexpr int CP = 16 * CPT, HALF = CPT / 2;
    __shared__ __attribute__((aligned(16))) double sA[VS_KC * VS_LDA];
    __shared__ double sB[VS_KC * CP];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * VS_BM;
    // loader roles: the field's chunk as 64 rows x 16 k (four consecutive k of one row per thread), W's chunk linearly
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const bool lrow_ok = row0 + lr < nrows;
    const double* arow = A + (size_t)(lrow_ok ? row0 + lr : 0) * D;
    double pa[4], pb[CPT];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + lk + u;
            pa[u] = (lrow_ok && k < D) ? arow[k] : 0.0;
        }
        const double* wsrc = W + (size_t)k0 * CP;
#pragma unroll
        for (int u = 0; u < CPT; ++u) pb[u] = wsrc[tid + 256 * u];
    };
    double acc[4][CPT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < CPT; ++c) acc[i][c] = 0;
    fetch(0);
    for (int k0 = 0; k0 < Dp; k0 += VS_KC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) sA[(lk + u) * VS_LDA + lr] = pa[u];
#pragma unroll
        for (int u = 0; u < CPT; ++u) sB[tid + 256 * u] = pb[u];
        __syncthreads();
        if (k0 + VS_KC < Dp) fetch(k0 + VS_KC);
#pragma unroll
        for (int kk = 0; kk < VS_KC; ++kk) {
            const double2 a01 = *reinterpret_cast<const double2*>(&sA[kk * VS_LDA + ty * 4]);
            const double2 a23 = *reinterpret_cast<const double2*>(&sA[kk * VS_LDA + ty * 4 + 2]);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y};
            double bv[CPT];
#pragma unroll
            for (int c = 0; c < CPT; ++c) bv[c] = sB[kk * CP + tx + 16 * c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < CPT; ++c) acc[i][c] = fma(a[i], bv[c], acc[i][c]);
        }
        __syncthreads();
    }
    // lane j = tx + 16 c of the atmosphere's product is column c, of the aerosol's column c + HALF, of the same thread
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + ty * 4 + i;
        if (row >= nrows) continue;
        const double a = ca[row], r = cr[row];
#pragma unroll
        for (int c = 0; c < HALF; ++c) {
            const int j = tx + 16 * c;
            if (j < V2) S[(size_t)row * V2 + j] = a * acc[i][c] + r * acc[i][c + HALF];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// transport at the view lanes
// ---------------------------------------------------------------------------------------------
// LINEAR: U_t = E U_{t+1} + w0 S_t + w1 S_{t+1}, E = e^{-x}, x = dtau / mu, a = (1 - E) / x, w0 = 1 - a, w1 = a - E.  Both
// differences cancel at small x; below kLinSeries the alternating series
//     w0 = sum_{n>=1} (-1)^{n+1} x^n / (n+1)!,   w1 = sum_{n>=1} (-1)^{n+1} n x^n / (n+1)!
// is summed to 12 terms (the first term dropped is 0.25^13 / 14! = 2e-19; at x = 0.25 the direct form has lost three bits).
constexpr double kLinSeries = 0.25;
__device__ __forceinline__ void linear_weights(double x, double E, double& w0, double& w1) {
    if (x < kLinSeries) {
        constexpr double f[13] = {1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                                  1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0};
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int n = 12; n >= 1; --n) {                      // Horner, innermost term first: c_n - x (c_{n+1} - ...)
            s0 = f[n - 1] - x * s0;
            s1 = n * f[n - 1] - x * s1;
        }
        w0 = x * s0;
        w1 = x * s1;
    } else {
        const double a = (1 - E) / x;
        w0 = 1 - a;
        w1 = a - E;
    }
}

struct ViewSweepArgs {
    int B, V, L, quad;
    int nlev_all;              // levels of the whole call: row stride of the outputs
    const double* tau;         // [B][L]
    const double* S;           // [B][L][2V]
    const ColDesc* desc;       // [B]
    double* out;               // [B][nlev_all][2V], offset to the first level of this launch
};

constexpr int VT_U = 4;        // rows whose loads are issued together

__global__ __launch_bounds__(64) void k_view_transport(ViewSweepArgs a, ViewMu vm, ViewLevels lv) {
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= a.B * a.V) return;
    const int V = a.V, V2 = 2 * V, L = a.L;
    const int b = gid / V, v = gid - b * V;
    const double mu = vm.s[V + v], rmu = 1.0 / mu;
    const double* __restrict__ tau = a.tau + (size_t)b * L;
    const double* __restrict__ S = a.S + (size_t)b * L * V2;
    const ColDesc* __restrict__ d = a.desc + b;
    double* __restrict__ out = a.out + (size_t)b * a.nlev_all * V2;
    const bool linear = a.quad == SOSRT_VIEW_QUAD_LINEAR;
    auto emit = [&](int t, int j, double val) {
        for (int i = 0; i < lv.n; ++i)
            if (lv.t[i] == t) out[(size_t)i * V2 + j] = val;
    };
    // weights of the current row and of the row the sweep comes from
    auto weights = [&](double x, double E, double& wc, double& wp) {
        if (linear) linear_weights(x, E, wc, wp);
        else { wc = 0.5 * x; wp = wc * E; }                  // (dtau / 2) (S_cur + S_prev E) / mu
    };
    // ---- downward, lane -mu ----
    double Dv = 0, tp = tau[0], sp = S[v];
    emit(0, v, 0.0);
    for (int t0 = 1; t0 < L; t0 += VT_U) {
        double tn[VT_U], sn[VT_U];
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = min(t0 + u, L - 1);
            tn[u] = tau[t];
            sn[u] = S[(size_t)t * V2 + v];
        }
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = t0 + u;
            if (t < L) {
                const double x = (tn[u] - tp) * rmu, E = exp(-x);
                double wc, wp;
                weights(x, E, wc, wp);
                Dv = E * Dv + (wc * sn[u] + wp * sp);
                emit(t, v, Dv);
                tp = tn[u]; sp = sn[u];
            }
        }
    }
    // ---- surface (spec:397/399): the mirror lane's downward value ----
    double Uv = d->surface == SOSRT_SURFACE_SPECULAR ? d->rho * Dv : 0.0;
    emit(L - 1, V + v, Uv);
    // ---- upward, lane +mu; GRID: the last row of every zone but the bottom one is attenuated and not integrated ----
    int z = d->nz - 1;
    int zb = d->r0[z] - 1;                                   // last row of the zone above the current one (-1: none)
    sp = S[(size_t)(L - 1) * V2 + V + v];
    for (int t0 = L - 2; t0 >= 0; t0 -= VT_U) {
        double tn[VT_U], sn[VT_U];
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = max(t0 - u, 0);
            tn[u] = tau[t];
            sn[u] = S[(size_t)t * V2 + V + v];
        }
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = t0 - u;
            if (t >= 0) {
                const double x = (tp - tn[u]) * rmu, E = exp(-x);
                double wc, wp;
                weights(x, E, wc, wp);
                if (t == zb) {
                    --z;
                    zb = d->r0[z] - 1;
                    if (!linear) { wc = 0; wp = 0; }
                }
                Uv = E * Uv + (wc * sn[u] + wp * sp);
                emit(t, V + v, Uv);
                tp = tn[u]; sp = sn[u];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// first order at the view lanes
// ---------------------------------------------------------------------------------------------
struct FirstLane {
    const ColDesc* d;
    const double* tau;
    int L;
    double mu0, T, F0, R;
    // scattering coefficient of zone z for a lane with first-order phase values (pa, pr): spec:149
    __device__ __forceinline__ double q(int z, double pa, double pr) const {
        const double c4pi = 1.0 / (4 * SOSRT_PI);
        return d->mix[z] ? (d->wa * pa * d->fa[z] + d->wr[z] * pr * d->fr[z]) * c4pi : d->wa * pa * c4pi;
    }
    // I1 at row t of the downward lane -mu (spec:113-201): (pa, pr) of the lane itself, (pam, prm) of its mirror
    __device__ double down(int t, double mu, double pa, double pr, double pam, double prm) const {
        const double md = -mu;
        const bool near = fabs(md + mu0) < 0.0001;           // spec:111
        const double gd = mu0 / (mu0 + md), gs = mu0 / (mu0 - md);
        double Ib = 0;
        for (int z = 0; z < d->nz; ++z) {
            const int r1 = d->r1[z];
            const bool last = t <= r1;
            const double tt = tau[last ? t : r1];
            const double t_bd = z ? tau[d->r0[z] - 1] : 0.0, t_bs = z ? tau[d->r0[z]] : 0.0;
            const double e0 = exp(-tt / mu0), eT = exp(-(T - tt) / mu0);
            const double x = exp((tt - t_bd) / md), xs = exp((tt - t_bs) / md);
            const double qz = q(z, pa, pr), qm = q(z, pam, prm);
            const double before = z ? Ib * x : 0.0;
            const double direct = near ? qz * F0 * e0 * (tt - t_bd) / mu0 : gd * qz * F0 * (e0 - exp(-t_bd / mu0) * x);
            const double surf = gs * qm * R * (eT - exp(-(T - t_bs) / mu0) * xs);
            Ib = before + direct + surf;
            if (last) break;
        }
        return Ib;
    }
    // I1 at row t of the upward lane +mu (spec:204-292); Bsurf: the reflected downward first order at the surface (spec:211)
    __device__ double up(int t, double mu, double pa, double pr, double pam, double prm, double Bsurf) const {
        const bool near = fabs(mu - mu0) < 0.0001;           // spec:204
        const double gd = mu0 / (mu0 + mu), gs = mu0 / (mu0 - mu);
        double Bv = Bsurf;
        for (int z = d->nz - 1; z >= 0; --z) {
            const bool bottom = z == d->nz - 1;
            const int r0 = d->r0[z], r1 = d->r1[z];
            const bool last = t >= r0;
            const double tt = tau[last ? t : r0];
            const double t_bu = bottom ? d->tau_bottom : tau[r1 + 1];
            const double t_bb = bottom ? tau[L - 1] : t_bu;
            const double t_su = bottom ? T : tau[r1];
            const double e0 = exp(-tt / mu0), eT = exp(-(T - tt) / mu0);
            const double yb = exp(-(t_bb - tt) / mu), yu = exp(-(t_bu - tt) / mu), ys = exp(-(t_su - tt) / mu);
            const double qz = q(z, pa, pr), qm = q(z, pam, prm);
            const double before = Bv * yb;
            const double direct = gd * qz * F0 * (e0 - exp(-t_bu / mu0) * yu);
            const double surf = near ? qm * R * eT * (t_su - tt) / mu0 : gs * qm * R * (eT - exp(-(T - t_su) / mu0) * ys);
            Bv = before + direct + surf;
            if (last) break;
        }
        return Bv;
    }
};

struct ViewFirstArgs {
    int B, V, L, nlev_all;
    const double* tau;
    const double* p0a;         // [B][2V]
    const double* p0r;         // [B][2V] (null: single slab, never read through a mix zone)
    const ColDesc* desc;
    double* out;               // [B][nlev_all][2V], offset to the first level of this launch
};

// one lane per (column, signed lane j)
__global__ __launch_bounds__(64) void k_view_first_order(ViewFirstArgs a, ViewMu vm, ViewLevels lv) {
    const int gid = blockIdx.x * 64 + threadIdx.x;
    const int V = a.V, V2 = 2 * V;
    if (gid >= a.B * V2) return;
    const int b = gid / V2, j = gid - b * V2;
    const bool upward = j >= V;
    const int mir = upward ? j - V : j + V;
    FirstLane f;
    f.d = a.desc + b;
    f.tau = a.tau + (size_t)b * a.L;
    f.L = a.L;
    f.mu0 = f.d->mu0;
    f.T = f.d->T;
    f.F0 = SOSRT_PI / f.mu0;                                 // spec:105
    f.R = f.F0 * f.d->rho * exp(-f.T / f.mu0);               // reflected beam at the surface
    const double mu = vm.s[upward ? j : mir];                // |s_j|
    const double* p0a = a.p0a + (size_t)b * V2;
    const double* p0r = a.p0r ? a.p0r + (size_t)b * V2 : p0a;
    const double pa = p0a[j], pam = p0a[mir], pr = p0r[j], prm = p0r[mir];
    double* out = a.out + (size_t)b * a.nlev_all * V2 + j;
    double Bsurf = 0;
    if (upward) Bsurf = f.d->rho * f.down(a.L - 1, mu, pam, prm, pa, pr);
    for (int i = 0; i < lv.n; ++i) {
        const int t = lv.t[i];
        out[(size_t)i * V2] = upward ? f.up(t, mu, pa, pr, pam, prm, Bsurf) : f.down(t, mu, pa, pr, pam, prm);
    }
}

}  // namespace

int view_source_cols(int V) { return V <= 16 ? 64 : V <= 32 ? 128 : 256; }
int view_source_kpad(int D) { return (D + VS_KC - 1) / VS_KC * VS_KC; }

void launch_view_source(hipStream_t s, int nrows, int D, int V, const double* w, const double* rows_atm, const double* rows_aer,
                        const double* Isrc, const double* ca, const double* cr, double* Wfold, double* S) {
    const int CP = view_source_cols(V), Dp = view_source_kpad(D), V2 = 2 * V;
    hipLaunchKernelGGL(k_view_fold, dim3((Dp * CP + 255) / 256), dim3(256), 0, s, D, Dp, V2, CP, w, rows_atm, rows_aer, Wfold);
    const dim3 grid((nrows + VS_BM - 1) / VS_BM);
    if (CP == 64) hipLaunchKernelGGL(k_view_source<4>, grid, dim3(256), 0, s, nrows, D, Dp, V2, Isrc, Wfold, ca, cr, S);
    else if (CP == 128) hipLaunchKernelGGL(k_view_source<8>, grid, dim3(256), 0, s, nrows, D, Dp, V2, Isrc, Wfold, ca, cr, S);
    else hipLaunchKernelGGL(k_view_source<16>, grid, dim3(256), 0, s, nrows, D, Dp, V2, Isrc, Wfold, ca, cr, S);
}

void launch_view_transport(hipStream_t s, int B, int V, int L, int quad, int nlev_all, const double* tau, const double* S,
                           const ColDesc* desc, const ViewMu& mu, const ViewLevels& lv, double* out) {
    ViewSweepArgs a{B, V, L, quad, nlev_all, tau, S, desc, out};
    hipLaunchKernelGGL(k_view_transport, dim3((B * V + 63) / 64), dim3(64), 0, s, a, mu, lv);
}

void launch_view_first_order(hipStream_t s, int B, int V, int L, int nlev_all, const double* tau, const double* p0a,
                             const double* p0r, const ColDesc* desc, const ViewMu& mu, const ViewLevels& lv, double* out) {
    ViewFirstArgs a{B, V, L, nlev_all, tau, p0a, p0r, desc, out};
    hipLaunchKernelGGL(k_view_first_order, dim3((B * 2 * V + 63) / 64), dim3(64), 0, s, a, mu, lv);
}

}  // namespace sosrt
