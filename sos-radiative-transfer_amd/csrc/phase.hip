// The builders of the phase functions on the device (DESIGN sections 11, 15 and 16), gfx950: every table of (exit direction,
// second direction, azimuth mode) the solve and the view stage take comes from the kernels of this file, and every one of them is
// normalised by the one rule below.
//
//   k_phase_pairs<SECOND, EXITS, K>
//                     one workgroup per second direction -- the grid's mu[n], a column n of the stored matrix (phase:107-131, 169-193,
//                     266-290), or a batch column's mu0[b], its first-order P0 (phase:86-103, 148-165, 245-262) -- the threads over
//                     the exit directions: the 2N grid nodes, or view cosines s_j off the grid.  K = 0 is the azimuth mean by the
//                     reference's 25-node ring; K = 9, 17, 33, kMaxModes + 1 bounds the accumulators of the Fourier modes m >= 1
//                     (the m = 0 ring that normalises plus m_count modes): one evaluation of p per (pair, phi node) feeds them all.
//   k_phase_p0_azimuth
//                     p(c(s_j, mu0_b, phi_i)) / Z0_b: the first-order phase value at a view lane and an azimuth, the sum the modes
//                     of P0 converge to, with the normaliser of the plain P0 rows.
//   k_phase_p0_normaliser
//                     Z0_b itself and nothing else: what rescales point values of one function by the normaliser of another (the
//                     TMS first order of DESIGN section 28).
//
// The normalisation is a policy with one owner: normaliser() is the reference's trapz over the 2N grid exits of the m = 0 ring
// of a second direction, Constants<SECOND> holds the factor in front of the ring and the rescaling by the normaliser.  A row at
// view cosines takes the normaliser first and then scales its values; a grid builder stores the raw values on the way, reduces,
// and rescales what each thread stored.  So at a node the row at a view cosine is the stored matrix's row; for the modes the one
// remaining difference is that the row's normaliser comes from ring_modes<1> and the matrix's from accumulator 0 of
// ring_modes<K>, the same expression in two instantiations, whose equal bits tests/test_gpu_view_azimuth.py pins at all four K.
#include "phasefn.hpp"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup; every thread gets the result
__device__ double bsum(double x, double* s_red) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    const double v = wsum(x);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    double r = 0;
    for (int i = 0; i < nw; ++i) r += s_red[i];
    return r;
}

enum Second { COLUMN, MU0 };       // the second direction: the grid's mu[n], or a batch column's mu0[b]
enum Exits { NODES, LANES };       // the exit directions: the grid's 2N nodes, or the view cosines

// The two pairs of constants of the reference: the factor in front of a ring and the rescaling by the normaliser.  The pairs are
// not one expression: each keeps its order of operations.
template <Second S>
struct Constants;
template <>
struct Constants<COLUMN> {         // phase:128, 131; isotropic: 2 everywhere (phase:74)
    static constexpr double iso = 2.0;
    static __device__ __forceinline__ double raw(double ring) { return ring / (2 * SOSRT_PI); }
    static __device__ __forceinline__ double scaled(double v, double norm) { return 4 * v / norm; }
};
template <>
struct Constants<MU0> {            // phase:101, 103; isotropic: ones (phase:68-76)
    static constexpr double iso = 1.0;
    static __device__ __forceinline__ double raw(double ring) { return ring / (4 * SOSRT_PI); }
    static __device__ __forceinline__ double scaled(double v, double norm) { return v / norm * 2; }
};

// The rings of a pair of directions by the job's rule.  K = 0: acc[0] is the plain ring on the job's nphi nodes; K >= 1: ring_modes
// with accumulator 0 the m = 0 ring and accumulators 1 .. mc the modes m_first ...
template <int K>
__device__ __forceinline__ void rings(const PhaseJob& a, int mc, double cc, double ss, double (&acc)[K ? K : 1]) {
    if constexpr (K == 0) acc[0] = ring(a.p, cc, ss, a.cosphi, a.wq, a.nphi);
    else ring_modes<K>(a.p, cc, ss, a.cosphi, a.wq, a.nphi, a.m_first, mc, acc);
}

// The value of accumulator j before the rescaling: a mode that vanishes identically is an exact zero
template <Second S, int K>
__device__ __forceinline__ double raw_value(const PhaseJob& a, int j, double acc) {
    if constexpr (K == 0) return Constants<S>::raw(acc);
    else return vanishes(a.p, a.m_first + j - 1) ? 0.0 : Constants<S>::raw(acc);
}

// The normaliser of the second direction (c, s = sin): trapz over the grid's 2N exits of the m = 0 ring (phase:103, 131), a
// workgroup reduction every thread gets the result of.  each(m, acc) sees the K accumulators of exit m on the way (the grid
// builders store them); a caller that only wants the normaliser asks for K = 1 (0 for the plain ring) and mc = 0.
template <Second S, int K, typename Each>
__device__ __forceinline__ double normaliser(const Grid& g, const PhaseJob& a, int mc, double c, double s, double* s_red, Each&& each) {
    const int tid = threadIdx.x, D = g.D;
    double part = 0;
    for (int m0 = 0; m0 < D; m0 += blockDim.x) {
        const int m = m0 + tid;
        if (m < D) {
            const double mu = g.mu[m];
            double acc[K ? K : 1];
            rings<K>(a, mc, mu * c, s * sqrt(1 - mu * mu), acc);
            part += a.w[m] * Constants<S>::raw(acc[0]);
            each(m, acc);
        }
    }
    return bsum(part, s_red);
}

// The job's arrays come once more as arguments of their own: only an argument's __restrict__ tells the compiler that the stores
// to out leave the weights and tables alone, which keeps their wave-uniform loads scalar.
#define PHASE_JOB_ARRAYS                                                                                                  \
    const double *__restrict__ w, const double *__restrict__ cosphi, const double *__restrict__ wq, const double *__restrict__ mu0, \
        const double *__restrict__ phi, double *__restrict__ out
__device__ __forceinline__ PhaseJob with_arrays(PhaseJob a, PHASE_JOB_ARRAYS) {
    a.w = w; a.cosphi = cosphi; a.wq = wq; a.mu0 = mu0; a.phi = phi; a.out = out;
    return a;
}

// out: table t (K = 0: the one table; else mode m_first + t), exit e, second direction blockIdx.x.  A column of the matrix is
// strided by D over the exits ([t][exit][D]); the values of a batch column are contiguous ([t][B][exit]).
template <Second S, Exits E, int K>
__global__ __launch_bounds__(256) void k_phase_pairs(Grid g, ViewMu vm, PhaseJob job, PHASE_JOB_ARRAYS) {
    const PhaseJob a = with_arrays(job, w, cosphi, wq, mu0, phi, out);
    using C = Constants<S>;
    constexpr int KA = K ? K : 1, J0 = K ? 1 : 0;            // accumulators; the first one that is stored
    const int tid = threadIdx.x, D = g.D;
    const int nE = E == NODES ? D : a.V2, nT = K ? a.m_count : 1;
    const size_t st = S == COLUMN ? (size_t)nE * D : (size_t)a.B * nE, se = S == COLUMN ? D : 1;
    double* o = a.out + (size_t)blockIdx.x * (S == COLUMN ? 1 : nE);
    __shared__ double s_red[8];
    auto signed_odd = [&](int t, double x) { return (a.sign_odd && ((a.m_first + t) & 1)) ? -x : x; };   // (-1)^m of mode m: exact
    if (a.p.kind == SOSRT_PHASE_ISO) {                       // no normalisation, no azimuth dependence: every mode m >= 1 vanishes
        // (a zero of the grid's tables carries the sign of its mode, -0 for an odd one under sign_odd; the lanes' zeros are +0)
        for (int t = 0; t < nT; ++t)
            for (int e = tid; e < nE; e += blockDim.x) o[t * st + e * se] = !K ? C::iso : E == NODES ? signed_odd(t, 0.0) : 0.0;
        return;
    }
    const double c = S == COLUMN ? g.mu[blockIdx.x] : a.mu0[blockIdx.x], s = sqrt(1 - c * c);
    if constexpr (E == NODES) {
        const double norm = normaliser<S, K>(g, a, a.m_count, c, s, s_red, [&](int m, const double(&acc)[KA]) {
#pragma unroll
            for (int j = J0; j < KA; ++j)
                if (j - J0 < nT) o[(j - J0) * st + m * se] = raw_value<S, K>(a, j, acc[j]);
        });
        for (int m = tid; m < D; m += blockDim.x)             // (each thread rescales what it wrote)
            for (int t = 0; t < nT; ++t) o[t * st + m * se] = signed_odd(t, C::scaled(o[t * st + m * se], norm));
    } else {
        const double norm = normaliser<S, K ? 1 : 0>(g, a, 0, c, s, s_red, [](int, const double(&)[1]) {});
        for (int e = tid; e < nE; e += blockDim.x) {
            const double x = vm.s[e];
            double acc[KA];
            rings<K>(a, a.m_count, x * c, s * sqrt(1 - x * x), acc);
#pragma unroll
            for (int j = J0; j < KA; ++j)
                if (j - J0 < nT) o[(j - J0) * st + e * se] = signed_odd(j - J0, C::scaled(raw_value<S, K>(a, j, acc[j]), norm));
        }
    }
}

// out[i][b][j] = p(c(s_j, mu0_b, phi_i)) / Z0_b, Z0_b the normaliser of the plain P0 rows: one workgroup per column
__global__ __launch_bounds__(256) void k_phase_p0_azimuth(Grid g, ViewMu vm, PhaseJob job, PHASE_JOB_ARRAYS) {
    const PhaseJob a = with_arrays(job, w, cosphi, wq, mu0, phi, out);
    const int b = blockIdx.x, tid = threadIdx.x, V2 = a.V2;
    const size_t BV = (size_t)a.B * V2;
    __shared__ double s_red[8];
    double* o = a.out + (size_t)b * V2;
    if (a.p.kind == SOSRT_PHASE_ISO) {
        for (int i = tid; i < a.nphi_out * V2; i += blockDim.x) o[(size_t)(i / V2) * BV + i % V2] = 1.0;
        return;
    }
    const double c0 = a.mu0[b];
    const double s0 = sqrt(1 - c0 * c0);
    const double norm = normaliser<MU0, 0>(g, a, 0, c0, s0, s_red, [](int, const double(&)[1]) {});
    for (int i = tid; i < a.nphi_out * V2; i += blockDim.x) {
        const int q = i / V2, j = i - q * V2;
        const double s = vm.s[j];
        const double c = -(s * c0 + s0 * sqrt(1 - s * s) * cos(a.phi[q]));
        o[(size_t)q * BV + j] = a.p(c) / norm;
    }
}

// out[b] = Z0_b, the normaliser k_phase_p0_azimuth divides by (for the isotropic function, which that kernel does not
// normalise, the value the rule gives: 1): one workgroup per column
__global__ __launch_bounds__(256) void k_phase_p0_normaliser(Grid g, PhaseJob job, PHASE_JOB_ARRAYS) {
    const PhaseJob a = with_arrays(job, w, cosphi, wq, mu0, phi, out);
    __shared__ double s_red[8];
    const double c0 = a.mu0[blockIdx.x];
    const double s0 = sqrt(1 - c0 * c0);
    const double norm = normaliser<MU0, 0>(g, a, 0, c0, s0, s_red, [](int, const double(&)[1]) {});
    if (threadIdx.x == 0) a.out[blockIdx.x] = norm;
}

// accumulators of the mode builders: the m = 0 ring plus mc modes, rounded up to a compiled size (column of the table below)
int modes_dispatch(int mc) { return mc == 0 ? 0 : mc + 1 <= 9 ? 1 : mc + 1 <= 17 ? 2 : mc + 1 <= 33 ? 3 : 4; }

}  // namespace

void launch_phase_builder(hipStream_t s, const Grid& g, const ViewMu* vm, const PhaseJob& job) {
    constexpr int KM = kMaxModes + 1;
    // [second direction][exits][accumulators]
    static constexpr decltype(&k_phase_pairs<COLUMN, NODES, 0>) kernels[2][2][5] = {
        {{k_phase_pairs<COLUMN, NODES, 0>, k_phase_pairs<COLUMN, NODES, 9>, k_phase_pairs<COLUMN, NODES, 17>,
          k_phase_pairs<COLUMN, NODES, 33>, k_phase_pairs<COLUMN, NODES, KM>},
         {k_phase_pairs<COLUMN, LANES, 0>, k_phase_pairs<COLUMN, LANES, 9>, k_phase_pairs<COLUMN, LANES, 17>,
          k_phase_pairs<COLUMN, LANES, 33>, k_phase_pairs<COLUMN, LANES, KM>}},
        {{k_phase_pairs<MU0, NODES, 0>, k_phase_pairs<MU0, NODES, 9>, k_phase_pairs<MU0, NODES, 17>, k_phase_pairs<MU0, NODES, 33>,
          k_phase_pairs<MU0, NODES, KM>},
         {k_phase_pairs<MU0, LANES, 0>, k_phase_pairs<MU0, LANES, 9>, k_phase_pairs<MU0, LANES, 17>, k_phase_pairs<MU0, LANES, 33>,
          k_phase_pairs<MU0, LANES, KM>}},
    };
    const auto kernel = job.phi ? k_phase_p0_azimuth : kernels[job.mu0 ? MU0 : COLUMN][job.V2 ? LANES : NODES][modes_dispatch(job.m_count)];
    hipLaunchKernelGGL(kernel, dim3(job.mu0 ? job.B : g.D), dim3(256), 0, s, g, vm ? *vm : ViewMu{}, job, job.w, job.cosphi, job.wq,
                       job.mu0, job.phi, job.out);
}

void launch_phase_p0_normaliser(hipStream_t s, const Grid& g, const PhaseJob& job) {
    hipLaunchKernelGGL(k_phase_p0_normaliser, dim3(job.B), dim3(256), 0, s, g, job, job.w, job.cosphi, job.wq, job.mu0, job.phi,
                       job.out);
}

}  // namespace sosrt
