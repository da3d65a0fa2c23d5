// The phase functions of the builders in phase.hip, their ring rules, and the one launcher of those builders (the matrix, P0, their
// Fourier modes in azimuth, and the rows of all four at view cosines off the grid).
// Phase-function kinds: isotropic (phase:68), Rayleigh (phase:79), Henyey-Greenstein (phase:141) and a
// tabulated function with the reference's linear interpolation (phase:198-236; fwc:3,173 is its table).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sosrt.h"
#include "kernels.hpp"

namespace sosrt {

struct PhaseFn {
    int kind;
    double g;
    const double* tab_mu;
    const double* tab_p;
    int ntab;
    // p(cos Theta)
    __device__ __forceinline__ double operator()(double c) const {
        if (kind == SOSRT_PHASE_RAYLEIGH) return (3.0 / 4) * (1 + c * c);                    // phase:96
        if (kind == SOSRT_PHASE_HG) {                                                         // phase:158
            const double x = 1 + g * g - 2 * g * c;
            return (1 - g * g) / (x * sqrt(x));
        }
        if (kind == SOSRT_PHASE_TABLE) {                                                      // phase:198-236
            c = fmin(fmax(c, -1.0), 1.0);
            int lo = 0, hi = ntab;                                                            // searchsorted, side='left'
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab_mu[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo == 0) return tab_p[0];
            if (lo >= ntab) return tab_p[ntab - 1];
            const double ml = tab_mu[lo - 1], mh = tab_mu[lo], pl = tab_p[lo - 1], ph = tab_p[lo];
            return pl + (c - ml) / (mh - ml) * (ph - pl);
        }
        return 1.0;
    }
};

// trapz over phi = linspace(0, pi, nphi) of p(cos Theta+) + p(cos Theta-), cos Theta+- = -(a b +- sa sb cos phi)
__device__ __forceinline__ double ring(const PhaseFn& p, double cc, double ss, const double* __restrict__ cosphi,
                                       const double* __restrict__ wphi, int nphi) {
    double acc = 0;
    for (int q = 0; q < nphi; ++q) {
        const double x = ss * cosphi[q];
        acc += wphi[q] * (p(-(cc + x)) + p(-(cc - x)));
    }
    return acc;
}

// Ring of mode m: R^m(a, b) = trapz_q [p(c(phi_q)) + (-1)^m p(c(phi_q + pi))] cos(m phi_q),
// c(phi) = -(mu_a mu_b + s_a s_b cos phi), phi_q = linspace(0, pi, nphi).  acc[0] is the m = 0 ring (the normaliser),
// acc[j], 1 <= j <= mc, mode mf + j - 1.  tab[j][q] = w_q cos(m_j phi_q) (row 0: w_q).  K is a compile-time bound so that
// the accumulators stay in registers; the guard j <= mc is uniform.
template <int K>
__device__ __forceinline__ void ring_modes(const PhaseFn& p, double cc, double ss, const double* __restrict__ cosphi,
                                           const double* __restrict__ tab, int nphi, int mf, int mc, double (&acc)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0;
    for (int q = 0; q < nphi; ++q) {
        const double x = ss * cosphi[q];
        const double p1 = p(-(cc + x)), p2 = p(-(cc - x));
        const double sp = p1 + p2, sm = p1 - p2;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j <= mc) acc[j] += tab[(size_t)j * nphi + q] * ((j > 0 && ((mf + j - 1) & 1)) ? sm : sp);
    }
}

// Rayleigh's p is quadratic in cos phi: its modes m >= 3 are zero, not rounding noise (a matrix of noise has no flip symmetry to
// rounding and would cost the solve of that mode the full contraction product)
__device__ __forceinline__ bool vanishes(const PhaseFn& p, int m) { return p.kind == SOSRT_PHASE_RAYLEIGH && m >= 3; }

// One launch of a phase builder (phase.hip).  What is built follows from the fields:
//   second direction  mu0 == nullptr: the grid's mu[n], a column of the matrix, tables [D exits][D] or rows [V2][D];
//                     else the batch columns' mu0 [B] (device), tables [B][D exits] or [B][V2]
//   exit directions   V2 == 0: the grid's 2N nodes; else the view cosines vm.s[0 .. V2)
//   ring rule         m_count == 0: the azimuth mean on nphi trapezoid nodes, cosphi [nphi] and wq [nphi] their weights, one table;
//                     else the modes [m_first, m_first + m_count), m_first >= 1, m_count <= kMaxModes: m_count tables, mode m as
//                     (-1)^m of it with sign_odd; wq [1 + m_count][nphi] holds the trapezoid weights (row 0, the m = 0 ring that
//                     normalises) and w_q cos(m phi_q) of each mode (modes_table, handle.hpp)
//   phi != nullptr    (mu0, view cosines, the plain ring) point values at the azimuths phi [nphi_out] (device) in place of a ring:
//                     out [nphi_out][B][V2] = p(c(s_j, mu0_b, phi_i)) / Z0_b
// w [D]: np.trapz weights on the whole direction grid.
struct PhaseJob {
    PhaseFn p;
    const double* w;
    const double* cosphi;
    const double* wq;
    int nphi, m_first, m_count, sign_odd;
    const double* mu0;
    int B, V2, nphi_out;
    const double* phi;
    double* out;
};
// vm may be null where V2 == 0
void launch_phase_builder(hipStream_t s, const Grid& g, const ViewMu* vm, const PhaseJob& job);
// out [B] = the normaliser of the plain P0 rows of the columns mu0 [B] (the plain ring): the Z0_b of the point values above,
// and nothing else
void launch_phase_p0_normaliser(hipStream_t s, const Grid& g, const PhaseJob& job);

}  // namespace sosrt
