// Phase matrices of a handle: sosrt_set_phase* (fold, flip-symmetry measure, low-rank certificate of W_atm, aerosol sets),
// atmosphere phase sets, the read-backs about them, and the matrices a solve derives from them on the device (combined
// slab matrices, folded copies of the symmetric contraction, float copies).  Host code; the kernels are in kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "handle.hpp"

using namespace sosrt;

namespace sosrt {

// buffers of the float contraction (SOSRT_CONTRACT_F32)
int ensure_w32(sosrt_handle* h) {
    if (h->gemm.mode != SOSRT_CONTRACT_F32) return 0;
    if (h->cols.nslab > 0 && h->cols.mix_groups == 0)
        return fail(SOSRT_E_INVALID, "the float contraction needs at most %d distinct slab coefficient pairs in a batch", sosrt_handle::Columns::kMaxMixGroups);
    const size_t need = (size_t)h->g.Dp * h->g.Wld * (size_t)(h->cols.mix_groups > 0 ? h->cols.mix_groups : 1);
    const bool grows = need > h->cols.d_Wmix32.cap;
    if (int e = h->cols.d_Wmix32.reserve(need)) return e;
    if (grows) h->phase.w32_dirty = true;
    return 0;
}

// combined slab matrices and, for the symmetric contraction, the folded copies of every matrix (on stream s)
int ensure_matrices(sosrt_handle* h, hipStream_t s) {
    const Grid& g = h->g;
    const size_t per = (size_t)g.Dp * g.Wld;
    const bool mixed = h->cols.mix_groups > 0 && h->cols.mix_dirty;
    if (mixed) {
        prof_break(h);
        const bool sets = h->cols.max_set_used > 0, atm = h->cols.max_atm_used > 0;
        launch_wmix(s, per, h->cols.mix_groups, atm ? h->phase.d_Wasets.p : h->phase.d_Wa, sets ? h->phase.d_Wrsets.p : h->phase.d_Wr, h->cols.d_mixca, h->cols.d_mixcr,
                    h->cols.d_Wmix.p, sets ? h->cols.d_mixset : nullptr, atm ? h->cols.d_mixatm : nullptr);
        h->cols.mix_dirty = false;
        h->phase.symmix_dirty = true;
    }
    if (!use_sym(h)) return 0;
    if (h->phase.sym_dirty) {
        prof_break(h);
        if (!h->phase.d_Wa_s) { if (int e = dalloc(&h->phase.d_Wa_s, per)) return e; }
        if (!h->phase.d_Wr_s) { if (int e = dalloc(&h->phase.d_Wr_s, per)) return e; }
        launch_symfold(s, 1, g.N, g.D, g.Dp, g.Wld, h->phase.d_Wa, h->phase.d_Wa_s);
        launch_symfold(s, 1, g.N, g.D, g.Dp, g.Wld, h->phase.d_Wr, h->phase.d_Wr_s);
        h->phase.sym_dirty = false;
        h->phase.symsets_dirty = true;
    }
    // the folded copies of every set: only the two-pass form with sets reads them
    if (h->phase.symsets_dirty && h->phase.nsets > 1 && h->cols.mix_groups == 0 && h->cols.max_set_used > 0) {
        prof_break(h);
        if (int e = h->phase.d_Wrsets_s.reserve(per * h->phase.nsets)) return e;
        launch_symfold(s, h->phase.nsets, g.N, g.D, g.Dp, g.Wld, h->phase.d_Wrsets.p, h->phase.d_Wrsets_s.p);
        h->phase.symsets_dirty = false;
    }
    if (h->cols.mix_groups > 0 && h->phase.symmix_dirty) {
        prof_break(h);
        if (int e = h->cols.d_Wmix_s.reserve(per * h->cols.mix_groups)) return e;
        launch_symfold(s, h->cols.mix_groups, g.N, g.D, g.Dp, g.Wld, h->cols.d_Wmix.p, h->cols.d_Wmix_s.p);
        h->phase.symmix_dirty = false;
    }
    return 0;
}

}  // namespace sosrt

// max |W[k][m] - W[D-1-k][D-1-m]| / max |W| of a folded matrix: the flip-symmetry measure of sosrt_set_phase* and of
// sosrt_set_atm_phase_sets (see sosrt.h, sosrt_set_contraction)
static double flip_asymmetry(const std::vector<double>& W, int D) {
    double wmax = 0, amax = 0;
    for (int k = 0; k < D; ++k)
        for (int m = 0; m < D; ++m) {
            const double x = W[(size_t)k * D + m], y = W[(size_t)(D - 1 - k) * D + (D - 1 - m)];
            const double ax = std::fabs(x), d = std::fabs(x - y);
            if (!(ax <= wmax)) wmax = ax;          // a NaN ends up here and switches the symmetric form off
            if (!(d <= amax)) amax = d;
        }
    return wmax > 0 ? amax / wmax : 0.0;
}

// Common part of sosrt_set_phase / sosrt_set_phase_sets[_dev]: S aerosol matrices [S][2N][2N] (S = 0: none), host (P_aer) or
// device (d_P_aer: folded and measured on the device, in the handle's stream order; the host keeps no copy of their folds
// until sosrt_plan_fold asks for one)
static int set_phase_impl(sosrt_handle* h, const double* P_atm, int S, const double* P_aer, const double* d_P_aer = nullptr) {
    if (!h || !P_atm) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (h->have_cols && h->cols.max_set_used >= (S > 0 ? S : 1))
        return fail(SOSRT_E_INVALID, "the current columns use aerosol set %d, but only %d set(s) are given (sosrt_set_columns resets them to set 0)",
                    h->cols.max_set_used, S > 0 ? S : 1);
    if (S > 1 && h->first_order_mode == SOSRT_FIRST_ORDER_README)
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one aerosol matrix: it cannot be combined with %d phase sets", S);
    if (h->have_cols && h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "the current columns use atmosphere set %d, and sosrt_set_phase leaves one atmosphere set (sosrt_set_columns resets them to set 0)",
                    h->cols.max_atm_used);
    const size_t DD = (size_t)h->D * h->D;
    h->plan.fold(P_atm, h->phase.Wa_h);
    h->have_aer = S > 0;
    h->phase.wr_on_device = d_P_aer != nullptr;
    if (S > 0 && !d_P_aer) h->plan.fold(P_aer, h->phase.Wr_h);
    else h->phase.Wr_h.clear();
    h->phase.Wrx_h.clear();
    h->phase.Wrx_h.resize(S > 1 ? S - 1 : 0);
    for (int q = 1; q < S && !d_P_aer; ++q) h->plan.fold(P_aer + (size_t)q * DD, h->phase.Wrx_h[q - 1]);
    h->phase.nsets = S > 1 ? S : 1;
    h->phase.natm = 1;
    h->have_phase = true;
    h->cols.mix_dirty = true;
    h->phase.w32_dirty = true;
    h->phase.sym_dirty = true; h->phase.symmix_dirty = true; h->phase.symsets_dirty = true;
    {   // flip symmetry of the folded matrices (see sosrt.h, sosrt_set_contraction): the maximum over W_atm and every set
        const int D = h->D;
        h->phase.asymmetry = 0;
        std::vector<const std::vector<double>*> all = {&h->phase.Wa_h, &h->phase.Wr_h};
        for (const auto& W : h->phase.Wrx_h) all.push_back(&W);
        for (const std::vector<double>* W : all) {
            if (W->empty()) continue;
            const double r = flip_asymmetry(*W, D);
            if (!(r <= h->phase.asymmetry)) h->phase.asymmetry = r;
        }
        // (a compile-time constant: nothing in the environment can put the symmetric form on a matrix without the symmetry)
        h->phase.sym_ok = h->phase.asymmetry <= SOSRT_SYMMETRY_TOL;      // (device sets: their measure joins below)
    }
    // low rank of W_atm (see sosrt.h, sosrt_phase_rank): from the matrix alone, never from the batch
    std::vector<double> lrU, lrV;
    h->phase.lr_rank = lowrank_factor(h->phase.Wa_h, h->D, kLowRankMax, SOSRT_LOWRANK_TOL, lrU, lrV, &h->phase.lr_residual);
    if (h->gpu) {
        HIPCHK(hipSetDevice(h->device));
        const Grid& g = h->g;
        HIPCHK(hipMemcpy2D(h->phase.d_Wa, g.Wld * sizeof(double), h->phase.Wa_h.data(), g.D * sizeof(double), g.D * sizeof(double),
                           g.D, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->phase.d_lrU, lrU.data(), lrU.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->phase.d_lrV, lrV.data(), lrV.size() * sizeof(double), hipMemcpyHostToDevice));
        if (S > 0 && !d_P_aer)
            HIPCHK(hipMemcpy2D(h->phase.d_Wr, g.Wld * sizeof(double), h->phase.Wr_h.data(), g.D * sizeof(double),
                               g.D * sizeof(double), g.D, hipMemcpyHostToDevice));
        if (d_P_aer) {
            // fold and asymmetry measure on the device: the matrices never visit the host, two partial maxima per block do
            constexpr int kAsymBlocks = 32;
            const size_t per = (size_t)g.Dp * g.Wld, scratch = (size_t)2 * kAsymBlocks * S;
            if (int e = h->phase.d_Wrsets.reserve(per * S + scratch)) return e;
            hipStream_t s = h->stream;
            double* d_part = h->phase.d_Wrsets.p + per * S;
            HIPCHK(hipMemsetAsync(h->phase.d_Wrsets.p, 0, per * S * sizeof(double), s));       // the padding rows and columns stay zero
            launch_fold_sets(s, S, g.D, g.Wld, per, h->grid.d_w, d_P_aer, h->phase.d_Wrsets.p);
            launch_fold_asymmetry(s, S, kAsymBlocks, g.D, g.Wld, per, h->phase.d_Wrsets.p, d_part);
            HIPCHK(hipMemcpyAsync(h->phase.d_Wr, h->phase.d_Wrsets.p, per * sizeof(double), hipMemcpyDeviceToDevice, s));
            std::vector<double> part(scratch);
            HIPCHK(hipMemcpyAsync(part.data(), d_part, scratch * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipGetLastError());
            for (int q = 0; q < S; ++q) {
                double wmax = 0, amax = 0;
                for (int b = 0; b < kAsymBlocks; ++b) {
                    const double w = part[((size_t)q * kAsymBlocks + b) * 2], a = part[((size_t)q * kAsymBlocks + b) * 2 + 1];
                    if (!(w <= wmax)) wmax = w;              // (a NaN ends up here, as in the host loop)
                    if (!(a <= amax)) amax = a;
                }
                const double r = (wmax != wmax || amax != amax) ? std::nan("") : (wmax > 0 ? amax / wmax : 0.0);
                if (!(r <= h->phase.asymmetry)) h->phase.asymmetry = r;
            }
            h->phase.sym_ok = h->phase.asymmetry <= SOSRT_SYMMETRY_TOL;
        } else if (S > 1) {
            const size_t per = (size_t)g.Dp * g.Wld;
            if (int e = h->phase.d_Wrsets.reserve(per * S)) return e;
            HIPCHK(hipMemset(h->phase.d_Wrsets.p, 0, per * S * sizeof(double)));       // the padding rows and columns stay zero
            for (int q = 0; q < S; ++q)
                HIPCHK(hipMemcpy2D(h->phase.d_Wrsets.p + q * per, g.Wld * sizeof(double), (q ? h->phase.Wrx_h[q - 1] : h->phase.Wr_h).data(),
                                   g.D * sizeof(double), g.D * sizeof(double), g.D, hipMemcpyHostToDevice));
        }
    }
    return 0;
}

extern "C" {

int sosrt_phase_asymmetry(sosrt_t* h, double* asymmetry, int* uses_symmetry) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (asymmetry) *asymmetry = h->phase.asymmetry;
    if (uses_symmetry) *uses_symmetry = use_sym(h) ? 1 : 0;
    return 0;
}

int sosrt_phase_rank(sosrt_t* h, int* rank, double* residual, int* uses) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (rank) *rank = h->phase.lr_rank;
    if (residual) *residual = h->phase.lr_residual;
    if (uses) *uses = use_lowrank(h) ? 1 : 0;
    return 0;
}

int sosrt_set_phase(sosrt_t* h, const double* P_atm, const double* P_aer) {
    return set_phase_impl(h, P_atm, P_aer ? 1 : 0, P_aer);
}

int sosrt_set_phase_sets(sosrt_t* h, const double* P_atm, int S, const double* P_aer) {
    if (!h || !P_atm || !P_aer) return fail(SOSRT_E_INVALID, "null argument");
    if (S < 1 || S > SOSRT_MAX_PHASE_SETS) return fail(SOSRT_E_INVALID, "S=%d outside 1..SOSRT_MAX_PHASE_SETS=%d", S, SOSRT_MAX_PHASE_SETS);
    return set_phase_impl(h, P_atm, S, P_aer);
}

int sosrt_set_phase_sets_dev(sosrt_t* h, const double* P_atm, int S, const double* d_P_aer) {
    if (!h || !P_atm || !d_P_aer) return fail(SOSRT_E_INVALID, "null argument");
    if (S < 1 || S > SOSRT_MAX_PHASE_SETS) return fail(SOSRT_E_INVALID, "S=%d outside 1..SOSRT_MAX_PHASE_SETS=%d", S, SOSRT_MAX_PHASE_SETS);
    if (int e = need_gpu(h)) return e;
    return set_phase_impl(h, P_atm, S, nullptr, d_P_aer);
}

int sosrt_phase_sets_info(sosrt_t* h, int* out) {
    if (!h || !out) return fail(SOSRT_E_INVALID, "null argument");
    out[0] = h->phase.nsets;
    out[1] = h->have_cols ? h->cols.mix_groups : 0;
    out[2] = (h->have_cols && (h->cols.nslab == 0 || h->cols.mix_groups > 0)) ? 1 : 0;
    out[3] = h->have_grid ? mix_group_cap(h, true) : 0;
    return 0;
}

int sosrt_set_atm_phase_sets(sosrt_t* h, int S_atm, const double* P_atm_sets) {
    if (!h || !P_atm_sets) return fail(SOSRT_E_INVALID, "null argument");
    if (int e = need_gpu(h)) return e;
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called (it defines the aerosol matrices; the atmosphere sets follow it)");
    if (S_atm < 1 || S_atm > SOSRT_MAX_PHASE_SETS)
        return fail(SOSRT_E_INVALID, "S_atm=%d outside 1..SOSRT_MAX_PHASE_SETS=%d", S_atm, SOSRT_MAX_PHASE_SETS);
    if (h->have_cols && h->cols.max_atm_used >= S_atm)
        return fail(SOSRT_E_INVALID, "the current columns use atmosphere set %d, but only %d set(s) are given (sosrt_set_columns resets them to set 0)",
                    h->cols.max_atm_used, S_atm);
    if (S_atm > 1) {
        if (h->gemm.mode != SOSRT_CONTRACT_F64)
            return fail(SOSRT_E_INVALID, "atmosphere phase sets need SOSRT_CONTRACT_F64: their plain rows exist in its low-rank form only "
                                         "(the other contractions tile row lists that straddle columns)");
        if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with %d atmosphere sets", S_atm);
        if (!h->phase.sym_ok)
            return fail(SOSRT_E_INVALID, "atmosphere phase sets need the flip-symmetric contraction, and the matrices of the last sosrt_set_phase "
                                         "are not symmetric (asymmetry %.3g > %.3g)", h->phase.asymmetry, (double)SOSRT_SYMMETRY_TOL);
    }
    // every set: folded as sosrt_set_phase folds W_atm, then the same two certificates; nothing changes unless all pass
    const int D = h->D;
    const size_t DD = (size_t)D * D, LR = (size_t)kLowRankMax * D;
    std::vector<std::vector<double>> W(S_atm);
    std::vector<double> U(LR * S_atm), V(LR * S_atm), res(S_atm);
    std::vector<int> ranks(S_atm);
    double asym = 0;
    for (int q = 0; q < S_atm; ++q) {
        h->plan.fold(P_atm_sets + (size_t)q * DD, W[q]);
        std::vector<double> u, v;
        ranks[q] = lowrank_factor(W[q], D, kLowRankMax, SOSRT_LOWRANK_TOL, u, v, &res[q]);
        if (ranks[q] < 0)
            return fail(SOSRT_E_INVALID, "atmosphere set %d is not low-rank: no factorisation of at most %d terms within %.3g of its largest element "
                                         "(residual %.3g; a NaN or an infinity gives this too) -- atmosphere sets take the low-rank form of the plain rows only",
                        q, kLowRankMax, (double)SOSRT_LOWRANK_TOL, res[q]);
        const double r = flip_asymmetry(W[q], D);
        if (!(r <= SOSRT_SYMMETRY_TOL))
            return fail(SOSRT_E_INVALID, "atmosphere set %d is not flip-symmetric: asymmetry %.3g > %.3g", q, r, (double)SOSRT_SYMMETRY_TOL);
        if (r > asym) asym = r;
        std::copy(u.begin(), u.end(), U.begin() + LR * q);
        std::copy(v.begin(), v.end(), V.begin() + LR * q);
    }
    HIPCHK(hipSetDevice(h->device));
    const Grid& g = h->g;
    const size_t per = (size_t)g.Dp * g.Wld;
    if ((size_t)S_atm > h->phase.d_lrranks.cap) {        // (the new stacks first: a failure leaves the old ones in place)
        GrowBuf<double> nW, nU, nV;
        GrowBuf<int> nR;
        int e = nW.reserve(per * S_atm);
        if (!e) e = nU.reserve(LR * S_atm);
        if (!e) e = nV.reserve(LR * S_atm);
        if (!e) e = nR.reserve((size_t)S_atm);
        if (!e) { nW.swap(h->phase.d_Wasets); nU.swap(h->phase.d_lrUsets); nV.swap(h->phase.d_lrVsets); nR.swap(h->phase.d_lrranks); }
        nW.release(); nU.release(); nV.release(); nR.release();       // the old stacks -- or, after a failure, the new ones
        if (e) return e;
    }
    HIPCHK(hipStreamSynchronize(h->stream));             // a solve in flight still reads W_atm
    HIPCHK(hipMemset(h->phase.d_Wasets.p, 0, per * S_atm * sizeof(double)));       // the padding rows and columns stay zero
    for (int q = 0; q < S_atm; ++q)
        HIPCHK(hipMemcpy2D(h->phase.d_Wasets.p + q * per, g.Wld * sizeof(double), W[q].data(), g.D * sizeof(double), g.D * sizeof(double),
                           g.D, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->phase.d_lrUsets.p, U.data(), U.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->phase.d_lrVsets.p, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->phase.d_lrranks.p, ranks.data(), ranks.size() * sizeof(int), hipMemcpyHostToDevice));
    // set 0 is the handle's W_atm: what sosrt_set_phase would have left for this matrix
    h->phase.Wa_h = W[0];
    HIPCHK(hipMemcpy2D(h->phase.d_Wa, g.Wld * sizeof(double), h->phase.Wa_h.data(), g.D * sizeof(double), g.D * sizeof(double), g.D,
                       hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->phase.d_lrU, U.data(), LR * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->phase.d_lrV, V.data(), LR * sizeof(double), hipMemcpyHostToDevice));
    h->phase.lr_rank = ranks[0]; h->phase.lr_residual = res[0];
    if (asym > h->phase.asymmetry) h->phase.asymmetry = asym;        // (still within the tolerance: the choice of the symmetric form stands)
    h->phase.natm = S_atm;
    h->cols.mix_dirty = true; h->phase.w32_dirty = true;
    h->phase.sym_dirty = true; h->phase.symmix_dirty = true;
    return 0;
}

int sosrt_atm_sets_info(sosrt_t* h, int* out) {
    if (!h || !out) return fail(SOSRT_E_INVALID, "null argument");
    out[0] = h->phase.natm;
    out[1] = (h->have_cols && h->cols.max_atm_used > 0) ? 1 : 0;
    return 0;
}

}  // extern "C"
