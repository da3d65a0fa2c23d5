// C ABI of libsosrt.so (see include/sosrt.h): the error text, life cycle of a handle, streams, the setters that are not
// about phase matrices or columns, sosrt_set_grid, fluxes and the epilogue, the sosrt_plan_* read-backs, profiling, diagnostics (stamps,
// machine peaks -- the kernels they time are in kernels.hip), and the RCCL gather.  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "handle.hpp"

using namespace sosrt;

namespace sosrt {
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace sosrt

constexpr int kProfPool = 8192;

extern "C" {

const char* sosrt_last_error(void) { return g_err.c_str(); }
int sosrt_version(void) { return SOSRT_VERSION; }

int sosrt_plan_fix_count(double tau_ref, int N) { return fix_count(tau_ref, N); }

int sosrt_create(int device, int L, int N, int max_batch, int max_orders, sosrt_t** out) {
    if (!out) return fail(SOSRT_E_INVALID, "out is null");
    *out = nullptr;
    if (L < 2) return fail(SOSRT_E_INVALID, "nb_layers must be >= 2 (got %d)", L);
    if (N < 4) return fail(SOSRT_E_INVALID, "nb_angles must be >= 4 (got %d)", N);
    if (N > 1024) return fail(SOSRT_E_INVALID, "nb_angles must be <= 1024 (got %d)", N);
    if (max_batch < 1 || max_orders < 1) return fail(SOSRT_E_INVALID, "max_batch and max_orders must be >= 1");
    {   // the first-order kernel keeps three values per layer of its column in LDS (the largest per-layer need of any kernel)
        const int nt = (N + 63) / 64 * 64;
        const size_t need = (size_t)(3 * (size_t)L + nt + nt / 64 + 4) * sizeof(double);
        if (need > 64 * 1024)
            return fail(SOSRT_E_INVALID, "nb_layers = %d does not fit: at most %d layers at nb_angles = %d", L,
                        (int)((64 * 1024 / sizeof(double) - nt - nt / 64 - 4) / 3), N);
    }
    sosrt_handle* h = new (std::nothrow) sosrt_handle();
    if (!h) return fail(SOSRT_E_NOMEM, "out of host memory");
    h->device = device; h->L = L; h->N = N; h->D = 2 * N; h->max_batch = max_batch; h->max_orders = max_orders;
    h->order_budget = max_orders;
    h->saved_slots = max_orders;
    h->gpu = device >= 0;
    h->cu_count = 256;                       // (a host-only handle plans for an MI355X; a device handle asks the device below)
    if (const char* ev = getenv("SOSRT_ETAB")) h->tr.use_etab = atoi(ev);
    if (const char* ev = getenv("SOSRT_CONTRACT"))            // "full": the D x D product whatever the symmetry of the matrices
        if (strcmp(ev, "full") == 0) h->gemm.mode = SOSRT_CONTRACT_F64_FULL;
    if (const char* ev = getenv("SOSRT_TRANSPORT"))
        h->tr.mode = strcmp(ev, "general") == 0 ? TransportKnob::General : (strcmp(ev, "ring") == 0 ? TransportKnob::Ring : (strcmp(ev, "scan") == 0 ? TransportKnob::Scan : (strcmp(ev, "auto") == 0 ? TransportKnob::Auto : TransportKnob::Fast)));
    if (const char* ev = getenv("SOSRT_SCAN_COLS")) h->tr.scan_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_RING_MOMENTS")) h->tr.ring_moments = atoi(ev) != 0;
    if (const char* ev = getenv("SOSRT_SCAN_MOMENTS")) h->tr.scan_moments = atoi(ev) != 0;
    if (const char* ev = getenv("SOSRT_SCAN_MOMENTS_MIN")) h->tr.scan_moments_min_live = atoi(ev);
    if (const char* ev = getenv("SOSRT_SCAN_SPLIT")) h->tr.scan_split = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_TAIL")) h->gemm.gemm_tail_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_TAIL_FRAC")) h->gemm.gemm_tail_frac = atof(ev);
    if (const char* ev = getenv("SOSRT_GEMM_SMALL")) h->gemm.gemm_small_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_DENSE_LIVE_LIST")) h->gemm.dense_live_list = atoi(ev) != 0;
    if (const char* ev = getenv("SOSRT_GEMM_REGS")) h->gemm.gemm_regs_cols = atoi(ev);           // (A/B: 0 = the staged tilings for every live count)
    if (const char* ev = getenv("SOSRT_GROUPS")) h->grp.want_groups = atoi(ev) >= 2 ? 2 : (atoi(ev) == 1 ? 1 : 0);      // column groups of the order loop (0: auto)
    if (const char* ev = getenv("SOSRT_SPLIT_MIN")) h->grp.split_min = atoi(ev);                  // smallest batch that is split
    if (const char* ev = getenv("SOSRT_MIX_GROUPS")) h->cols.mix_groups_max = atoi(ev);          // (tests, A/B: fewer combined matrices than the cache would hold -- the two-pass form sooner)
#ifdef SOSRT_DIAG   // measurement knobs of DESIGN section 5 (items 1, 5, 8): diagnostic builds only (-DSOSRT_DIAG), never in the product library
    if (const char* ev = getenv("SOSRT_STAGGER")) h->grp.stagger = atof(ev);
    if (const char* ev = getenv("SOSRT_GROUP_SPLIT")) h->grp.split_at = atoi(ev);
    if (const char* ev = getenv("SOSRT_GROUP_PRIO")) h->grp.prio2 = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_PAD_LDS")) h->grp.coresident_pad = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_KS_MULT")) h->gemm.diag_ks_mult = atoi(ev);
#endif
    if (const char* ev = getenv("SOSRT_GROUP_RING_SLOTS")) h->grp.coresident_slots = atoi(ev);
    if (const char* ev = getenv("SOSRT_ORDER_LOOP")) h->ol.mode = atoi(ev) != 0;           // (A/B: 0 = every order as two launches)
    if (const char* ev = getenv("SOSRT_RING_SLOTS")) h->tr.ring_slots = atoi(ev);
#ifdef SOSRT_RING_DEBUG   // diagnostic builds only: the switches make the ring kernel skip work, its results are wrong
    if (const char* ev = getenv("SOSRT_RING_DEBUG")) h->tr.ring_debug = atoi(ev);
#endif
    Grid& g = h->g;
    g.L = L; g.N = N; g.D = 2 * N;
    g.Dp = (g.D + GEMM_KC - 1) / GEMM_KC * GEMM_KC;
    g.Wld = (g.D + GEMM_BN - 1) / GEMM_BN * GEMM_BN;
    if (h->gpu) {
        int e = 0;
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(device));
            // the handle's own stream is a BLOCKING stream: it orders against the legacy default stream (handle NULL), which is
            // where a caller without an explicit stream -- torch's default stream is that one -- fills and reads its buffers
            HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault));
            h->stream = h->own_stream;
            // (the second group's stream is created when a batch first takes two groups: HIP maps streams onto a few hardware
            // queues, and a handle that never splits should not take one from the caller's other streams)
            HIPCHK(hipEventCreateWithFlags(&h->grp.ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->grp.ev_join, hipEventDisableTiming));
            const size_t mb = max_batch, fe = field_elems(h);
            if ((e = dalloc(&h->grid.d_mu, g.D))) return e;
            if ((e = dalloc(&h->phase.d_Wa, (size_t)g.Dp * g.Wld))) return e;
            if ((e = dalloc(&h->phase.d_Wr, (size_t)g.Dp * g.Wld))) return e;
            if ((e = dalloc(&h->phase.d_lrU, (size_t)kLowRankMax * g.D))) return e;
            if ((e = dalloc(&h->phase.d_lrV, (size_t)kLowRankMax * g.D))) return e;
            if ((e = dalloc(&h->grid.d_wfdn, N))) return e;
            if ((e = dalloc(&h->grid.d_wfup, N))) return e;
            if ((e = dalloc(&h->grid.d_w, g.D))) return e;
            if ((e = dalloc(&h->grid.d_phi, 2 * kNPhi))) return e;
            if ((e = dalloc(&h->grid.d_z, L))) return e;
            if ((e = dalloc(&h->grid.d_fix, 4))) return e;
            if ((e = dalloc(&h->grid.d_small, N))) return e;
            if ((e = dalloc(&h->cols.d_idx_up, mb))) return e;
            if ((e = dalloc(&h->cols.d_idx_down, mb))) return e;
            if ((e = dalloc(&h->cols.d_nz, mb))) return e;
            if ((e = dalloc(&h->cols.d_zr0, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->cols.d_zmix, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->cols.d_zwr, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->cols.d_zdtr, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->cols.d_scal, 7 * mb))) return e;
            if ((e = dalloc(&h->cols.d_desc, mb))) return e;
            if ((e = dalloc(&h->cols.d_rca, mb * L))) return e;
            if ((e = dalloc(&h->cols.d_rcr, mb * L))) return e;
            if ((e = dalloc(&h->cols.d_slabrows, mb * L + 64 * (size_t)sosrt_handle::Columns::kMaxMixGroupsSets * sosrt_handle::kMaxGroups))) return e;   // + padding
            if ((e = dalloc(&h->cols.d_slabtilegroup, mb * L / 32 + 2 * sosrt_handle::Columns::kMaxMixGroupsSets * sosrt_handle::kMaxGroups + 2))) return e;
            if ((e = dalloc(&h->cols.d_mainrows, mb * L))) return e;
            if ((e = dalloc(&h->fld.d_tau, mb * L))) return e;
            if ((e = dalloc(&h->fld.d_P0a, mb * g.D))) return e;
            if ((e = dalloc(&h->fld.d_P0r, mb * g.D))) return e;
            if ((e = dalloc(&h->fld.d_Jn, fe))) return e;
            if ((e = dalloc(&h->fld.d_InA, fe))) return e;
            if ((e = dalloc(&h->fld.d_InB, fe))) return e;
            if ((e = dalloc(&h->fld.d_I, fe))) return e;
            if ((e = dalloc(&h->fld.d_E, fe))) return e;
            if ((e = dalloc(&h->fld.d_active, mb))) return e;
            if ((e = dalloc(&h->fld.d_norders, mb))) return e;
            if ((e = dalloc(&h->fld.d_status, mb))) return e;
            if ((e = dalloc(&h->fld.d_nactive_sets, 2 * (sosrt_handle::kMaxGroups + 1)))) return e;   // live columns per group; any column needs k_smallmu
            HIPCHK(hipMemset(h->fld.d_nactive_sets, 0, 2 * (sosrt_handle::kMaxGroups + 1) * sizeof(int)));
            h->fld.d_nactive = h->fld.d_nactive_sets;
            if ((e = dalloc(&h->fld.d_redo, mb))) return e;
            if ((e = dalloc(&h->fld.d_erep, mb))) return e;
            if ((e = dalloc(&h->cols.d_mixgroup, mb))) return e;
            if ((e = dalloc(&h->gemm.d_livelist, mb))) return e;
            if ((e = dalloc(&h->cols.d_mixca, sosrt_handle::Columns::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->cols.d_mixcr, sosrt_handle::Columns::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->cols.d_mixset, sosrt_handle::Columns::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->cols.d_mixatm, sosrt_handle::Columns::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->cols.d_colatm, mb))) return e;
            if ((e = dalloc(&h->fld.d_tauhash, mb))) return e;
            if ((e = dalloc(&h->fld.d_ratio, mb))) return e;
            if ((e = dalloc(&h->tr.d_scan_scratch, mb * transport_scan_scratch_doubles()))) return e;
            if ((e = dalloc(&h->tr.d_scan_sync, 2 * mb))) return e;
            if ((e = dalloc(&h->tr.d_mom, mb * L * kMomDoubles))) return e;
            if ((e = dalloc(&h->ol.d_sync, sosrt_handle::kMaxGroups * order_loop_sync_ints(kOrderLoopMaxCols)))) return e;
            HIPCHK(hipHostMalloc((void**)&h->ol.h_done, 2 * sosrt_handle::kMaxGroups * sizeof(int), hipHostMallocCoherent));
            memset(h->ol.h_done, 0, 2 * sosrt_handle::kMaxGroups * sizeof(int));
            HIPCHK(hipMemset(h->tr.d_scan_sync, 0, 2 * mb * sizeof(int)));
            HIPCHK(hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, device));
            // + 2 ints at the end: {needs k_smallmu, tag} published at the start of a solve
            HIPCHK(hipHostMalloc((void**)&h->fld.h_pub, (8 * sosrt_handle::kMaxGroups + 2) * sizeof(int), hipHostMallocCoherent));
            memset(h->fld.h_pub, 0, (8 * sosrt_handle::kMaxGroups + 2) * sizeof(int));

            HIPCHK(hipMemset(h->phase.d_Wa, 0, (size_t)g.Dp * g.Wld * sizeof(double)));
            HIPCHK(hipMemset(h->phase.d_Wr, 0, (size_t)g.Dp * g.Wld * sizeof(double)));
            HIPCHK(hipMemset(h->fld.d_status, 0, mb * sizeof(int)));
            HIPCHK(hipMemset(h->fld.d_redo, 0, mb * sizeof(int)));
            HIPCHK(hipMemset(h->fld.d_tau, 0, mb * L * sizeof(double)));
            return 0;
        };
        if ((e = body())) { sosrt_destroy(h); return e; }
        g.mu = h->grid.d_mu; g.Wa = h->phase.d_Wa; g.Wr = h->phase.d_Wr; g.fix = h->grid.d_fix; g.small_lanes = h->grid.d_small;
        g.wflux_dn = h->grid.d_wfdn; g.wflux_up = h->grid.d_wfup; g.nsmall = 0;
    }
    *out = h;
    return 0;
}

int sosrt_destroy(sosrt_t* h) {
    if (!h) return 0;
    if (h->gpu) {
        hipSetDevice(h->device);
        if (h->net.comm) { rccl().CommDestroy(h->net.comm); h->net.comm = nullptr; }
        if (h->own_stream) hipStreamSynchronize(h->own_stream);
        void* ptrs[] = {h->grid.d_mu, h->phase.d_Wa, h->phase.d_Wr, h->grid.d_wfdn, h->grid.d_wfup, h->grid.d_fix, h->grid.d_small, h->cols.d_idx_up,
                        h->cols.d_idx_down, h->cols.d_scal, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr, h->cols.d_slabrows, h->cols.d_mainrows, h->fld.d_tau, h->fld.d_P0a,
                        h->fld.d_P0r, h->fld.d_Jn, h->fld.d_InA, h->fld.d_InB, h->fld.d_I, h->fld.d_E, h->fld.d_active, h->fld.d_norders, h->fld.d_status,
                        h->fld.d_nactive_sets, h->fld.d_ratio, h->fld.d_redo, h->fld.d_erep, h->fld.d_tauhash, h->cols.d_mixca, h->cols.d_mixcr,
                        h->cols.d_mixgroup, h->phase.d_Wa_s, h->phase.d_Wr_s, h->tr.d_scan_scratch, h->tr.d_scan_sync, h->grid.d_w, h->grid.d_phi, h->grid.d_z, h->pf.d_tab, h->cols.d_slabtilegroup, h->gemm.d_livelist, h->phase.d_Wa32, h->cols.d_nz, h->cols.d_zr0, h->cols.d_zmix, h->cols.d_zwr, h->cols.d_zdtr, h->ol.d_sync, h->ol.d_log, h->phase.d_lrU, h->phase.d_lrV, h->cols.d_mixset,
                        h->cols.d_colatm, h->cols.d_mixatm, h->tr.d_mom};
        for (void* p : ptrs)
            if (p) hipFree(p);
        if (h->fld.h_pub) hipHostFree(h->fld.h_pub);
        if (h->ol.h_done) hipHostFree(h->ol.h_done);
        h->cols.d_Wmix.release(); h->cols.d_Wmix_s.release(); h->cols.d_Wmix32.release(); h->cols.d_P0rz.release();
        h->cols.d_rwa.release(); h->cols.d_rwr.release();
        h->phase.d_Wrsets.release(); h->phase.d_Wrsets_s.release(); h->phase.d_Wasets.release(); h->phase.d_lrUsets.release();
        h->phase.d_lrVsets.release(); h->phase.d_lrranks.release(); h->pf.d_modetab.release(); h->pf.d_mie.release(); h->pf.h_mie.release();
        h->pf.d_deltam.release();
        h->view.d_fold.release(); h->view.d_S.release(); h->view.d_rc.release(); h->view.d_desc.release();
        for (auto& e : h->view.ev)
            if (e) hipEventDestroy(e);
        if (h->pf.mie_ev) hipEventDestroy(h->pf.mie_ev);
        for (auto& e : h->pf.mie_t)
            if (e) hipEventDestroy(e);

        for (auto& p : h->prof)
            for (auto& e : p.ev) hipEventDestroy(e);
        if (h->grp.stream2) { hipStreamSynchronize(h->grp.stream2); hipStreamDestroy(h->grp.stream2); }
        if (h->grp.ev_fork) hipEventDestroy(h->grp.ev_fork);
        if (h->grp.ev_join) hipEventDestroy(h->grp.ev_join);
        if (h->own_stream) hipStreamDestroy(h->own_stream);
    }
    delete h;
    return 0;
}

int sosrt_set_stream(sosrt_t* h, void* s) {
    if (int e = need_gpu(h)) return e;
    h->stream = (hipStream_t)s;              // NULL is the legacy default stream, as everywhere in HIP
    return 0;
}

int sosrt_use_own_stream(sosrt_t* h) {
    if (int e = need_gpu(h)) return e;
    h->stream = h->own_stream;
    return 0;
}

int sosrt_set_saved_orders(sosrt_t* h, int slots) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (slots < 1 || slots > h->max_orders) return fail(SOSRT_E_INVALID, "slots must be in 1..max_orders=%d (got %d)", h->max_orders, slots);
    h->saved_slots = slots;
    return 0;
}

int sosrt_set_order_budget(sosrt_t* h, int max_orders) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (max_orders < 1 || max_orders > h->max_orders)
        return fail(SOSRT_E_INVALID, "the order budget must be in 1..max_orders=%d of sosrt_create (got %d)", h->max_orders, max_orders);
    h->order_budget = max_orders;
    return 0;
}

int sosrt_set_first_order(sosrt_t* h, int mode) {
    if (int e = need_gpu(h)) return e;
    if (mode != SOSRT_FIRST_ORDER_CODED && mode != SOSRT_FIRST_ORDER_README) return fail(SOSRT_E_INVALID, "unknown first-order mode %d", mode);
    if (mode == SOSRT_FIRST_ORDER_README && (h->phase.nsets > 1 || h->cols.p0_zones > 0))
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one aerosol matrix: it cannot be combined with several phase sets");
    if (mode == SOSRT_FIRST_ORDER_README && (h->phase.natm > 1 || h->cols.max_atm_used > 0))
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with atmosphere phase sets");
    if (mode == SOSRT_FIRST_ORDER_README && h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "the README's Lambertian first order needs the three-zone geometry (it has a surface)");
    h->first_order_mode = mode;
    return 0;
}

int sosrt_set_contraction(sosrt_t* h, int mode) {
    if (int e = need_gpu(h)) return e;
    if (mode != SOSRT_CONTRACT_F64 && mode != SOSRT_CONTRACT_F32 && mode != SOSRT_CONTRACT_F64_FULL && mode != SOSRT_CONTRACT_F64_DENSE) return fail(SOSRT_E_INVALID, "unknown contraction mode %d", mode);
    if (mode != SOSRT_CONTRACT_F64 && (h->phase.natm > 1 || h->cols.max_atm_used > 0))
        return fail(SOSRT_E_INVALID, "atmosphere phase sets are in use: their plain rows exist in the low-rank form of SOSRT_CONTRACT_F64 only "
                                     "(the other contractions tile row lists that straddle columns)");
    if (mode == SOSRT_CONTRACT_F32) {
        HIPCHK(hipSetDevice(h->device));
        const size_t per = (size_t)h->g.Dp * h->g.Wld;
        if (!h->phase.d_Wa32) { if (int e = dalloc(&h->phase.d_Wa32, per)) return e; }
        h->phase.w32_dirty = true;
    }
    h->gemm.mode = mode;
    return 0;
}

int sosrt_set_order_loop(sosrt_t* h, int mode) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (mode < 0 || mode > 2) return fail(SOSRT_E_INVALID, "order-loop mode must be 0, 1 or 2 (got %d)", mode);
    h->ol.mode = mode;
    return 0;
}

int sosrt_order_loop_stats(sosrt_t* h, int* launches, int* refused, long long* column_orders) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (launches) *launches = h->ol.launches;
    if (refused) *refused = h->ol.refused;
    if (column_orders) {
        *column_orders = 0;
        if (h->gpu && h->ol.launches > 0) {             // every launch of the last solve left its count in its group's words
            HIPCHK(hipSetDevice(h->device));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (h->grp.stream2) HIPCHK(hipStreamSynchronize(h->grp.stream2));
            for (int k = 0; k < sosrt_handle::kMaxGroups; ++k) {
                if (!h->ol.group_used[k]) continue;
                int v = 0;
                HIPCHK(hipMemcpy(&v, h->ol.d_sync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols) + kOlOrders, sizeof v, hipMemcpyDeviceToHost));
                *column_orders += v;
            }
        }
    }
    return 0;
}

int sosrt_ring_moments_stats(sosrt_t* h, int* moment_orders, int* orders) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (moment_orders) *moment_orders = h->tr.moment_orders;
    if (orders) *orders = h->tr.orders;
    return 0;
}

int sosrt_scan_moments_stats(sosrt_t* h, int* moment_orders, int* orders) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (moment_orders) *moment_orders = h->tr.scan_moment_orders;
    if (orders) *orders = h->tr.orders;
    return 0;
}

int sosrt_synchronize(sosrt_t* h) {
    if (int e = need_gpu(h)) return e;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int sosrt_set_grid(sosrt_t* h, const double* mu) {
    if (!h || !mu) return fail(SOSRT_E_INVALID, "null argument");
    for (int k = 0; k < h->D; ++k)
        if (!std::isfinite(mu[k])) return fail(SOSRT_E_INVALID, "mu[%d] is not finite", k);
    for (int k = 0; k < h->N; ++k) {
        if (!(mu[k] <= 0)) return fail(SOSRT_E_INVALID, "mu[%d]=%g: the first nb_angles directions must be <= 0", k, mu[k]);
        if (!(mu[h->N + k] >= 0)) return fail(SOSRT_E_INVALID, "mu[%d]=%g: the last nb_angles directions must be >= 0", h->N + k, mu[h->N + k]);
    }
    h->plan.set_grid(h->N, mu);
    for (int b = 0; b < 4; ++b)
        if (h->plan.fix[b].idx > kFixMaxIdx) return fail(SOSRT_E_INVALID, "nb_angles too large for the extrapolation tables");
    h->have_grid = true;
    h->have_phase = false;
    h->tr.fast_ok = transport_fast_ok(h->plan);
    if (h->gpu) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpy(h->grid.d_mu, mu, h->D * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->grid.d_wfdn, h->plan.wflux_dn.data(), h->N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->grid.d_wfup, h->plan.wflux_up.data(), h->N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->grid.d_w, h->plan.w.data(), h->D * sizeof(double), hipMemcpyHostToDevice));
        {   // phi = np.linspace(0, pi, 25) (phase:81-82): cos(phi0 - phi) and the trapezoid weights of np.trapz(., phi)
            double phi[kNPhi], tab[2 * kNPhi];
            const double step = 3.141592653589793 / (kNPhi - 1);
            for (int q = 0; q < kNPhi; ++q) phi[q] = q * step;
            phi[kNPhi - 1] = 3.141592653589793;
            for (int q = 0; q < kNPhi; ++q) {
                tab[q] = std::cos(0 - phi[q]);
                tab[kNPhi + q] = ((q > 0 ? phi[q] - phi[q - 1] : 0.0) + (q + 1 < kNPhi ? phi[q + 1] - phi[q] : 0.0)) / 2;
            }
            HIPCHK(hipMemcpy(h->grid.d_phi, tab, sizeof tab, hipMemcpyHostToDevice));
        }
        std::vector<FixTab> ft(4);
        for (int b = 0; b < 4; ++b) {
            const FixTable& t = h->plan.fix[b];
            memset(&ft[b], 0, sizeof(FixTab));
            ft[b].idx = t.idx; ft[b].s0 = t.s0; ft[b].ns = t.ns;
            for (size_t i = 0; i < t.C.size(); ++i) ft[b].C[i] = t.C[i];
        }
        HIPCHK(hipMemcpy(h->grid.d_fix, ft.data(), 4 * sizeof(FixTab), hipMemcpyHostToDevice));
        h->g.nsmall = (int)h->plan.small_lanes.size();
        if (h->g.nsmall)
            HIPCHK(hipMemcpy(h->grid.d_small, h->plan.small_lanes.data(), h->g.nsmall * sizeof(int), hipMemcpyHostToDevice));
    }
    // which kernels take this shape (pure functions of the grid: a host-only handle answers sosrt_plan_launch with them)
    h->g.nsmall = (int)h->plan.small_lanes.size();
    h->tr.ring_ok = h->tr.fast_ok && transport_ring_ok(h->g);
    h->tr.scan_ok = h->tr.ring_ok && transport_scan_ok(h->g);
    // (N in (128, 256]: the chunk-parallel kernel has this form only; it does not need the ring kernel's shape -- odd N, N up to
    // 512 and L up to 1024 take its WIDE instantiation: the reference's shipped N = 501, L = 800)
    // (nor the condition of the wave-independent kernels that the rewritten mu -> 0- directions and their sources sit in the last
    // wave of a half row: part 0 of the split form holds the downward directions N-64 .. N-1 in ONE wave whatever N is)
    h->tr.scan_split_ok = transport_scan_split_ok(h->g);
    return 0;
}

int sosrt_fluxes(sosrt_t* h, int B, const double* tau, const double* I, int beam_norm, double* flux_down,
                 double* flux_up) {
    if (int e = check_ready(h, B, false)) return e;
    if (!tau || !I || !flux_down || !flux_up) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    h->resident = false;                     // d_tau and d_I are overwritten
    hipStream_t s = h->stream;
    const size_t n = (size_t)B * h->L * h->D, r = (size_t)B * h->L;
    HIPCHK(hipMemcpyAsync(h->fld.d_tau, tau, r * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->fld.d_I, I, n * sizeof(double), hipMemcpyHostToDevice, s));
    launch_prepare(s, h->g, B, h->geom, h->surface, scalars_of(h), h->fld.d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr);
    launch_fluxes(s, h->g, B, h->fld.d_tau, h->fld.d_I, h->cols.d_desc, beam_norm, h->cols.d_rca, h->cols.d_rcr);   // row-sized scratch
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(flux_down, h->cols.d_rca, r * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flux_up, h->cols.d_rcr, r * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// epilogue on a resident field
// ---------------------------------------------------------------------------------------------
int sosrt_epilogue_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, int beam_norm, const double* d_z_profile,
                       double* d_flux_down, double* d_flux_up, double* d_diffusivity, double* d_heating_rate,
                       double* d_net_toa) {
    if (int e = check_ready(h, B, false)) return e;
    if (!d_tau || !d_I) return fail(SOSRT_E_INVALID, "null argument");
    if (d_heating_rate && !d_z_profile) return fail(SOSRT_E_INVALID, "the heating rate needs z_profile");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    launch_prepare(s, h->g, B, h->geom, h->surface, scalars_of(h), d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr);
    EpilogueOut out{d_flux_down, d_flux_up, d_diffusivity, d_heating_rate, d_net_toa};
    launch_epilogue(s, h->g, h->grid.d_w, B, d_tau, d_I, h->cols.d_desc, beam_norm, d_z_profile, out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_epilogue(sosrt_t* h, int B, int beam_norm, const double* z_profile, double* flux_down, double* flux_up,
                   double* diffusivity, double* heating_rate, double* net_toa) {
    if (int e = check_ready(h, B, false)) return e;
    if (!h->resident) return fail(SOSRT_E_STATE, "no resident field: call sosrt_solve first (and nothing that overwrites it since)");
    if (B != h->resident_B) return fail(SOSRT_E_INVALID, "B=%d but the resident field is of %d columns", B, h->resident_B);
    if (heating_rate && !z_profile) return fail(SOSRT_E_INVALID, "the heating rate needs z_profile");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t r = (size_t)B * h->L;
    if (4 * r + B > field_elems(h)) return fail(SOSRT_E_INVALID, "batch too large for the scratch buffer");
    if (z_profile) HIPCHK(hipMemcpyAsync(h->grid.d_z, z_profile, h->L * sizeof(double), hipMemcpyHostToDevice, s));
    double* o = h->fld.d_Jn;                                     // scratch: the source function of the last order is dead
    if (int e = sosrt_epilogue_dev(h, B, h->fld.d_tau, h->fld.d_I, beam_norm, z_profile ? h->grid.d_z : nullptr, flux_down ? o : nullptr,
                                   flux_up ? o + r : nullptr, diffusivity ? o + 2 * r : nullptr,
                                   heating_rate ? o + 3 * r : nullptr, net_toa ? o + 4 * r : nullptr))
        return e;
    if (flux_down) HIPCHK(hipMemcpyAsync(flux_down, o, r * sizeof(double), hipMemcpyDeviceToHost, s));
    if (flux_up) HIPCHK(hipMemcpyAsync(flux_up, o + r, r * sizeof(double), hipMemcpyDeviceToHost, s));
    if (diffusivity) HIPCHK(hipMemcpyAsync(diffusivity, o + 2 * r, r * sizeof(double), hipMemcpyDeviceToHost, s));
    if (heating_rate) HIPCHK(hipMemcpyAsync(heating_rate, o + 3 * r, r * sizeof(double), hipMemcpyDeviceToHost, s));
    if (net_toa) HIPCHK(hipMemcpyAsync(net_toa, o + 4 * r, B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU gather over RCCL
// ---------------------------------------------------------------------------------------------
#define NCCLCHK(x)                                                                                          \
    do {                                                                                                    \
        const int r_ = (x);                                                                                 \
        if (r_ != 0) return fail(SOSRT_E_HIP, "%s failed: %s", #x, rccl().GetErrorString(r_));              \
    } while (0)

int sosrt_comm_unique_id(void* id_out) {
    if (!id_out) return fail(SOSRT_E_INVALID, "null argument");
    if (const char* e = rccl().load()) return fail(SOSRT_E_STATE, "%s", e);
    Rccl::UniqueId id;
    NCCLCHK(rccl().GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return 0;
}

int sosrt_comm_init(sosrt_t* h, int rank, int world, const void* unique_id) {
    if (int e = need_gpu(h)) return e;
    if (!unique_id || world < 1 || rank < 0 || rank >= world) return fail(SOSRT_E_INVALID, "bad rank / world / id");
    if (h->net.comm) return fail(SOSRT_E_STATE, "the handle already has a communicator");
    if (const char* e = rccl().load()) return fail(SOSRT_E_STATE, "%s", e);
    HIPCHK(hipSetDevice(h->device));
    Rccl::UniqueId id;
    memcpy(&id, unique_id, sizeof id);
    NCCLCHK(rccl().CommInitRank(&h->net.comm, world, id, rank));
    h->net.rank = rank; h->net.world = world;
    return 0;
}

int sosrt_gather(sosrt_t* h, int root, const long long* counts, const double* d_send, double* d_recv) {
    if (int e = need_gpu(h)) return e;
    if (!h->net.comm) return fail(SOSRT_E_STATE, "sosrt_comm_init has not been called");
    if (!counts || root < 0 || root >= h->net.world) return fail(SOSRT_E_INVALID, "bad root / counts");
    for (int r = 0; r < h->net.world; ++r)
        if (counts[r] < 0) return fail(SOSRT_E_INVALID, "counts[%d] < 0", r);
    const int me = h->net.rank;
    if (counts[me] > 0 && !d_send) return fail(SOSRT_E_INVALID, "d_send is null");
    if (me == root && !d_recv) return fail(SOSRT_E_INVALID, "d_recv is null on the root");
    HIPCHK(hipSetDevice(h->device));
    const int kF64 = 8;                                      // ncclFloat64
    // every exit below goes through GroupEnd: a group left open would swallow the communicator's next calls
    int rc = 0, nrc = 0;
    hipError_t hrc = hipSuccess;
    NCCLCHK(rccl().GroupStart());
    if (me == root) {
        size_t off = 0;
        for (int r = 0; r < h->net.world && !nrc && hrc == hipSuccess; ++r) {
            if (counts[r] > 0) {
                if (r == me) {
                    if (d_recv + off != d_send)
                        hrc = hipMemcpyAsync(d_recv + off, d_send, (size_t)counts[r] * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
                } else {
                    nrc = rccl().Recv(d_recv + off, (size_t)counts[r], kF64, r, h->net.comm, h->stream);
                }
            }
            off += (size_t)counts[r];
        }
    } else if (counts[me] > 0) {
        nrc = rccl().Send(d_send, (size_t)counts[me], kF64, root, h->net.comm, h->stream);
    }
    const int erc = rccl().GroupEnd();
    if (hrc != hipSuccess) rc = fail(SOSRT_E_HIP, "sosrt_gather: copy of the root's own block failed: %s", hipGetErrorString(hrc));
    else if (nrc) rc = fail(SOSRT_E_HIP, "sosrt_gather: ncclSend/ncclRecv failed: %s", rccl().GetErrorString(nrc));
    else if (erc) rc = fail(SOSRT_E_HIP, "sosrt_gather: ncclGroupEnd failed: %s", rccl().GetErrorString(erc));
    return rc;
}

int sosrt_comm_destroy(sosrt_t* h) {
    if (int e = need_gpu(h)) return e;
    if (h->net.comm) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        NCCLCHK(rccl().CommDestroy(h->net.comm));
        h->net.comm = nullptr; h->net.rank = -1; h->net.world = 0;
    }
    return 0;
}

int sosrt_limit_mu_down(sosrt_t* h, int R, int idx, const double* rows, double* out) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (R < 1 || !rows || !out) return fail(SOSRT_E_INVALID, "bad argument");
    int table = -1;
    for (int b = 0; b < 4; ++b)
        if (h->plan.fix[b].idx == idx) table = b;
    if (table < 0) return fail(SOSRT_E_INVALID, "idx=%d is not one of the reference's int(c*nb_angles) values for nb_angles=%d", idx, h->N);
    if (idx == 0) return 0;
    if ((size_t)R * h->N > field_elems(h)) return fail(SOSRT_E_INVALID, "too many rows");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->fld.d_Jn, rows, (size_t)R * h->N * sizeof(double), hipMemcpyHostToDevice, s));
    launch_limit_rows(s, h->g, R, table, h->fld.d_Jn, h->fld.d_InB);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->fld.d_InB, (size_t)R * idx * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int sosrt_asymptotic_down(sosrt_t* h, int R, int stride, const int* len, const double* J, const double* tau,
                          const double* tau_t, const double* mu, double* out) {
    if (int e = need_gpu(h)) return e;
    if (R < 1 || stride < 1 || !len || !J || !tau || !tau_t || !mu || !out) return fail(SOSRT_E_INVALID, "bad argument");
    const size_t n = (size_t)R * stride;
    if (2 * n + 4 * (size_t)R > field_elems(h)) return fail(SOSRT_E_INVALID, "too many rows");
    for (int r = 0; r < R; ++r)
        if (len[r] < 0 || len[r] > stride) return fail(SOSRT_E_INVALID, "len[%d] out of range", r);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dJ = h->fld.d_Jn; double* dT = h->fld.d_Jn + n;
    double* dtt = h->fld.d_InB; double* dmu = h->fld.d_InB + R; double* dout = h->fld.d_InB + 2 * (size_t)R;
    int* dlen = (int*)(h->fld.d_InA);
    HIPCHK(hipMemcpyAsync(dJ, J, n * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dT, tau, n * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dtt, tau_t, R * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dmu, mu, R * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlen, len, R * sizeof(int), hipMemcpyHostToDevice, s));
    launch_asymptotic(s, R, stride, dlen, dJ, dT, dtt, dmu, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, R * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// plan introspection (host only)
// ---------------------------------------------------------------------------------------------
int sosrt_plan_weights(sosrt_t* h, double* w_out) {
    if (!h || !w_out) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    memcpy(w_out, h->plan.w.data(), h->D * sizeof(double));
    return 0;
}

int sosrt_plan_fold(sosrt_t* h, int which, double* W_out) {
    if (!h || !W_out) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (which < 0 || which > h->phase.nsets) return fail(SOSRT_E_INVALID, "which=%d: 0 is W_atm, 1 + s the aerosol set s of %d", which, h->phase.nsets);
    std::vector<double>& W = which > 1 ? h->phase.Wrx_h[which - 2] : (which ? h->phase.Wr_h : h->phase.Wa_h);
    if (which >= 1 && h->phase.wr_on_device && h->have_aer && W.empty()) {       // a fold made on the device: fetched when asked for
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        W.assign((size_t)h->D * h->D, 0.0);
        HIPCHK(hipMemcpy2D(W.data(), h->D * sizeof(double), h->phase.d_Wrsets.p + (size_t)(which - 1) * h->g.Dp * h->g.Wld,
                           h->g.Wld * sizeof(double), h->D * sizeof(double), h->D, hipMemcpyDeviceToHost));
    }
    if (W.empty()) return fail(SOSRT_E_STATE, "that phase matrix was not set");
    memcpy(W_out, W.data(), W.size() * sizeof(double));
    return 0;
}

int sosrt_plan_fix_table(sosrt_t* h, int idx, int* s0, int* ns, double* C_out) {
    if (!h || !s0 || !ns) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (idx < 0 || idx > kFixMaxIdx || idx + 5 > h->N) return fail(SOSRT_E_INVALID, "idx out of range");
    FixTable t = h->plan.make_fix_table(idx);
    *s0 = t.s0; *ns = t.ns;
    if (C_out && !t.C.empty()) memcpy(C_out, t.C.data(), t.C.size() * sizeof(double));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// diagnostics: cycle stamps of k_transport_fast ([B][2 waves][8] clock64 values; pass NULL to stop), written by the transport
// launches of this handle alone
// ---------------------------------------------------------------------------------------------
int sosrt_debug_stamps(sosrt_t* h, unsigned long long* d_stamps) {
    if (int e = need_gpu(h)) return e;
    h->tr.d_stamps = d_stamps;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// machine peaks
// ---------------------------------------------------------------------------------------------
int sosrt_microbench(sosrt_t* h, int which, double* result) {
    if (int e = need_gpu(h)) return e;
    if (!result || which < 0 || (which > 2 && which < 10) || which > 49) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const size_t n = (size_t)1 << 27;                 // 1 GiB of doubles per buffer for the copy test
    double *a = nullptr, *b = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        const size_t na = which == 1 ? n : 16;
        if (int e = dalloc(&a, na)) return e;
        if (which == 1) { if (int e = dalloc(&b, na)) return e; HIPCHK(hipMemsetAsync(a, 0, na * sizeof(double), s)); }
        const int iters = 20000;
        double best = 0;
        for (int rep = 0; rep < 4; ++rep) {
            HIPCHK(hipEventRecord(e0, s));
            launch_bench(s, which, a, b, na, iters);
            HIPCHK(hipEventRecord(e1, s));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            double v;
            if (which >= 10) {
                const int code = which - 10, nacc = 2 << (code / 10), bpc = (code % 10) ? (code % 10) : 1;
                v = 256.0 * bpc * 4 * (double)iters * nacc * 2048.0 / (ms * 1e-3) / 1e12;
            } else if (which == 0) v = 2048.0 * 4 * (double)iters * 8 * 2048.0 / (ms * 1e-3) / 1e12;        // TFLOP/s
            else if (which == 1) v = 2.0 * na * sizeof(double) / (ms * 1e-3) / 1e9;                  // GB/s read+write
            else v = 2048.0 * 256 * (double)iters * 16 * 2.0 / (ms * 1e-3) / 1e12;                   // TFLOP/s
            if (rep > 0 && v > best) best = v;
        }
        *result = best;
        return 0;
    };
    rc = body();
    if (a) hipFree(a);
    if (b) hipFree(b);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
int sosrt_profile_enable(sosrt_t* h, int on) {
    if (int e = need_gpu(h)) return e;
    for (Prof& p : h->prof) {
        if (on && p.ev.empty()) {
            HIPCHK(hipSetDevice(h->device));
            p.ev.resize(2 * kProfPool);
            p.kind.assign(kProfPool, -1); p.first.assign(kProfPool, 0); p.last.assign(kProfPool, 0);
            // timing markers only: no system-scope fence (cache write-back / invalidate) at each of them
            for (auto& e : p.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        }
        p.on = on != 0;
    }
    return 0;
}

int sosrt_profile_reset(sosrt_t* h) {
    if (int e = need_gpu(h)) return e;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->grp.stream2) HIPCHK(hipStreamSynchronize(h->grp.stream2));
    for (Prof& p : h->prof) { p.used = 0; p.nint = 0; p.adjacent = -1; p.open = -1; }
    return 0;
}

int sosrt_profile_get(sosrt_t* h, int kernel, double* total_ms, long long* launches, double* work) {
    if (int e = need_gpu(h)) return e;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->grp.stream2) HIPCHK(hipStreamSynchronize(h->grp.stream2));
    double tot = 0;
    long long cnt = 0;
    for (Prof& p : h->prof)
        for (size_t i = 0; i < p.nint; ++i) {
            if (p.kind[i] != kernel) continue;
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, p.ev[p.first[i]], p.ev[p.last[i]]));
            tot += ms;
            ++cnt;
        }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = cnt;
    if (work) *work = 0;
    return 0;
}

}  // extern "C"
