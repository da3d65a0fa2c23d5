// The solve: the launch plan of an order (plan_order: host only, one place for the whole policy), the arguments of a transport
// launch (transport_args: one place for every condition on a field), the source-function launch, the order loop of sosrt_solve_dev with its lagged convergence polling, and the step-level entry points
// around them (fluxes and the epilogue on a resident field are in api.hip).  Host code, and one kernel: k_init_from_I1, the
// first order supplied by the caller.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "handle.hpp"

using namespace sosrt;

namespace {

// Spins on a pinned slot {value, tag, ...} until the device has written `tag`: 0, or an error code after 120 s without it --
// or, with a column group's stream to ask (grp >= 0), once that stream has failed or drained without the tag.
int await_tag(sosrt_handle* h, volatile int* slot, int tag, int grp) {
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::milliseconds(20);
    for (unsigned it = 1;; ++it) {
        if (__atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) == tag) return 0;
        // The stream is asked only when the wait is far longer than any order takes (an error has happened, or the GPU is shared):
        // hipStreamQuery puts a marker into the queue, and the kernel behind a marker starts ~6 us late (measured: a query every
        // 0.3 ms of waiting cost every dense order of the headline sweep that gap).
        if ((it & 0x3fff) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (grp >= 0 && now >= next_query) {
                next_query = now + std::chrono::milliseconds(20);
                const hipError_t q = hipStreamQuery(group_stream(h, grp));
                if (q != hipSuccess && q != hipErrorNotReady) return fail(SOSRT_E_HIP, "order loop: %s", hipGetErrorString(q));
                if (q == hipSuccess && __atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) != tag)
                    return fail(SOSRT_E_HIP, "order loop: the stream drained without publishing order tag %d", tag);
            }
            if (now - t0 > std::chrono::seconds(120)) return fail(SOSRT_E_HIP, "order loop: no progress for 120 s");
        }
        __builtin_ia32_pause();
    }
}

// Live columns after the order whose tag is `tag`, as published by the source-function launch of the
// next order (publish_live in kernels.hpp).  Spins on pinned memory; negative = error code.
int wait_published(sosrt_handle* h, int grp, int tag) {
    volatile int* slot = h->fld.h_pub + 8 * grp + 4 * (tag & 1);
    if (int e = await_tag(h, slot, tag, grp)) return e;
    h->fld.need_small = slot[2] != 0;
    return slot[0];
}

// What every contraction of the current columns reads, whoever launches it (call it after ensure_matrices, which may move the
// folded copies): the matrices, plain or folded, with Ks; the low-rank factors; the mix groups; the shape.  live_cols: also a
// column's slab bounds and the most rows any column has, which the tiles laid over live columns need.  The caller adds what is
// its own: operand and result, row lists, live list and publication (run_source), or none of them (the order-loop launch).
GemmArgs gemm_args(const sosrt_handle* h, bool live_cols) {
    GemmArgs ga{};
    ga.Wa = h->phase.d_Wa; ga.Wr = h->phase.d_Wr; ga.ca = h->cols.d_rca; ga.cr = h->cols.d_rcr;
    ga.D = h->g.D; ga.Dp = h->g.Dp; ga.Wld = h->g.Wld; ga.L = h->L;
    if (h->cols.mix_groups > 0) { ga.Wmix = h->cols.d_Wmix.p; ga.mix_group = h->cols.d_mixgroup; }
    const bool two_pass_sets = h->cols.mix_groups == 0 && h->cols.max_set_used > 0 && h->cols.nslab > 0;
    if (two_pass_sets) { ga.Wr = h->phase.d_Wrsets.p; ga.mix_group = h->cols.d_mixgroup; }   // the second pass picks the W_aer of a tile's / a column's set
    if (use_lowrank(h)) { ga.lr_rank = h->phase.lr_rank; ga.lrU = h->phase.d_lrU; ga.lrV = h->phase.d_lrV; }
    if (h->cols.max_atm_used > 0) { ga.lrU = h->phase.d_lrUsets.p; ga.lrV = h->phase.d_lrVsets.p; }   // (run_source: AtmSets)
    if (use_sym(h)) {
        ga.sym = 1; ga.Ks = (h->g.N + GEMM_KC - 1) / GEMM_KC * GEMM_KC;
        ga.Wa = h->phase.d_Wa_s; ga.Wr = two_pass_sets ? h->phase.d_Wrsets_s.p : h->phase.d_Wr_s;
        if (ga.Wmix) ga.Wmix = h->cols.d_Wmix_s.p;
    }
    if (live_cols) {
        ga.max_main = h->cols.max_main; ga.max_slab = h->cols.max_slab;
        ga.idx_up = h->cols.nslab > 0 ? h->cols.d_idx_up : nullptr; ga.idx_down = h->cols.nslab > 0 ? h->cols.d_idx_down : nullptr;
    }
    return ga;
}

struct SourceOpts {
    int tail_cols = 0;                   // > 0: tiles over the live columns, a launch of this capacity (else the dense tiling over the row lists)
    int pub_tag = 0;                     // != 0: the launch publishes the group's live count under this tag
    int grp = -1;                        // column group (< 0: the whole batch)
    bool all_live = false;               // the host knows every column of the launch to be live
    bool regs_tile = false;              // live columns: the register-resident 16-row tile (SOSRT_PLAN_GEMM_LIVE16_REGS)
    int dense_live_cap = 0;              // > 0: the dense tiling writes the transport's live list, of this capacity
    bool moments = false;                // the plain rows as moment records, not rows of Jn (LaunchPlan::moments or ::scan_moments)
};

// Jn for every row of a column group (grp < 0: the whole batch) in one launch: plain rows against W_atm, slab rows
// against the combined matrix of their coefficient pair (or W_atm and W_aer in two passes)
void run_source(sosrt_handle* h, const double* In_1, double* Jn, const int* active, const SourceOpts& o = SourceOpts()) {
    const int g0 = o.grp < 0 ? 0 : o.grp, g1 = o.grp < 0 ? h->grp.ngroups : o.grp + 1;
    const int pg = g0, col0 = h->grp.gb[g0], nb = h->grp.gb[g1] - col0;
    hipStream_t s = group_stream(h, pg);
    if (ensure_matrices(h, s)) return;                 // (allocation failure: reported by the caller's hipGetLastError / next call)
    const bool live_tiles = o.tail_cols > 0 && active && h->cols.nslab >= 0;
    GemmArgs ga = gemm_args(h, live_tiles);
    ga.A = In_1;
    if (h->cols.nslab > 0) {
        ga.rows_main = h->cols.d_mainrows + h->grp.main_off[g0];
        ga.n_main = h->grp.main_off[g1] - h->grp.main_off[g0];
    } else {                                           // no slab rows: the identity list, offset by the group's first row
        ga.rows_main = nullptr;
        ga.n_main = nb * h->L;
        ga.A = In_1 + (size_t)col0 * h->L * h->D;
        Jn += (size_t)col0 * h->L * h->D;
        ga.ca += (size_t)col0 * h->L;
        ga.cr += (size_t)col0 * h->L;
        if (active) active += col0;
    }
    // (records are indexed like the rows of Jn: by global row, or from the group's first row with the identity list)
    if (o.moments) ga.mom = h->tr.d_mom + (h->cols.nslab > 0 ? 0 : (size_t)col0 * h->L * kMomDoubles);
    ga.rows_slab = h->cols.d_slabrows + h->grp.slab_off[g0]; ga.n_slab = h->grp.slab_off[g1] - h->grp.slab_off[g0];
    ga.C = Jn; ga.active = active;
    if (ga.mix_group) ga.slab_tile_group = h->cols.d_slabtilegroup + h->grp.slab_off[g0] / 32;
    // Two column groups: the large tilings of the contraction are capped at two workgroups per CU (unused LDS up to a
    // third of the CU's) so that a transport workgroup of the other group -- 53 KB with a two-slot ring -- runs beside
    // them: the MFMA-bound contraction of one group then overlaps the HBM-bound transport of the other
    if (o.grp >= 0 && h->grp.ngroups > 1) ga.pad_lds = h->grp.coresident_pad;
    if (o.pub_tag) {
        ga.nactive = h->fld.d_nactive + pg; ga.need_small = h->fld.d_nactive + sosrt_handle::kMaxGroups;
        ga.host_pub = h->fld.h_pub + 8 * pg; ga.tag = o.pub_tag;
    }
    // The dense tiling skips the tiles whose columns have all converged -- two barriers and a dependent load per tile.  When the
    // host knows every column of the launch to be live (its count lags by one order: at most the columns that converged in the
    // last order are multiplied once more, and the transport ignores them) the check is dropped: 160 -> 157 us per 512-column launch.
    ga.check_tiles = o.all_live ? 0 : 1;
    // atmosphere sets in use: the launches' twins that pick a plain row's factors by its column's set (every set is low-rank, the
    // contraction is the symmetric f64 one: sosrt_set_atm_phase_sets / sosrt_set_atmosphere_sets refuse anything else)
    AtmSets at;
    const AtmSets* atp = nullptr;
    if (h->cols.max_atm_used > 0) {
        at.col_atm = h->cols.d_colatm + (h->cols.nslab > 0 ? 0 : col0);
        at.lr_ranks = h->phase.d_lrranks.p;
        atp = &at;
    }
#ifdef SOSRT_DIAG
    // diagnostic builds (timing only; the results do not change: the extra chunks multiply zeros): SOSRT_GEMM_KS_MULT=2 doubles
    // the chunks per tile at the same prologue / epilogue, which separates the two (tile time = P + chunks * C); read once,
    // at sosrt_create
    if (ga.sym && h->gemm.diag_ks_mult > 1 && ga.Ks * h->gemm.diag_ks_mult <= h->g.Dp) ga.Ks *= h->gemm.diag_ks_mult;
#endif
    if (h->gemm.mode == SOSRT_CONTRACT_F32) {
        // float operands, float accumulator: the dense tiling over the row lists for every order (tiles of converged
        // columns leave at once)
        if (h->phase.w32_dirty) {
            prof_break(h);
            const size_t per = (size_t)h->g.Dp * h->g.Wld;
            launch_to_float(s, per, h->phase.d_Wa, h->phase.d_Wa32);
            if (h->cols.mix_groups > 0) launch_to_float(s, per * h->cols.mix_groups, h->cols.d_Wmix.p, h->cols.d_Wmix32.p);
            h->phase.w32_dirty = false;
        }
        prof_begin(h, SOSRT_K_GEMM, pg);
        launch_gemm_f32(s, ga, h->phase.d_Wa32, h->cols.d_Wmix32.p);
        prof_end(h, SOSRT_K_GEMM, pg);
        return;
    }
    prof_begin(h, SOSRT_K_GEMM, pg);
    if (live_tiles || (o.dense_live_cap > 0 && active && h->cols.nslab >= 0)) {     // (the dense tiling writes the transport's live list too)
        ga.col0 = h->cols.nslab > 0 ? col0 : 0; ga.B = nb;
        ga.live_list = h->gemm.d_livelist + col0; ga.live_cap = live_tiles ? o.tail_cols : o.dense_live_cap;
    }
    if (live_tiles) launch_gemm_tail(s, ga, o.tail_cols, o.tail_cols <= h->gemm.gemm_small_cols, o.regs_tile, atp);
    else launch_gemm(s, ga, atp, h->cu_count);
    prof_end(h, SOSRT_K_GEMM, pg);
}

// ---------------------------------------------------------------------------------------------
// Launch plan: which kernels run an order of a column group.  One function, host only -- it reads the handle's shape and
// knobs and touches no device -- so that the policy can be read in one place and tested without a GPU (sosrt_plan_launch).
// ---------------------------------------------------------------------------------------------
struct SolveShape {                      // what a solve fixes for all its orders (from the grid and the batch's zone tables)
    bool ring_like = false;              // the ring / chunk-parallel kernels take the batch (they hold its zone tables)
    bool fast = false;                   // a wave-independent kernel runs (else the general kernel)
    int nzcap = kRingZones;              // most zones of any column, at least three
    bool ring_mode = false;              // the wave-independent kernel is of the ring class (else the register-streaming kernel)
};
static_assert((int)TransportKernel::General == SOSRT_PLAN_TRANSPORT_GENERAL && (int)TransportKernel::Fast == SOSRT_PLAN_TRANSPORT_FAST &&
              (int)TransportKernel::Ring == SOSRT_PLAN_TRANSPORT_RING && (int)TransportKernel::Scan == SOSRT_PLAN_TRANSPORT_SCAN,
              "sosrt_plan_launch reports TransportKernel as SOSRT_PLAN_TRANSPORT_*");
SolveShape solve_shape(const sosrt_handle* h, int max_nz) {
    SolveShape sh;
    // The ring / chunk-parallel kernels take columns of any zone count (an instantiation that tests every boundary of the zone
    // table, chosen when the batch holds such a column); the register-streaming kernel knows three zones, so a batch with more
    // goes to the general kernel where that one would run (odd N, N > 256).
    sh.ring_like = h->tr.mode >= TransportKnob::Ring && h->tr.ring_ok && (max_nz <= kRingZones || transport_ring_fits(h->g, max_nz));
    sh.fast = h->tr.mode >= TransportKnob::Fast && h->tr.fast_ok && (max_nz <= kRingZones || sh.ring_like);
    sh.nzcap = max_nz > kRingZones ? max_nz : kRingZones;
    sh.ring_mode = h->tr.mode >= TransportKnob::Ring && h->tr.ring_ok;
    return sh;
}
struct OrderInputs {                     // what the plan of one order depends on besides the handle
    int nb = 0;                          // columns of the group
    int known = 0;                       // upper bound of its live columns (the host's count lags by one order)
    int surface = SOSRT_SURFACE_NONE;
    bool simple_zones = true;            // every column is (clear, slab, clear), or a single slab
    bool slabs_mixed = true;             // slab rows have their combined matrices (or there are none)
    bool need_small = false;             // some |mu| < 0.01 lane keeps its k_smallmu value
    bool saving = false;                 // the caller wants every order's field (I_saved)
    int orders_left = 1 << 30;           // order budget from this order on
    int cu_share = 0;                    // CUs an order-loop launch of this group may take (0: none)
    bool atm_sets = false;               // some column reads an atmosphere phase set other than W_atm
    bool row_weights = false;            // per-level weights on the row coefficients (sosrt_set_row_weights_dev)
};
struct LaunchPlan {
    int tail_cols = 0;                   // contraction over the live columns: capacity of the launch (0: dense tiling over the row lists)
    int live_cap = 0;                    // transport over the live list: its capacity (0: over all columns of the group)
    int gemm = SOSRT_PLAN_GEMM_DENSE;
    TransportKernel transport = TransportKernel::General;
    int parts = 1;                       // chunk-parallel kernel: workgroups per column
    int repair = 0;                      // register-streaming kernel: the general kernel behind it for searches that leave wave 0
    int order_loop = 0;                  // this and every later order of the group in ONE order-loop launch
    int ol_parts = 0;                    // ... workgroups per column of its transport role
    int ol_grid = 0;                     // ... workgroups of the launch
    int moments = 0;                     // both launches of the order: moment records for the plain rows, expanded by the ring kernel
    int scan_moments = 0;                // ... expanded by the chunk-parallel kernel (never both)
};
LaunchPlan plan_order(const sosrt_handle* h, const SolveShape& sh, const OrderInputs& in) {
    LaunchPlan pl;
    const Grid& g = h->g;
    // contraction: the tilings over the live columns whenever some column has converged -- and for a small batch from the
    // start: their 32-row tiles put a few columns on more CUs than the dense tiling's 64-row tiles; same bits either way.
    // (the float contraction has the dense tiling only: no live list for the transport either)
    const bool live_tiling = h->gemm.mode != SOSRT_CONTRACT_F32 && in.simple_zones && in.known <= h->gemm.gemm_tail_cols &&
                             (in.known <= h->gemm.gemm_tail_frac * in.nb || in.nb <= h->gemm.gemm_small_cols) &&
                             (in.known < in.nb || in.nb <= h->gemm.gemm_small_cols);
    pl.tail_cols = live_tiling ? in.known : 0;
    pl.gemm = !live_tiling ? SOSRT_PLAN_GEMM_DENSE
                           : (pl.tail_cols <= h->gemm.gemm_small_cols ? ((use_sym(h) && pl.tail_cols <= 32) ? SOSRT_PLAN_GEMM_LIVE32_DEEP : SOSRT_PLAN_GEMM_LIVE32)
                                                                 : SOSRT_PLAN_GEMM_LIVE64);
    // The last few columns: a tile's latency is the launch's, and the register-resident 16-row tile (jn_gemm_tile.hpp:
    // gemm_tile_lone) has half the staged tile's -- a lone column's launch 12.6 -> 10.0 us at N = 128, 4.7 of which an empty launch
    // takes (profiles/r04_gemm_regs_ab.txt).  Its workgroups are alone on their CUs and each fetches its own share of the matrix:
    // it wins while they make at most about a round and a half (13 columns at L = 200, N = 128; 6 at N = 256), measured break-even
    // at 16 / 8 -- and loses where a lone column is already more than that: L = 800, N = 501, 133 -> 144 us per order (profiles/r04_gemm_regs_ab.txt).  (Its tile's rows of In_1 must fit the LDS, and N rounded up to the k-chunk must be whole register blocks of 64.)
    {
        const int nct = (g.D + GEMM_BN - 1) / GEMM_BN;
        const int auto_cap = (3 * h->cu_count / 2) / (((g.L + 15) / 16 + 1) * nct);
        const int cap = h->gemm.gemm_regs_cols >= 0 ? h->gemm.gemm_regs_cols : auto_cap;       // (0 at the reference's shipped size: 408 workgroups for a lone column)
        if (live_tiling && use_sym(h) && pl.tail_cols <= cap && 16 * (g.D + 2) * 8 <= 150 * 1024 &&
            ((g.N + GEMM_KC - 1) / GEMM_KC * GEMM_KC) % 64 == 0) pl.gemm = SOSRT_PLAN_GEMM_LIVE16_REGS;
    }
    // The transport takes its columns from the live list whenever some column has converged: the live-column tilings write the
    // list, and so does the dense tiling (one more workgroup) -- the ring-class kernels then run over the live columns, dealt to
    // the CUs one by one, instead of over a batch whose live columns sit where they were put.  (Not the float contraction.)
    pl.live_cap = live_tiling ? pl.tail_cols : ((h->gemm.mode != SOSRT_CONTRACT_F32 && h->gemm.dense_live_list && in.known < in.nb) ? in.known : 0);
    // transport
    {
        const int cols_now = pl.live_cap > 0 ? pl.live_cap : in.nb;
        // chunk-parallel kernel: a column on ceil(N / 64) CUs (two at N = 128, four at N = 256) while that many workgroups per
        // live column fit the device at once (the reflection must stay inside a part)
        // (where the shape has no ring kernel -- odd N, N > 256: the split form's WIDE instantiation -- the alternative is the
        // register-streaming kernel, one workgroup per column and 650 us per order at the shipped size against 133 for a round of
        // split workgroups: up to four rounds of them are the faster way)
        const int split_cap = sh.ring_mode ? h->cu_count : 4 * h->cu_count;
        const bool can_split = h->tr.scan_split && h->tr.scan_split_ok && transport_scan_parts(g) * cols_now <= split_cap &&
                               (in.surface == SOSRT_SURFACE_SPECULAR || in.surface == SOSRT_SURFACE_NONE);
        const bool want_scan = h->tr.mode == TransportKnob::Scan || (h->tr.mode == TransportKnob::Auto && cols_now <= h->tr.scan_cols);
        // (the split form also takes the shapes no wave-independent kernel does -- the rewritten directions straddle two waves of a
        // half row, e.g. N = 70, 129, 257: sh.fast is false -- as long as the attenuation tables are built)
        const bool split = can_split && transport_scan_fits(g, sh.nzcap, true) && (sh.fast || (h->tr.use_etab && h->tr.mode >= TransportKnob::Auto));
        const bool scan = want_scan && ((sh.fast && sh.ring_mode && h->tr.scan_ok && transport_scan_fits(g, sh.nzcap, false)) || split);
        pl.transport = scan ? TransportKernel::Scan
                            : (!sh.fast ? TransportKernel::General : (sh.ring_mode ? TransportKernel::Ring : TransportKernel::Fast));
        if (scan && split) pl.parts = transport_scan_parts(g);
        pl.repair = (h->N - 3 > 61 && pl.transport == TransportKernel::Fast) ? 1 : 0;
    }
    // order-loop kernel: the remaining orders in one launch once the live columns' transport workgroups are a small share of the
    // CUs it may take (the other workgroups contract).  It holds the chunk-parallel transport (three zones, no kept k_smallmu
    // lane) and the symmetric contraction's live-column tiles; the default transport policy only (a forced kernel stays forced).
    if (h->ol.mode && in.cu_share > 0 && h->tr.mode == TransportKnob::Auto && sh.fast && sh.ring_mode && sh.nzcap <= kRingZones &&
        use_sym(h) && in.simple_zones && in.slabs_mixed && !in.saving && !in.row_weights && !in.need_small && in.orders_left >= 1 &&
        in.known <= kOrderLoopMaxCols) {
        Grid gt = g;
        gt.nsmall = 0;
        const bool split_ok = h->tr.scan_split && (in.surface == SOSRT_SURFACE_SPECULAR || in.surface == SOSRT_SURFACE_NONE) && order_loop_ok(gt, true);
        const int sp = order_loop_parts(gt, true);
        if (split_ok && sp * in.known <= h->ol.frac * in.cu_share) {
            pl.order_loop = 1; pl.ol_parts = sp;
        } else if (order_loop_ok(gt, false) && in.known <= h->ol.frac * in.cu_share) {
            pl.order_loop = 1; pl.ol_parts = 1;
        }
        if (pl.order_loop) pl.ol_grid = in.cu_share;
    }
    // Moment mode, for the contraction and the transport of the order at once: the plain rows in the low-rank form of the symmetric
    // f64 contraction, one W_atm for the batch, no saved orders, the ring kernel for every column of the group (its three-zone
    // instantiation) and no k_smallmu launch, which reads rows of Jn.  Anything else: rows of Jn, as always.
    pl.moments = (h->tr.ring_moments && use_lowrank(h) && use_sym(h) && !in.atm_sets && !in.saving && !pl.order_loop &&
                  pl.transport == TransportKernel::Ring && sh.nzcap <= kRingZones && !in.need_small) ? 1 : 0;
    // The same for an order the chunk-parallel kernel transports -- a decision of its own (pl.moments keeps its meaning): the
    // kernel's one-workgroup and split forms have the MOM instantiation, its WIDE form does not; and only while the group's
    // planned live count is at least scan_moments_min_live -- below, the launches sit on their latency floor, the records save
    // nothing and the expansion lands on the computing waves' instruction streams (profiles/r08_scan_moments_threshold.txt).
    pl.scan_moments = (h->tr.scan_moments && use_lowrank(h) && use_sym(h) && !in.atm_sets && !in.saving && !pl.order_loop &&
                       pl.transport == TransportKernel::Scan && sh.nzcap <= kRingZones && !in.need_small &&
                       !transport_scan_wide(g) && in.known >= h->tr.scan_moments_min_live) ? 1 : 0;
    return pl;
}

// The transport of the step entry (sosrt_transport), as a plan of its own and deliberately not plan_order's: a step has no live
// count, so the Auto knob never picks the chunk-parallel kernel here, and that kernel runs in its one-workgroup form.
LaunchPlan plan_step_transport(const sosrt_handle* h, const SolveShape& sh) {
    LaunchPlan pl;
    if (!sh.fast) return pl;                 // the general kernel, without attenuation tables
    const bool scan = h->tr.mode == TransportKnob::Scan && h->tr.scan_ok && transport_scan_fits(h->g, sh.nzcap, false);
    pl.transport = scan ? TransportKernel::Scan : (sh.ring_like ? TransportKernel::Ring : TransportKernel::Fast);
    pl.repair = (h->N - 3 > 61 && !sh.ring_mode) ? 1 : 0;
    return pl;
}

// One transport launch of a column group, by name: which columns, which buffers, which order.
struct TransportCall {
    int b0 = 0, nb = 0;                  // the group's first column and count
    const double* tau = nullptr;         // whole-batch pointers (the builder offsets them to the group's first column) ...
    double* In = nullptr;
    double* I = nullptr;
    double* saved = nullptr;             // ... this order's slot of the batch's first column; null: not saved
    size_t saved_stride = 0;
    Conv cv;                             // the group's
    int order = 0;
    bool accumulate = false;             // an order of a solve (else the step entry: In only)
    bool etab = false;                   // the attenuation tables of this tau are built ...
    const int* erep = nullptr;           // ... one per distinct profile ([batch], values are whole-batch column ids); null: one per column
    bool need_small = true;              // some |mu| < 0.01 lane keeps its k_smallmu value
    bool coresident = false;             // another column group runs beside this one
};

// The arguments of that launch with `kernel` (for an order-loop launch, whose transport role is the chunk-parallel kernel: Scan).
// Every condition on a field is stated here, once, in terms of the kernel; launch_transport honours what it is given.
int transport_args(const sosrt_handle* h, const TransportCall& c, const LaunchPlan& pl, const SolveShape& sh, TransportKernel kernel,
                   TransportArgs* out) {
    const bool ring_class = kernel == TransportKernel::Ring || kernel == TransportKernel::Scan;
    const size_t LD = (size_t)h->L * h->D;
    // The contraction of a moment order has written records and NOT the plain rows of Jn: the ring kernel must expand them
    // (plan_order turns the mode on only where it can)
    // (or the chunk-parallel kernel, in its forms that have the MOM instantiation)
    if ((pl.moments && (kernel != TransportKernel::Ring || !c.accumulate || c.saved || sh.nzcap > kRingZones)) ||
        (pl.scan_moments && (kernel != TransportKernel::Scan || pl.order_loop || !c.accumulate || c.saved || sh.nzcap > kRingZones ||
                             transport_scan_wide(h->g))) ||
        (pl.moments && pl.scan_moments))
        return fail(SOSRT_E_STATE, "internal: moment records planned for a transport launch that cannot read them");
    TransportArgs a{};
    a.g = h->g;
    // once the device has reported that no |mu| < 0.01 lane keeps its k_smallmu value, the ring kernel
    // need not stage those rows either
    if (ring_class && !c.need_small) a.g.nsmall = 0;
    a.tau = c.tau + (size_t)c.b0 * h->L; a.Jn = h->fld.d_Jn + (size_t)c.b0 * LD; a.desc = h->cols.d_desc + c.b0;
    a.In = c.In ? c.In + (size_t)c.b0 * LD : nullptr; a.I = c.I ? c.I + (size_t)c.b0 * LD : nullptr;
    a.saved = (c.accumulate && c.saved) ? c.saved + (size_t)c.b0 * c.saved_stride : nullptr; a.saved_col_stride = c.saved_stride;
    a.cv = c.cv; a.order = c.order; a.accumulate = c.accumulate ? 1 : 0;
    a.Etab = c.etab ? h->fld.d_E : nullptr;
    a.erep = (c.etab && c.erep) ? c.erep + c.b0 : nullptr;      // (values are whole-batch column ids; the table base is not offset)
    a.stamps = pl.order_loop ? nullptr : h->tr.d_stamps;         // (an order-loop launch has its own event log)
    // over the live columns only: the grid is then `live` (an order-loop launch finds its live columns itself)
    if (ring_class && c.accumulate && !pl.order_loop && pl.live_cap > 0 && pl.live_cap < c.nb) { a.live = pl.live_cap; a.live_list = h->gemm.d_livelist + c.b0; }
    a.slots = ring_slots_word(c.coresident && h->grp.coresident_slots > 0 ? h->grp.coresident_slots : h->tr.ring_slots, h->tr.ring_debug);
    a.nzcap = sh.nzcap > kRingZones ? sh.nzcap : kRingZones;
    if (kernel == TransportKernel::Scan && (pl.order_loop ? pl.ol_parts : pl.parts) > 1) {
        a.scan_split = 1;
        a.scan_scratch = h->tr.d_scan_scratch + (size_t)c.b0 * transport_scan_scratch_doubles(); a.scan_sync = h->tr.d_scan_sync + 2 * c.b0;
    }
    if (pl.moments || pl.scan_moments) { a.mom = h->tr.d_mom + (size_t)c.b0 * h->L * kMomDoubles; a.lrV = h->phase.d_lrV; a.lr_rank = h->phase.lr_rank; }
    *out = a;
    return 0;
}

// CUs of a device that order-loop launches of this process hold (their workgroups wait for each other, so every one of them must
// be resident: the launches of all handles together never ask for more workgroups than the device has CUs)
std::mutex g_ol_mutex;
int g_ol_held[64];
int ol_acquire(int device, int total, int want, int least) {
    if (device < 0 || device >= 64) return 0;
    std::lock_guard<std::mutex> lk(g_ol_mutex);
    int got = total - g_ol_held[device];
    if (got > want) got = want;
    if (got < least || got <= 0) return 0;
    g_ol_held[device] += got;
    return got;
}
void ol_release(int device, int n) {
    if (device < 0 || device >= 64 || n <= 0) return;
    std::lock_guard<std::mutex> lk(g_ol_mutex);
    g_ol_held[device] -= n;
}


// The plan of one order as the host-only queries ask for it: a batch of `batch` (clear, slab, clear)-like columns with up to `zones`
// zones as sosrt_set_columns and the order loop of sosrt_solve_dev see it -- the column groups, then the plan of an order of the
// first group with `live` columns of it live.  flags: SOSRT_PLAN_*.  assume_sym: a handle without matrices plans for flip-symmetric
// ones, what every phase function of the scattering angle gives.
int plan_query(sosrt_handle* h, int batch, int live, int surface, int zones, int cus, int flags, bool assume_sym, int* groups,
               LaunchPlan* out) {
    if (!h) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (batch < 1 || live < 0 || live > batch) return fail(SOSRT_E_INVALID, "need 0 <= live <= batch, batch >= 1");
    if (zones < 1 || zones > kMaxZones) return fail(SOSRT_E_INVALID, "zones must be in 1..%d", kMaxZones);
    int want = h->grp.want_groups;
    if (want == 0) want = batch > h->grp.split_min ? 2 : 1;
    const int ng = (want >= 2 && batch >= h->grp.split_min && batch >= 2) ? 2 : 1;
    const int nb = ng == 2 ? batch / 2 : batch;
    const int saved_cus = h->cu_count;
    if (cus > 0) h->cu_count = cus;
    const SolveShape sh = solve_shape(h, zones);
    OrderInputs oi;
    oi.nb = nb; oi.known = live < nb ? live : nb; oi.surface = surface;
    oi.simple_zones = zones == 3 || zones == 1;
    oi.cu_share = h->cu_count / ng;
    oi.saving = (flags & SOSRT_PLAN_SAVED_ORDERS) != 0;
    oi.atm_sets = (flags & SOSRT_PLAN_ATM_SETS) != 0 || h->cols.max_atm_used > 0;
    oi.need_small = (flags & SOSRT_PLAN_NEED_SMALLMU) != 0 && h->g.nsmall > 0;
    const bool saved_sym = h->phase.sym_ok;
    if (assume_sym && !h->have_phase) h->phase.sym_ok = true;
    *out = plan_order(h, sh, oi);
    h->phase.sym_ok = saved_sym;
    h->cu_count = saved_cus;
    *groups = ng;
    return 0;
}

}  // namespace

extern "C" {

int sosrt_plan_launch(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int* out) {
    if (!out) return fail(SOSRT_E_INVALID, "null argument");
    int ng = 0;
    LaunchPlan pl;
    if (int e = plan_query(h, batch, live, surface, zones, cus, 0, true, &ng, &pl)) return e;
    out[0] = ng; out[1] = pl.gemm; out[2] = pl.tail_cols; out[3] = (int)pl.transport; out[4] = pl.parts; out[5] = pl.repair;
    out[6] = pl.order_loop; out[7] = pl.ol_parts; out[8] = pl.ol_grid;
    return 0;
}

int sosrt_plan_ring_moments(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int flags, int* on) {
    if (!on) return fail(SOSRT_E_INVALID, "null argument");
    int ng = 0;
    LaunchPlan pl;
    if (int e = plan_query(h, batch, live, surface, zones, cus, flags, false, &ng, &pl)) return e;
    *on = pl.moments;
    return 0;
}

int sosrt_plan_scan_moments(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int flags, int* on) {
    if (!on) return fail(SOSRT_E_INVALID, "null argument");
    int ng = 0;
    LaunchPlan pl;
    if (int e = plan_query(h, batch, live, surface, zones, cus, flags, false, &ng, &pl)) return e;
    *on = pl.scan_moments;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// step level
// ---------------------------------------------------------------------------------------------
// host P0_aer -> device: [B][2N], or [B][p0_zones][2N] when the zone table carries aerosol sets (sosrt_set_aerosol_sets)
static int stage_p0_aer(sosrt_handle* h, int B, const double* P0_aer, hipStream_t s, const double** d_out) {
    *d_out = nullptr;
    if (!P0_aer) return 0;
    if (h->cols.p0_zones == 0) {
        HIPCHK(hipMemcpyAsync(h->fld.d_P0r, P0_aer, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, s));
        *d_out = h->fld.d_P0r;
        return 0;
    }
    const size_t need = (size_t)B * h->cols.p0_zones * h->D;
    if (int e = h->cols.d_P0rz.reserve(need)) return e;
    HIPCHK(hipMemcpyAsync(h->cols.d_P0rz.p, P0_aer, need * sizeof(double), hipMemcpyHostToDevice, s));
    *d_out = h->cols.d_P0rz.p;
    return 0;
}

extern "C" {

int sosrt_first_order(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer,
                      double* I1_out) {
    if (int e = check_ready(h, B, false)) return e;
    if (int e = no_row_weights(h, "sosrt_first_order")) return e;
    if (!tau || !P0_atm || !I1_out) return fail(SOSRT_E_INVALID, "null argument");
    if (h->geom == SOSRT_GEOM_THREE_ZONE && !P0_aer) return fail(SOSRT_E_INVALID, "three-zone geometry needs P0_aer");
    HIPCHK(hipSetDevice(h->device));
    h->resident = false;                     // d_tau is overwritten
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->fld.d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->fld.d_P0a, P0_atm, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const double* d_p0r = nullptr;
    if (int e = stage_p0_aer(h, B, P0_aer, h->stream, &d_p0r)) return e;
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->fld.d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr);
    prof_begin(h, SOSRT_K_FIRST);
    if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
        launch_first_order_readme(h->stream, h->g, h->grid.d_w, B, h->fld.d_tau, h->fld.d_P0a, d_p0r, h->cols.d_desc, h->fld.d_InA,
                                  nullptr, nullptr, 0, make_conv(h, 0), 0);
    else
        launch_first_order(h->stream, h->g, B, h->fld.d_tau, h->fld.d_P0a, d_p0r, h->cols.d_desc, h->fld.d_InA, nullptr,
                           nullptr, 0, make_conv(h, 0), 0, h->cols.p0_zones);
    prof_end(h, SOSRT_K_FIRST);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(I1_out, h->fld.d_InA, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int sosrt_source(sosrt_t* h, int B, const double* In_1, double* Jn_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!In_1 || !Jn_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (int e = ensure_w32(h)) return e;
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->fld.d_InA, In_1, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // the row coefficients depend on tau only through the zone bounds; prepare needs a tau buffer
    // for the a4b buckets, which the source function does not use
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->fld.d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr);
    apply_row_weights(h, h->stream, B);
    run_source(h, h->fld.d_InA, h->fld.d_Jn, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Jn_out, h->fld.d_Jn, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int sosrt_transport(sosrt_t* h, int B, const double* tau, const double* Jn, double* In_out, int* status_out) {
    if (int e = check_ready(h, B, false)) return e;
    if (!tau || !Jn || !In_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    h->resident = false;                     // d_tau is overwritten
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->fld.d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->fld.d_Jn, Jn, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->fld.d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr);
    HIPCHK(hipMemsetAsync(h->fld.d_InB, 0, n * sizeof(double), h->stream));
    prof_begin(h, SOSRT_K_SMALLMU);
    launch_smallmu(h->stream, h->g, B, h->fld.d_tau, h->fld.d_Jn, h->fld.d_InB, h->cols.d_desc, nullptr);
    prof_end(h, SOSRT_K_SMALLMU);
    prof_begin(h, SOSRT_K_TRANSPORT);
    const SolveShape sh = solve_shape(h, h->cols.max_nz);
    const LaunchPlan pl = plan_step_transport(h, sh);
    TransportCall c;
    c.nb = B; c.tau = h->fld.d_tau; c.In = h->fld.d_InB; c.cv = make_conv(h, 0);
    c.etab = pl.transport != TransportKernel::General;           // (tables for every column: no erep)
    if (c.etab) {
        launch_attenuation(h->stream, h->g, B, h->fld.d_tau, h->fld.d_E, nullptr);
        HIPCHK(hipMemsetAsync(h->fld.d_redo, 0, B * sizeof(int), h->stream));
    }
    TransportArgs ta;
    if (int e = transport_args(h, c, pl, sh, pl.transport, &ta)) return e;
    launch_transport(h->stream, pl.transport, B, ta);
    if (pl.repair) {
        if (int e = transport_args(h, c, pl, sh, TransportKernel::Repair, &ta)) return e;
        launch_transport(h->stream, TransportKernel::Repair, B, ta);
    }
    prof_end(h, SOSRT_K_TRANSPORT);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(In_out, h->fld.d_InB, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status_out) HIPCHK(hipMemcpyAsync(status_out, h->fld.d_status, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// column level
// ---------------------------------------------------------------------------------------------
// spec:309 with In = ones when the first order is supplied by the caller
__global__ void k_init_from_I1(Grid g, const double* __restrict__ I1, double* __restrict__ In1, double* __restrict__ I,
                               double* __restrict__ saved, size_t saved_col_stride, Conv cv) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t n = (size_t)g.L * g.D;
    const double* src = I1 + (size_t)b * n;
    for (size_t i = tid; i < n; i += blockDim.x) {
        const double v = src[i];
        In1[(size_t)b * n + i] = v;
        I[(size_t)b * n + i] = v;
        if (saved) saved[(size_t)b * saved_col_stride + i] = v;
    }
    if (tid == 0) {
        // the reference's test with In = ones: python max over the rows, in order
        double a = 1.0 / src[g.N];
        for (int m = g.N + 1; m < g.D; ++m) { const double x = 1.0 / src[m]; if (x > a) a = x; }
        const double* last = src + (size_t)(g.L - 1) * g.D;
        double bb = 1.0 / last[0];
        for (int m = 1; m < g.N; ++m) { const double x = 1.0 / last[m]; if (x > bb) bb = x; }
        const double r = (bb > a) ? bb : a;
        cv.ratio[b] = r; cv.norders[b] = 1; cv.status[b] = SOSRT_COL_OK;
        const int go = conv_go(cv, b, 1, r) ? 1 : 0;
        cv.active[b] = go;
        if (go) atomicAdd(cv.nactive, 1);
    }
}

namespace {

struct GroupState {                      // a column group's place in the order loop
    int b0 = 0, nb = 0, n = 1, known = 0;
    bool done = false, started = false;
    bool ol_pending = false, ol_off = false;             // an order-loop launch is running; one was refused: no more in this solve
    int ol_tag = 0;
    unsigned ol_polls = 0;
    std::chrono::steady_clock::time_point ol_t0;         // when the polls of the running launch first looked at the clock
    double *In_1 = nullptr, *In = nullptr;
    Conv cv;
};
enum { kPollWaiting, kPollFinished, kPollRefused };      // poll_order_loop (errors are negative)

// One sosrt_solve_dev: the caller's arguments, what the solve fixes for all its orders, and the state of its column groups.
// The destructor is the clean-up of every early return: the success path leaves it nothing to do (finish()).
struct SolveRun {
    sosrt_handle* const h;
    const int B;
    const double *d_tau, *d_P0_atm, *d_P0_aer;
    const double tol;
    const double* d_I1_in;
    double *d_I_out, *d_I_saved_out;
    hipStream_t s = h->stream;
    const size_t LD = (size_t)h->L * h->D, saved_stride = (size_t)h->saved_slots * LD;
    const int NG = h->grp.ngroups;
    SolveShape shape;
    int small_tag = 0, tagbase = 0;
    bool small_published = false, forked = false, used_order_loop = false;
    GroupState gs[sosrt_handle::kMaxGroups];
    int ol_held[sosrt_handle::kMaxGroups] = {0, 0};      // CUs this solve's order-loop launches hold (ol_acquire)
    int live_groups = 0, n_max = 1;

    // an error return after the fork still joins the internal stream back onto the caller's
    ~SolveRun() {
        if (forked && hipEventRecord(h->grp.ev_join, h->grp.stream2) == hipSuccess) (void)hipStreamWaitEvent(s, h->grp.ev_join, 0);
        for (int k = 0; k < NG; ++k)
            if (ol_held[k]) {                                 // (a launch still running keeps its CUs until its stream has drained)
                (void)hipStreamSynchronize(group_stream(h, k));
                ol_release(h->device, ol_held[k]);
            }
    }
    void retire(int k) { gs[k].done = true; --live_groups; }
    double* saved_of(int k) const { return d_I_saved_out ? d_I_saved_out + (size_t)gs[k].b0 * saved_stride : nullptr; }

    // per-sweep setup on the caller's stream: zone tables, shared attenuation tables, combined slab matrices
    int prepare() {
        const Grid& g = h->g;
        prof_break(h);
        // this solve's counters were zeroed by the previous solve's first kernel (or at sosrt_create); its own first kernel zeroes
        // the other set, clears the redo flags and hashes the optical-depth profiles -- one launch instead of four
        h->fld.nactive_set ^= 1;
        h->fld.d_nactive = h->fld.d_nactive_sets + h->fld.nactive_set * (sosrt_handle::kMaxGroups + 1);
        SolveSetup su;
        su.zero_next = h->fld.d_nactive_sets + (h->fld.nactive_set ^ 1) * (sosrt_handle::kMaxGroups + 1);
        su.n_zero = sosrt_handle::kMaxGroups + 1;
        su.redo = h->fld.d_redo;
        su.hash = h->fld.d_tauhash;
        su.scan_sync = h->tr.d_scan_sync;
        launch_prepare(s, g, B, h->geom, h->surface, scalars_of(h), d_tau, h->cols.d_desc, h->cols.d_rca, h->cols.d_rcr,
                       h->fld.d_nactive + sosrt_handle::kMaxGroups, su);
        apply_row_weights(h, s, B);
        h->fld.need_small = true;
        small_tag = ((++h->fld.pub_seq) & 0x3fffffff) | 0x40000000;       // never equals an order tag
        shape = solve_shape(h, h->cols.max_nz);
        if (h->tr.use_etab || shape.fast) {
            // one attenuation table per distinct optical-depth profile
            launch_tau_groups(s, g, B, d_tau, h->fld.d_tauhash, h->fld.d_erep, h->fld.d_nactive + sosrt_handle::kMaxGroups,
                              h->fld.h_pub + 8 * sosrt_handle::kMaxGroups, small_tag);
            launch_attenuation(s, g, B, d_tau, h->fld.d_E, h->fld.d_erep);
            small_published = true;
        }
        if (int e = ensure_matrices(h, s)) return e;
        h->ol.launches = 0; h->ol.refused = 0;
        h->tr.moment_orders = 0; h->tr.scan_moment_orders = 0; h->tr.orders = 0;
        for (bool& u : h->ol.group_used) u = false;
        tagbase = ((++h->fld.pub_seq) & 0x3fff) << 16;      // tag of order n = tagbase + n
        live_groups = NG;
        for (int k = 0; k < NG; ++k) {
            GroupState& q = gs[k];
            q.b0 = h->grp.gb[k]; q.nb = h->grp.gb[k + 1] - h->grp.gb[k]; q.known = q.nb;
            q.In_1 = h->fld.d_InA; q.In = h->fld.d_InB;                   // whole-batch buffers; every kernel gets its group's offset
            // The coded first order writes I = I1 only: the second order's contraction reads its operand there (the same numbers),
            // and the first order is bound by its stores (one 8 L D array instead of two: 91 -> 50 us for 512 columns)
            if (!d_I1_in && h->first_order_mode != SOSRT_FIRST_ORDER_README) q.In_1 = d_I_out;
            q.cv = make_conv(h, tol);
            q.cv.active += q.b0; q.cv.norders += q.b0; q.cv.status += q.b0; q.cv.ratio += q.b0; q.cv.redo += q.b0;
            q.cv.nactive = h->fld.d_nactive + k;
            if (h->d_targets) q.cv.target = h->d_targets + q.b0;
        }
        return 0;
    }

    // the first order of a group: the caller's, the README's, or the coded one
    void start_group(int k) {
        GroupState& q = gs[k];
        const Grid& g = h->g;
        q.started = true;
        hipStream_t sg = group_stream(h, k);
        const size_t fo = (size_t)q.b0 * LD;
        prof_begin(h, SOSRT_K_FIRST, k);
        if (d_I1_in)
            hipLaunchKernelGGL(k_init_from_I1, dim3(q.nb), dim3(256), 0, sg, g, d_I1_in + fo, q.In_1 + fo, d_I_out + fo, saved_of(k),
                               saved_stride, q.cv);
        else if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            launch_first_order_readme(sg, g, h->grid.d_w, q.nb, d_tau + (size_t)q.b0 * h->L, d_P0_atm + (size_t)q.b0 * g.D,
                                      d_P0_aer ? d_P0_aer + (size_t)q.b0 * g.D : nullptr, h->cols.d_desc + q.b0, q.In_1 + fo,
                                      d_I_out + fo, saved_of(k), saved_stride, q.cv, 1);
        else
            launch_first_order(sg, g, q.nb, d_tau + (size_t)q.b0 * h->L, d_P0_atm + (size_t)q.b0 * g.D,
                               d_P0_aer ? d_P0_aer + (size_t)q.b0 * g.D * (h->cols.p0_zones > 0 ? h->cols.p0_zones : 1) : nullptr,
                               h->cols.d_desc + q.b0, d_I_out + fo, nullptr, saved_of(k), saved_stride, q.cv, 1, h->cols.p0_zones);
        prof_end(h, SOSRT_K_FIRST, k);
    }

    // The second column group runs on the internal stream from here on.  The fork comes BEHIND the first group's first order:
    // the two calls cost the host ~25 us, which the GPU -- 20 us of setup kernels ahead of the host at this point -- would
    // otherwise wait for; the second group starts half a cycle after the first anyway.
    int fork() {
        if (NG < 2) return 0;
        HIPCHK(hipEventRecord(h->grp.ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->grp.stream2, h->grp.ev_fork, 0));
        forked = true;
        return 0;
    }

    // k_prepare's verdict on k_smallmu, published by the second kernel of the solve: by now it has long run (no stream is asked)
    int await_small() {
        if (!small_published || h->g.nsmall == 0) return 0;
        volatile int* slot = h->fld.h_pub + 8 * sosrt_handle::kMaxGroups;
        if (int e = await_tag(h, slot, small_tag, -1)) return e;
        h->fld.need_small = slot[0] != 0;
        return 0;
    }

    // the group's remaining orders run in one launch; its last workgroup reports {state, tag} to pinned memory
    int poll_order_loop(int k) {
        GroupState& q = gs[k];
        volatile int* dw = h->ol.h_done + 2 * k;
        if (__atomic_load_n(&dw[1], __ATOMIC_ACQUIRE) != q.ol_tag) {
            if ((++q.ol_polls & 0x3fff) != 0) return kPollWaiting;
            const hipError_t qe = hipStreamQuery(group_stream(h, k));
            if (qe != hipSuccess && qe != hipErrorNotReady) return fail(SOSRT_E_HIP, "order loop: %s", hipGetErrorString(qe));
            if (qe == hipSuccess && __atomic_load_n(&dw[1], __ATOMIC_ACQUIRE) != q.ol_tag)
                return fail(SOSRT_E_HIP, "order loop: the order-loop launch ended without reporting");
            const auto now = std::chrono::steady_clock::now();
            if (q.ol_polls == 0x4000) q.ol_t0 = now;
            if (now - q.ol_t0 > std::chrono::seconds(120)) return fail(SOSRT_E_HIP, "order loop: no progress for 120 s");
            return kPollWaiting;
        }
        const int state = dw[0];
        q.ol_pending = false;
        ol_release(h->device, ol_held[k]);
        ol_held[k] = 0;
#ifdef SOSRT_OL_STAMPS
        if (h->ol.d_log && getenv("SOSRT_OL_LOG")) {
            std::vector<unsigned long long> lg(65001);
            (void)hipStreamSynchronize(group_stream(h, k));
            (void)hipMemcpy(lg.data(), h->ol.d_log, lg.size() * 8, hipMemcpyDeviceToHost);
            if (FILE* f = fopen(getenv("SOSRT_OL_LOG"), "a")) {
                fprintf(f, "# launch columns<=%d order0=%d events=%llu\n", q.known, q.n + 1, lg[0]);
                for (unsigned long long i = 0; i < lg[0] && i < 65000; ++i)
                    fprintf(f, "%llu %llu %llu %llu\n", lg[1 + i] >> 48, (lg[1 + i] >> 40) & 0xff, (lg[1 + i] >> 32) & 0xff, lg[1 + i] & 0xffffffffull);
                fclose(f);
            }
        }
#endif
        if (state == kOlReady) { retire(k); h->ol.group_used[k] = true; return kPollFinished; }
        if (state == kOlAborted) {
            // never expected: say where the launch stood (the words of the launch, first columns)
            std::vector<int> w(order_loop_sync_ints(q.known < 6 ? q.known : 6));
            (void)hipStreamSynchronize(group_stream(h, k));
            (void)hipMemcpy(w.data(), h->ol.d_sync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols), w.size() * sizeof(int), hipMemcpyDeviceToHost);
            std::string cols;
            for (int c = 0; c < (q.known < 6 ? q.known : 6); ++c) {
                char buf[96];
                const int* cs = w.data() + kOlCols + c * kOlColStride;
                snprintf(buf, sizeof buf, " [%d: orders %d stop %d tiles %d]", c, cs[kOlOrdDone], cs[kOlColStop], cs[kOlJnDone]);
                cols += buf;
            }
            return fail(SOSRT_E_HIP, "order loop: a workgroup of the order-loop launch gave up waiting (arrived %d, left %d, order %d on, %d columns:%s)",
                        w[kOlArrive], w[kOlLeft], q.n + 1, q.known, cols.c_str());
        }
        // not resident (another process's kernels held CUs): nothing was touched; the one-order kernels take over
        q.ol_off = true;
        ++h->ol.refused;
        return kPollRefused;
    }

    OrderInputs order_inputs(int k) const {
        const GroupState& q = gs[k];
        OrderInputs oi;
        oi.nb = q.nb; oi.known = q.known; oi.surface = h->surface;
        oi.simple_zones = h->cols.simple_zones; oi.slabs_mixed = h->cols.nslab == 0 || h->cols.mix_groups > 0;
        oi.need_small = h->g.nsmall > 0 && h->fld.need_small; oi.saving = d_I_saved_out != nullptr;
        oi.orders_left = h->order_budget - q.n;
        oi.atm_sets = h->cols.max_atm_used > 0;
        oi.row_weights = h->cols.rw_on;
        oi.cu_share = (q.ol_off || h->d_targets || h->cols.max_atm_used > 0) ? 0 : h->cu_count / NG;   // (no order-loop launch with order targets, or atmosphere sets)
        return oi;
    }

    // this and every later order of the group in one launch
    int launch_order_loop(int k, const LaunchPlan& pl) {
        GroupState& q = gs[k];
        const Grid& g = h->g;
        hipStream_t sg = group_stream(h, k);
        const size_t fo = (size_t)q.b0 * LD;
        OrderLoopArgs oa;
        TransportCall c = transport_call(k);
        c.I = d_I_out; c.etab = true;
        if (int e = transport_args(h, c, pl, shape, TransportKernel::Scan, &oa.t)) return e;
        oa.gm = gemm_args(h, true);
        oa.gm.A = nullptr; oa.gm.C = h->fld.d_Jn;
        oa.in0 = q.In_1;
        oa.gbufP = q.In;
        oa.gbufQ = (q.In_1 == d_I_out) ? h->fld.d_InA : q.In_1;   // (after the second order: the buffer the first order left unused)
        oa.bufP = oa.gbufP + fo; oa.bufQ = oa.gbufQ + fo;
        oa.order0 = q.n + 1; oa.kmax = h->order_budget - q.n;
        oa.B = q.nb; oa.col0 = q.b0;
        oa.fixcap = (int)(0.06 * g.N) + 1;
        oa.sync = h->ol.d_sync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols);
        oa.host_done = h->ol.h_done + 2 * k;
        oa.tag = q.ol_tag = ((++h->fld.pub_seq) & 0x3fffffff) | 0x40000000;
#ifdef SOSRT_OL_STAMPS   // diagnostic builds: SOSRT_OL_LOG=<file> receives the launch's event log (tools/ol_timeline.py)
        if (getenv("SOSRT_OL_LOG")) {
            if (!h->ol.d_log) { if (int e = dalloc(&h->ol.d_log, 65001)) return e; }
            HIPCHK(hipMemsetAsync(h->ol.d_log, 0, 8, sg));
            oa.log = h->ol.d_log;
        }
#endif
        prof_break(h);
        HIPCHK(hipMemsetAsync(oa.sync, 0, order_loop_sync_ints(q.known) * sizeof(int), sg));
        prof_begin(h, SOSRT_K_ORDER_LOOP, k);
        const hipError_t le = sosrt::launch_order_loop(sg, pl.ol_grid, pl.ol_parts > 1, oa);
        prof_end(h, SOSRT_K_ORDER_LOOP, k);
        if (le != hipSuccess) return fail(SOSRT_E_HIP, "order-loop launch failed: %s", hipGetErrorString(le));
        q.ol_pending = true;
        q.ol_polls = 0;
        used_order_loop = true;
        ++h->ol.launches;
        return 0;
    }

    // what every transport launch of a group's orders has in common (the caller adds its buffers and the order)
    TransportCall transport_call(int k) const {
        const GroupState& q = gs[k];
        TransportCall c;
        c.b0 = q.b0; c.nb = q.nb; c.tau = d_tau; c.cv = q.cv;
        c.accumulate = true; c.erep = h->fld.d_erep;
        c.need_small = h->fld.need_small; c.coresident = NG > 1;
        return c;
    }

    // one order of a group as two (or three) launches: source function, small-mu lanes, transport
    int run_order(int k, const LaunchPlan& pl) {
        GroupState& q = gs[k];
        const Grid& g = h->g;
        hipStream_t sg = group_stream(h, k);
        const size_t fo = (size_t)q.b0 * LD;
        const double* tau_g = d_tau + (size_t)q.b0 * h->L;
        const int n = ++q.n;
        n_max = n > n_max ? n : n_max;
        // this launch also publishes the group's live count after order n-1
        SourceOpts so;
        so.tail_cols = pl.tail_cols; so.pub_tag = tagbase + n - 1; so.grp = k; so.all_live = q.known == q.nb;
        so.regs_tile = pl.gemm == SOSRT_PLAN_GEMM_LIVE16_REGS; so.dense_live_cap = pl.tail_cols > 0 ? 0 : pl.live_cap;
        so.moments = pl.moments != 0 || pl.scan_moments != 0;
        run_source(h, q.In_1, h->fld.d_Jn, h->fld.d_active, so);
        if (g.nsmall > 0 && h->fld.need_small) {      // skipped once the device has reported that every such lane is rewritten anyway
            prof_begin(h, SOSRT_K_SMALLMU, k);
            launch_smallmu(sg, g, q.nb, tau_g, h->fld.d_Jn + fo, q.In + fo, h->cols.d_desc + q.b0, q.cv.active);
            prof_end(h, SOSRT_K_SMALLMU, k);
        }
        prof_begin(h, SOSRT_K_TRANSPORT, k);
        TransportCall c = transport_call(k);
        c.In = q.In; c.I = d_I_out; c.order = n;
        if (d_I_saved_out && n <= h->saved_slots) { c.saved = d_I_saved_out + (size_t)(n - 1) * LD; c.saved_stride = saved_stride; }
        c.etab = pl.transport != TransportKernel::General || h->tr.use_etab;
        TransportArgs ta;
        if (int e = transport_args(h, c, pl, shape, pl.transport, &ta)) return e;
        launch_transport(sg, pl.transport, q.nb, ta);
        if (pl.repair) {
            // register-streaming kernel: a search that leaves wave 0 is redone by the general kernel (flag cv.redo); the ring
            // kernel redoes it itself
            if (int e = transport_args(h, c, pl, shape, TransportKernel::Repair, &ta)) return e;
            launch_transport(sg, TransportKernel::Repair, q.nb, ta);
        }
        prof_end(h, SOSRT_K_TRANSPORT, k);
        ++h->tr.orders;
        if (pl.moments) ++h->tr.moment_orders;
        if (pl.scan_moments) ++h->tr.scan_moment_orders;
        if (q.In_1 == d_I_out) { q.In_1 = q.In; q.In = h->fld.d_InA; }      // (after the second order: the buffer the first order left unused)
        else { double* tmp = q.In_1; q.In_1 = q.In; q.In = tmp; }
        return 0;
    }

    // back onto the caller's stream; after the join the destructor has nothing left to do
    int finish(int* d_n_orders_out, int* d_status_out) {
        if (NG > 1) {
            HIPCHK(hipEventRecord(h->grp.ev_join, h->grp.stream2));
            HIPCHK(hipStreamWaitEvent(s, h->grp.ev_join, 0));
            forked = false;
        }
        prof_break(h);
        launch_finalize(s, B, make_conv(h, tol), h->order_budget, d_n_orders_out, d_status_out);
        HIPCHK(hipGetLastError());
        h->fld.last_max_orders = used_order_loop ? -1 : n_max;      // (orders run inside an order-loop launch: read back with the counts)
        h->fld.last_sum_orders = -1;
        return 0;
    }
};

// norders [B] -> the handle's (max, sum of orders beyond the first) of the last solve
void record_order_stats(sosrt_handle* h, const std::vector<int>& no) {
    long long sum = 0;
    int mx = 1;
    for (int v : no) { sum += v - 1; mx = v > mx ? v : mx; }
    h->fld.last_sum_orders = sum;
    if (h->fld.last_max_orders < 0) h->fld.last_max_orders = mx;
}

}  // namespace

extern "C" {

int sosrt_solve_dev(sosrt_t* h, int B, const double* d_tau, const double* d_P0_atm, const double* d_P0_aer, double tol,
                    const double* d_I1_in, double* d_I_out, double* d_I_saved_out, int* d_n_orders_out,
                    int* d_status_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!d_tau || !d_I_out) return fail(SOSRT_E_INVALID, "null argument");
    if (!d_I1_in && !d_P0_atm) return fail(SOSRT_E_INVALID, "P0_atm is required unless I1 is supplied");
    if (int e = d_I1_in ? 0 : no_row_weights(h, "sosrt_solve_dev without a caller's first order")) return e;
    if (!d_I1_in && h->geom == SOSRT_GEOM_THREE_ZONE && !d_P0_aer) return fail(SOSRT_E_INVALID, "three-zone geometry needs P0_aer");
    if (h->max_orders >= 65536) return fail(SOSRT_E_INVALID, "max_orders must be < 65536");
    HIPCHK(hipSetDevice(h->device));
    if (int e = ensure_w32(h)) return e;
    SolveRun r{h, B, d_tau, d_P0_atm, d_P0_aer, tol, d_I1_in, d_I_out, d_I_saved_out};
    if (int e = r.prepare()) return e;
    r.start_group(0);
    if (int e = r.fork()) return e;
    if (int e = r.await_small()) return e;
    // Order loop (spec:309-458), per column group.  Converged columns are masked on the device (every kernel of an
    // order returns at once for them).  r_k = number of live columns of the group after order k is written to a
    // pinned slot by the first workgroup of order k+1's source-function launch; before launching order k+1 the
    // host checks r_{k-1}, which is there as soon as order k has started, so a stream never drains inside the loop
    // and at most one launch group runs on a fully converged group.  With two groups the host feeds them in turn:
    // each stream always holds the next order of its group, and the GPU overlaps the contraction of one group
    // (MFMA-bound) with the transport of the other (HBM-bound).
    while (r.live_groups > 0) {
        bool progressed = false;
        for (int k = 0; k < r.NG; ++k) {
            GroupState& q = r.gs[k];
            if (q.done) continue;
            if (q.ol_pending) {
                const int st = r.poll_order_loop(k);
                if (st < 0) return st;
                if (st == kPollWaiting) continue;
                progressed = true;
                if (st == kPollFinished) continue;
            }
            if (!q.started) {
                // Staggered start: the dense orders of this group (they fill the GPU) run beside the long tail of the
                // previous one (a few workgroups per order, latency-bound), instead of both being dense, then both in
                // their tails, together.
                const GroupState& p = r.gs[k - 1];
                if (!(p.done || (p.n >= 2 && p.known <= h->grp.stagger * p.nb))) continue;
                r.start_group(k);
            }
            progressed = true;
            if (q.n >= h->order_budget) { r.retire(k); continue; }
            if (q.n >= 2) {
                const int live = wait_published(h, k, r.tagbase + q.n - 1);
                if (live < 0) return live;
                if (live == 0) { r.retire(k); continue; }
                q.known = live;
            }
            // ---- the plan of this order (plan_order: one place for the whole policy) ----
            OrderInputs oi = r.order_inputs(k);
            LaunchPlan pl = plan_order(h, r.shape, oi);
            if (pl.order_loop) {
                // its workgroups wait for each other: they must all fit the CUs no other order-loop launch of this process holds
                const int got = ol_acquire(h->device, h->cu_count, pl.ol_grid, (int)(pl.ol_parts * q.known / h->ol.frac));
                if (got == 0) { oi.cu_share = 0; pl = plan_order(h, r.shape, oi); }
                else { pl.ol_grid = got; r.ol_held[k] = got; }
            }
            // (mode 2, for the tests of the refusal path: a grid of twice the CUs can never be resident -- the handshake times out,
            // nothing has been touched, and the order is run as two launches)
            if (pl.order_loop && h->ol.mode == 2) pl.ol_grid = 2 * h->cu_count;
            if (pl.order_loop) {
                if (int e = r.launch_order_loop(k, pl)) return e;
            } else {
                if (int e = r.run_order(k, pl)) return e;
            }
        }
        if (!progressed) __builtin_ia32_pause();      // (every live group is inside its order-loop launch)
    }
    return r.finish(d_n_orders_out, d_status_out);
}

int sosrt_solve(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer, double tol,
                const double* I1_in, double* I_out, double* I_saved_out, int* n_orders_out, int* status_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!tau) return fail(SOSRT_E_INVALID, "null argument");
    if (int e = I1_in ? 0 : no_row_weights(h, "sosrt_solve without a caller's first order")) return e;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->resident = false;
    const size_t LD = (size_t)h->L * h->D, n = (size_t)B * LD;
    HIPCHK(hipMemcpyAsync(h->fld.d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, s));
    if (P0_atm) HIPCHK(hipMemcpyAsync(h->fld.d_P0a, P0_atm, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, s));
    const double* d_p0r = nullptr;
    if (int e = stage_p0_aer(h, B, P0_aer, s, &d_p0r)) return e;
    double* d_I1 = nullptr;
    double* d_saved = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        if (I1_in) {
            if (int e = dalloc(&d_I1, n)) return e;
            HIPCHK(hipMemcpyAsync(d_I1, I1_in, n * sizeof(double), hipMemcpyHostToDevice, s));
        }
        if (I_saved_out) {
            if (int e = dalloc(&d_saved, (size_t)B * h->saved_slots * LD)) return e;
            HIPCHK(hipMemsetAsync(d_saved, 0, (size_t)B * h->saved_slots * LD * sizeof(double), s));
        }
        if (int e = sosrt_solve_dev(h, B, h->fld.d_tau, P0_atm ? h->fld.d_P0a : nullptr, d_p0r, tol, d_I1,
                                    h->fld.d_I, d_saved, nullptr, nullptr))
            return e;
        if (I_out) HIPCHK(hipMemcpyAsync(I_out, h->fld.d_I, n * sizeof(double), hipMemcpyDeviceToHost, s));
        if (I_saved_out)
            HIPCHK(hipMemcpyAsync(I_saved_out, d_saved, (size_t)B * h->saved_slots * LD * sizeof(double), hipMemcpyDeviceToHost, s));
        std::vector<int> no(B);
        HIPCHK(hipMemcpyAsync(no.data(), h->fld.d_norders, B * sizeof(int), hipMemcpyDeviceToHost, s));
        if (status_out) HIPCHK(hipMemcpyAsync(status_out, h->fld.d_status, B * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (n_orders_out) std::copy(no.begin(), no.end(), n_orders_out);
        record_order_stats(h, no);
        h->resident = true; h->resident_B = B;
        return 0;
    };
    rc = body();
    if (d_I1) hipFree(d_I1);
    if (d_saved) hipFree(d_saved);
    return rc;
}

int sosrt_last_solve_stats(sosrt_t* h, int* max_orders_run, long long* sum_orders) {
    if (int e = need_gpu(h)) return e;
    if ((h->fld.last_sum_orders < 0 || h->fld.last_max_orders < 0) && h->B > 0) {
        std::vector<int> no(h->B);
        HIPCHK(hipMemcpyAsync(no.data(), h->fld.d_norders, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        record_order_stats(h, no);
    }
    if (max_orders_run) *max_orders_run = h->fld.last_max_orders;
    if (sum_orders) *sum_orders = h->fld.last_sum_orders;
    return 0;
}

}  // extern "C"
