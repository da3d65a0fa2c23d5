// The handle behind the C ABI (include/sosrt.h) and what every host file of the library needs with it: error text, device
// allocation, HIP-event profiling, the state checks of the entry points.  Private to csrc: api.hip (life cycle, setters,
// read-backs), api_phase.hip (phase matrices), api_columns.hip (columns, zones, mix groups), solve.hip (launch plan, order
// loop), api_phasefn.hip (phase functions, Mie, azimuth modes), api_view.hip (view radiance).  The fields are grouped by the file that owns them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sosrt.h"
#include "comm.hpp"
#include "kernels.hpp"
#include "phasefn.hpp"
#include "plan.hpp"
#include "profile.hpp"

namespace sosrt {

int fail(int code, const char* fmt, ...);       // sets sosrt_last_error() (api.hip) and returns code

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return fail(SOSRT_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                           \
    } while (0)

constexpr int kNPhi = 25;                // phase:81  nb_phi

template <class T>
int dalloc(T** p, size_t n) {
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(SOSRT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    return 0;
}

// Grow-only buffer of the device (or, PINNED, of the host): reserve(n) keeps it while n elements fit, else frees it and allocates
// anew -- the contents are lost, and the error text is set on failure.  (The stream may still read the old buffer: hipFree
// synchronises.)
template <class T, bool PINNED = false>
struct GrowBuf {
    T* p = nullptr;
    size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        if (PINNED) HIPCHK(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
        else if (int e = dalloc(&p, n)) return e;
        cap = n;
        return 0;
    }
    void release() {
        if (p) PINNED ? (void)hipHostFree(p) : (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    void swap(GrowBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};

// HIP-event timing of launch groups.  An interval is a pair of events of the pool; when one bracket
// closes and the next opens with nothing enqueued in between (the order loop: contraction, transport,
// contraction, ...), the closing event is the next opening one, which halves the markers in the stream.
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;          // pool
    std::vector<int> kind, first, last;  // per interval: kernel family, opening / closing event
    size_t used = 0, nint = 0;           // events / intervals used
    int open = -1;                       // opening event of the current bracket
    int adjacent = -1;                   // closing event of the previous bracket, if nothing was enqueued since
};

// SOSRT_TRANSPORT, in ascending order of what it allows (solve_shape compares with >=).  General: the general kernel; Fast: the
// wave-independent register-streaming kernel (+ repair); Ring: the LDS-ring kernel; Auto (default): the ring kernel for
// launches with many live columns (HBM-bound) and the chunk-parallel kernel (transport_scan.hip) for launches with at
// most scan_cols (latency-bound); Scan: the chunk-parallel kernel always.  The ring and the chunk-parallel kernel share
// their arithmetic (chunk-local recurrence), so the choice follows the live count without touching a column's bits.
enum class TransportKnob { General = 0, Fast = 1, Ring = 2, Auto = 3, Scan = 4 };
}  // namespace sosrt

struct sosrt_handle {
    int device = -1, L = 0, N = 0, D = 0, max_batch = 0, max_orders = 0;
    int order_budget = 0;                // orders a solve runs at most (sosrt_set_order_budget; <= max_orders, the default)
    int saved_slots = 0;                 // orders per column in I_saved_out (sosrt_set_saved_orders; default max_orders)
    bool gpu = false;
    hipStream_t own_stream = nullptr, stream = nullptr;
    sosrt::Plan plan;
    bool have_grid = false, have_phase = false, have_aer = false, have_cols = false;
    int B = 0, geom = 0, surface = 0;
    sosrt::Grid g{};
    int first_order_mode = SOSRT_FIRST_ORDER_CODED;   // sosrt_set_first_order
    const int* d_targets = nullptr;      // sosrt_set_order_targets (caller's device array [B]); null: the spec:309 test
    bool resident = false;               // d_tau / d_I hold the inputs / result of the last sosrt_solve (of resident_B columns)
    int resident_B = 0;
    int cu_count = 0;
    static constexpr int kMaxGroups = 2;
    sosrt::Prof prof[kMaxGroups];        // per column group (= per stream)

    // Column groups of the order loop: a large batch is solved as two halves, the second on an internal stream, so
    // that the MFMA-bound contraction of one half overlaps the HBM-bound transport of the other (SOSRT_GROUPS)
    struct Groups {
        hipStream_t stream2 = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        // (round 4, alternating runs on one box, shards of the EVA sweep: 32 columns 1.54 -> 1.48 ms, 64 columns 1.71 -> 1.66, 128 columns
        // 2.06 -> 1.96, 256 columns 2.98 -> 2.82 -- round 3 had only measured 256 and up with the capped contraction; tools/ab_small_groups.py)
        int ngroups = 1, want_groups = 0, split_min = 48;       // want_groups 0: two groups above split_min columns (set_columns)
        int split_at = -1;                   // SOSRT_GROUP_SPLIT: first column of the second group (default: the middle)
        int prio2 = 0;                       // SOSRT_GROUP_PRIO: the internal stream is created with the highest priority
        // Round 2 capped the contraction at two workgroups per CU with LDS padding (27 008 bytes: 27 656 static + this > 1/3 of 160 KiB)
        // and ran the ring two slots deep, so that a transport workgroup of the other group fits beside them on every CU.  With round 3's
        // kernels the uncapped contraction and a three-slot ring are faster under two groups (alternating runs: 512 columns 4.81 -> 4.75 ms,
        // 1024 columns 8.45 -> 8.15, 384 columns unchanged): the groups share the GPU CU by CU rather than inside a CU.
        int coresident_pad = 0;             // SOSRT_GEMM_PAD_LDS (diagnostic builds)
        int coresident_slots = 3;           // SOSRT_GROUP_RING_SLOTS: ring depth of the transport under two groups
        double stagger = 1.0;                // a group starts when the previous one is down to this fraction of live columns (SOSRT_STAGGER; 1: together)
        int gb[kMaxGroups + 1] = {0, 0, 0};                    // column range of group g: [gb[g], gb[g+1])
        int main_off[kMaxGroups + 1] = {0, 0, 0};              // its plain rows in d_mainrows
        int slab_off[kMaxGroups + 1] = {0, 0, 0};              // its slab rows in d_slabrows (tile-aligned when grouped by coefficient pair)
    } grp;

    struct GridDev {                     // device: the grid (sosrt_set_grid)
        double *d_mu = nullptr, *d_wfdn = nullptr, *d_wfup = nullptr;
        double *d_w = nullptr;               // [D] np.trapz weights on the whole grid
        double *d_phi = nullptr;             // [2][kNPhi] cos(phi), trapz weights of phi = linspace(0, pi, kNPhi) (phase:81-82)
        double *d_z = nullptr;               // [L] altitude grid of the host epilogue
        sosrt::FixTab* d_fix = nullptr;
        int* d_small = nullptr;
    } grid;

    struct Phase {                       // phase matrices and their sets (api_phase.hip)
        std::vector<double> Wa_h, Wr_h;
        double *d_Wa = nullptr, *d_Wr = nullptr;
        bool wr_on_device = false;           // the sets were folded on the device (sosrt_set_phase_sets_dev): Wr_h / Wrx_h are filled on demand
        int nsets = 1;                       // aerosol phase sets of the last sosrt_set_phase* (1 also when there is no P_aer)
        std::vector<std::vector<double>> Wrx_h;   // folds of the sets 1 .. nsets-1 (set 0 is Wr_h)
        sosrt::GrowBuf<double> d_Wrsets;     // [nsets][Dp][Wld] folds of all sets (nsets > 1 only; set 0 is in d_Wr as well)
        sosrt::GrowBuf<double> d_Wrsets_s;   // their flip-symmetric folds (symmetric contraction)
        // Atmosphere phase sets (sosrt_set_atm_phase_sets): natm folded matrices, each certified low-rank, and
        // which one a column reads (sosrt_set_atmosphere_sets).  Set 0 is W_atm itself (d_Wa, d_lrU / d_lrV); the stacks below exist
        // from the first call on and are read only while a column is off set 0 (max_atm_used > 0).
        int natm = 1;                        // atmosphere sets of the last sosrt_set_atm_phase_sets (1 after every sosrt_set_phase*)
        sosrt::GrowBuf<double> d_Wasets;     // [natm][Dp][Wld] folds of all sets
        sosrt::GrowBuf<double> d_lrUsets, d_lrVsets;   // [natm][kLowRankMax][D] their factors
        sosrt::GrowBuf<int> d_lrranks;       // [natm] their ranks (its capacity: the sets the four stacks hold)
        // flip-symmetric contraction (jn_gemm.hip, SYM): folded copies [k][S | A] of W_atm, W_aer and the combined matrices
        double asymmetry = 0;                // max |W[k][m] - W[D-1-k][D-1-m]| / max |W| of the last sosrt_set_phase
        bool sym_ok = false;                 // asymmetry <= SOSRT_SYMMETRY_TOL
        bool sym_dirty = true, symmix_dirty = true, symsets_dirty = true;
        double *d_Wa_s = nullptr, *d_Wr_s = nullptr;
        // low-rank form of the plain rows (jn_gemm_tile.hpp, lowrank_rows): W_atm = U V by cross approximation in sosrt_set_phase
        int lr_rank = -1;                    // terms of the accepted factorisation; -1: none within SOSRT_LOWRANK_TOL
        double lr_residual = 0;              // max |W_atm - U V| / max |W_atm| after the last step taken
        double *d_lrU = nullptr, *d_lrV = nullptr;   // [kLowRankMax][D] each: U transposed, V
        float* d_Wa32 = nullptr;             // float copy of W_atm (SOSRT_CONTRACT_F32)
        bool w32_dirty = true;
    } phase;

    struct Columns {                     // columns, zone tables and mix groups (api_columns.hip)
        int *d_idx_up = nullptr, *d_idx_down = nullptr;
        int *d_nz = nullptr, *d_zr0 = nullptr, *d_zmix = nullptr;     // zone tables [max_batch][kMaxZones]
        double *d_zwr = nullptr, *d_zdtr = nullptr;
        int max_nz = 1;                      // most zones of any column (beyond three: the ring / chunk-parallel kernels' zone-table instantiation; general kernel where the register-streaming one would run)
        bool simple_zones = true;            // every column is (clear, slab, clear): the live-column tilings of the contraction apply
        double* d_scal = nullptr;            // 7 arrays of max_batch
        sosrt::ColDesc* d_desc = nullptr;
        double *d_rca = nullptr, *d_rcr = nullptr;
        int* d_slabrows = nullptr;
        int* d_mainrows = nullptr;
        int nslab = 0, nmain = 0;
        int max_main = 0, max_slab = 0;      // most plain / slab rows of any column
        // slab rows of the live-column tilings: one pass over ca W_atm + cr W_aer per distinct (ca, cr) of the batch
        static constexpr int kMaxMixGroups = 32;
        // Several aerosol phase sets (sosrt_set_phase_sets): a group is a distinct (set, ca, cr).  While every column uses set 0 the
        // cache holds kMaxMixGroups matrices, as it always did; once sosrt_set_aerosol_sets names another set it may grow to
        // kMaxMixGroupsSets, bounded by kMixCacheBytes of combined matrices (never below kMaxMixGroups).
        static constexpr int kMaxMixGroupsSets = 128;
        static constexpr size_t kMixCacheBytes = 256ull << 20;
        int mix_groups_max = 1 << 30;        // SOSRT_MIX_GROUPS: an upper bound on either cache (tests, A/B)
        int* d_mixset = nullptr;             // [kMaxMixGroupsSets] set of a group
        int max_set_used = 0;                // largest set index the current columns name (sosrt_set_aerosol_sets)
        int max_atm_used = 0;                // largest atmosphere set the current columns name
        std::vector<int> c_atmset;           // [B] atmosphere set of a column
        int* d_colatm = nullptr;             // [max_batch] atmosphere set of a column
        int* d_mixatm = nullptr;             // [kMaxMixGroupsSets] atmosphere set of a group
        int p0_zones = 0;                    // > 0: P0_aer of the first order is [B][p0_zones][2N], one row per zone of the caller's table
        sosrt::GrowBuf<double> d_P0rz;       // staging of such a P0_aer for the host entry points
        // host copy of the current columns' zone tables: sosrt_set_aerosol_sets groups the slab rows again
        std::vector<int> c_nz, c_zr0, c_zmix, c_zset;
        std::vector<double> c_zwr, c_zdtr, c_alb_atm, c_dtau_atm;
        int mix_groups = 0;                  // 0: disabled (too many distinct pairs, or no slab)
        bool mix_dirty = true;
        sosrt::GrowBuf<double> d_Wmix, d_Wmix_s;   // the combined matrices, and their folded copies (symmetric contraction)
        sosrt::GrowBuf<float> d_Wmix32;      // ... and their float copies (SOSRT_CONTRACT_F32)
        double *d_mixca = nullptr, *d_mixcr = nullptr;
        int* d_mixgroup = nullptr;
        int* d_slabtilegroup = nullptr;      // [tiles] group of every 32-row slab tile of the dense contraction
        // Per-level weights on the row coefficients (sosrt_set_row_weights_dev): while set, every k_prepare of a
        // solve or a source step is followed by one launch that multiplies d_rca / d_rcr by them, and the slab rows take two passes
        bool rw_on = false;
        bool rw_regrouped = false;           // setting them took the slab rows off their combined matrices: clearing puts them back
        sosrt::GrowBuf<double> d_rwa, d_rwr; // [B][L] copies of the caller's w_atm / w_aer (ones where it passed none)
    } cols;

    struct Contraction {                 // knobs of the contraction (plan_order, run_source)
        int mode = SOSRT_CONTRACT_F64;       // sosrt_set_contraction
        int diag_ks_mult = 1;                // SOSRT_GEMM_KS_MULT (diagnostic builds)
        int* d_livelist = nullptr;           // [max_batch] live columns of the current order, written by the source-function launch
        int gemm_tail_cols = 1 << 30;        // at or below this many live columns (and below the batch) tiles are laid over live columns (SOSRT_GEMM_TAIL)
        double gemm_tail_frac = 0.6;         // ... and at or below this fraction of the group's columns (SOSRT_GEMM_TAIL_FRAC): above it the dense
                                             // tiling, skipping the tiles of converged columns, is the faster one (contraction -3 % per step at 512 ... 4096 columns)
        int gemm_small_cols = 200;           // at or below this many, 32-row tiles (SOSRT_GEMM_SMALL)
        int dense_live_list = 1;             // the dense tiling writes the transport's live list (SOSRT_DENSE_LIVE_LIST=0: A/B)
        int gemm_regs_cols = -1;             // at or below this many (symmetric form), 16-row tiles with the matrix fragments in registers
                                             // (-1: while its workgroups, one per CU, are at most 1.5 rounds of the CUs; 0: never -- SOSRT_GEMM_REGS)
    } gemm;

    struct Transport {                   // knobs of the transport
        int use_etab = 1;
        sosrt::TransportKnob mode = sosrt::TransportKnob::Auto;
        int ring_slots = 3;                  // SOSRT_RING_SLOTS: ring depth of the ring kernel (a column group beside another: grp.coresident_slots)
        int ring_debug = 0;                  // SOSRT_RING_DEBUG, diagnostic builds only (-DSOSRT_RING_DEBUG)
        unsigned long long* d_stamps = nullptr;   // sosrt_debug_stamps: the caller's buffer, written by this handle's transport kernels
        int scan_cols = 200;                 // SOSRT_SCAN_COLS
        bool ring_ok = false, scan_ok = false, scan_split_ok = false, fast_ok = false;
        int scan_split = 1;                  // SOSRT_SCAN_SPLIT: two workgroups per column when at most half as many columns are live as the device has CUs
        // Moment mode of the ring kernel: in an order whose transport is the ring kernel for every column of the
        // group, the contraction writes a 64-byte moment record per plain row instead of the row of Jn and the ring kernel expands it
        int ring_moments = 1;                // SOSRT_RING_MOMENTS=0: rows of Jn always (A/B inside one process)
        double* d_mom = nullptr;             // [max_batch][L][kMomDoubles] records
        int moment_orders = 0, orders = 0;   // the last solve: (group, order) pairs transported in moment mode / by the two-launch loop (sosrt_ring_moments_stats)
        // Moment mode of the chunk-parallel kernel: the same records, expanded by k_transport_scan's MOM
        // instantiations, in an order that kernel transports -- a second decision, LaunchPlan::scan_moments; ring_moments and its
        // statistics keep their meaning
        int scan_moments = 1;                // SOSRT_SCAN_MOMENTS=0: rows of Jn always in the chunk-parallel kernel's orders
        // SOSRT_SCAN_MOMENTS_MIN: ... and below this many planned live columns of the group.  Measured, profiles/r08_scan_moments_threshold.txt:
        // the smallest of 8 .. 200 from which no order of the headline loses (an order with 126 live columns gains 6 us, one with 96
        // loses 1.6: the transport's launch is on its latency floor there and pays 3 us for the expansion, the contraction gains 2)
        int scan_moments_min_live = 128;
        int scan_moment_orders = 0;          // the last solve: pairs the chunk-parallel kernel transported in moment mode (sosrt_scan_moments_stats)
        double* d_scan_scratch = nullptr;    // [max_batch][transport_scan_scratch_doubles()] exchange rows of the split form
        int* d_scan_sync = nullptr;          // [max_batch][2] {arrivals, flags}, zero between launches
    } tr;

    struct Fields {                      // device: fields (internal) and the convergence state of a solve
        double *d_tau = nullptr, *d_P0a = nullptr, *d_P0r = nullptr;
        double *d_Jn = nullptr, *d_InA = nullptr, *d_InB = nullptr, *d_I = nullptr, *d_E = nullptr;
        int *d_active = nullptr, *d_norders = nullptr, *d_status = nullptr, *d_redo = nullptr, *d_erep = nullptr;
        // live columns per group + "some column needs k_smallmu": two sets used by alternate solves, the first kernel of a solve
        // zeroes the other set (no memset launch at the head of a solve); d_nactive points at the set of the current solve
        int *d_nactive_sets = nullptr, *d_nactive = nullptr;
        int nactive_set = 0;
        unsigned long long* d_tauhash = nullptr;
        double* d_ratio = nullptr;
        int* h_pub = nullptr;                // pinned [groups][2 slots][4]: {live count, tag, needs k_smallmu, -} published from the device
        bool need_small = true;              // some column keeps a k_smallmu value (known from the second order on)
        int pub_seq = 0;                     // tags are unique across solves
        int last_max_orders = 0;
        long long last_sum_orders = 0;
    } fld;

    // order-loop kernel (order_loop.hip): the last orders of a few live columns in one launch
    // (OFF by default: measured on MI355X it is bit-identical and slower -- a lone column 54.6 us per order against 47.0 with two
    // launches, 64 columns 137 against 50: the chain sweep -> tile of the next source function -> sweep is the same either way,
    // what the launches cost (~8 us per order) the polls and the write-through hand-offs cost too, and the contraction role has one
    // four-wave team per CU; profiles/r04_order_loop_ab_v0.txt)
    struct OrderLoop {
        int mode = 0;                        // sosrt_set_order_loop / SOSRT_ORDER_LOOP: 0 never (default), 1 where the launch plan says so
        double frac = 0.5;                   // ... while the transport workgroups of the live columns are at most this share of the grid
        int* d_sync = nullptr;               // [kMaxGroups][order_loop_sync_ints(kOrderLoopMaxCols)] words of a launch
        int* h_done = nullptr;               // pinned [kMaxGroups][2]: {state, tag} reported by the launch's last workgroup
        unsigned long long* d_log = nullptr; // diagnostic builds (-DSOSRT_OL_STAMPS): event log of an order-loop launch
        int launches = 0, refused = 0;       // launches of the last solve; launches that found their grid not resident
        bool group_used[kMaxGroups] = {false, false};      // column groups of the last solve that ran (to the end) in an order-loop launch
    } ol;

    struct PhaseFn {                     // phase functions on the device (api_phasefn.hip)
        double* d_tab = nullptr;             // [2][ntab] table of SOSRT_PHASE_TABLE
        int ntab = 0;
        sosrt::GrowBuf<double> d_modetab;    // cos(phi_q) [nphi] and w_q cos(m phi_q) [1 + m_count][nphi] of the last mode builder
        // Mie tables (sosrt_mie_ensembles): device arena and pinned staging of the per-call parameters, both grow-only; the
        // event orders a refill of the staging buffer behind the copy out of it; mie_t: events around the three kernels
        sosrt::GrowBuf<char> d_mie;
        sosrt::GrowBuf<char, true> h_mie;
        hipEvent_t mie_ev = nullptr, mie_t[4] = {nullptr, nullptr, nullptr, nullptr};
        bool mie_timed = false;
        sosrt::GrowBuf<double> d_deltam;     // delta-M (api_deltam.hip): the chunks' partial moments, or the series' coefficients
    } pf;

    struct View {                        // view radiance (api_view.hip): scratch of its own, so that the stage leaves the handle as it was
        sosrt::GrowBuf<double> d_fold;       // the folded rows [view_source_kpad(D)][view_source_cols(V)]
        sosrt::GrowBuf<double> d_S;          // [B][L][2V] source at the view lanes
        sosrt::GrowBuf<double> d_rc;         // [2][max_batch][L] row coefficients (ca, cr) of the call's own k_prepare
        sosrt::GrowBuf<sosrt::ColDesc> d_desc;   // [max_batch] its zone tables
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the source, the sweeps and the first order of the last call
        bool timed_scat = false, timed_first = false;
    } view;

    struct Comm {                        // RCCL communicator of the sharded solve (sosrt_comm_init)
        sosrt::Rccl::comm_t comm = nullptr;
        int rank = -1, world = 0;
    } net;
};

namespace sosrt {

inline size_t field_elems(const sosrt_handle* h) { return (size_t)h->max_batch * h->L * h->D; }

// the pools grow on demand (a long profiled run must not end up with timings of its first steps only)
inline bool prof_room(Prof& p) {
    if (p.used + 2 > p.ev.size()) {
        const size_t n0 = p.ev.size();
        p.ev.resize(n0 + 4096);
        for (size_t i = n0; i < p.ev.size(); ++i)
            if (hipEventCreateWithFlags(&p.ev[i], hipEventDisableSystemFence) != hipSuccess) { p.ev.resize(i); break; }
        if (p.used + 2 > p.ev.size()) return false;
    }
    if (p.nint >= p.kind.size()) {
        const size_t n = p.kind.size() + 4096;
        p.kind.resize(n, -1); p.first.resize(n, 0); p.last.resize(n, 0);
    }
    return true;
}
inline hipStream_t group_stream(sosrt_handle* h, int grp) { return grp == 0 ? h->stream : h->grp.stream2; }
inline void prof_begin(sosrt_handle* h, int kind, int grp = 0) {
    Prof& p = h->prof[grp];
    p.open = -1;
    if (!p.on || !prof_room(p)) return;
    if (p.adjacent >= 0) {
        p.open = p.adjacent;
    } else {
        p.open = (int)p.used++;
        hipEventRecord(p.ev[p.open], group_stream(h, grp));
    }
}
inline void prof_end(sosrt_handle* h, int kind, int grp = 0) {
    Prof& p = h->prof[grp];
    if (!p.on || p.open < 0) return;
    const int e = (int)p.used++;
    hipEventRecord(p.ev[e], group_stream(h, grp));
    p.kind[p.nint] = kind; p.first[p.nint] = p.open; p.last[p.nint] = e;
    ++p.nint;
    p.adjacent = e;
    p.open = -1;
}
// work enqueued outside a bracket: the next bracket needs its own opening event
inline void prof_break(sosrt_handle* h) { for (auto& p : h->prof) p.adjacent = -1; }

inline int need_gpu(sosrt_handle* h) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->gpu) return fail(SOSRT_E_STATE, "handle was created host-only (device < 0)");
    return 0;
}

inline Conv make_conv(sosrt_handle* h, double tol) {
    Conv c;
    c.active = h->fld.d_active; c.norders = h->fld.d_norders; c.status = h->fld.d_status;
    c.nactive = h->fld.d_nactive; c.ratio = h->fld.d_ratio; c.tol = tol; c.redo = h->fld.d_redo;
    c.target = nullptr;                 // (the solve sets its own: sosrt_set_order_targets)
    return c;
}

inline int check_ready(sosrt_handle* h, int B, bool need_phase) {
    if (int e = need_gpu(h)) return e;
    prof_break(h);
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (need_phase && !h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (B != h->B) return fail(SOSRT_E_INVALID, "B=%d does not match sosrt_set_columns (B=%d)", B, h->B);
    if (need_phase && h->geom == SOSRT_GEOM_THREE_ZONE && !h->have_aer)
        return fail(SOSRT_E_STATE, "three-zone geometry needs P_aer (sosrt_set_phase)");
    return 0;
}

inline ColScalars scalars_of(sosrt_handle* h) {
    ColScalars sc;
    const size_t mb = h->max_batch;
    double* d = h->cols.d_scal;
    sc.idx_up = h->cols.d_idx_up; sc.idx_down = h->cols.d_idx_down;
    sc.nz = h->cols.d_nz; sc.zr0 = h->cols.d_zr0; sc.zmix = h->cols.d_zmix; sc.zwr = h->cols.d_zwr; sc.zdtr = h->cols.d_zdtr;
    sc.mu0 = d + 0 * mb; sc.rho = d + 1 * mb; sc.alb_atm = d + 2 * mb;
    sc.alb_aer = d + 3 * mb; sc.dtau_atm = d + 4 * mb; sc.dtau_aer = d + 5 * mb;
    sc.T = d + 6 * mb;
    return sc;
}

// behind launch_prepare, wherever the row coefficients feed a contraction: rowcoef *= weights (nothing while no weights are set)
inline void apply_row_weights(sosrt_handle* h, hipStream_t s, int B) {
    if (h->cols.rw_on) launch_row_weights_apply(s, (size_t)B * h->L, h->cols.d_rwa.p, h->cols.d_rwr.p, h->cols.d_rca, h->cols.d_rcr);
}
// the guard of the entries that evaluate per-zone constants (first order, view stage, emission): not on a weighted column
inline int no_row_weights(const sosrt_handle* h, const char* what) {
    if (h && h->cols.rw_on)
        return fail(SOSRT_E_STATE, "%s evaluates one constant per zone, and per-level weights are set (sosrt_set_row_weights_dev): use "
                                   "sosrt_first_order_profile_dev / sosrt_emission_profile_dev, or clear the weights", what);
    return 0;
}

// api_profile.hip: what every entry of the weighted stages refuses (no grid, no columns, the single slab, B outside the current
// columns, L > kProfileMaxL, no weights set)
int profile_check(sosrt_handle* h, int B, const char* what);

inline bool use_sym(const sosrt_handle* h) {
    return (h->gemm.mode == SOSRT_CONTRACT_F64 || h->gemm.mode == SOSRT_CONTRACT_F64_DENSE) && h->phase.sym_ok;
}
inline bool use_lowrank(const sosrt_handle* h) { return h->gemm.mode == SOSRT_CONTRACT_F64 && h->phase.lr_rank >= 0; }

// api_phase.hip: buffers of the float contraction; combined and folded matrices of the current columns (on stream s)
int ensure_w32(sosrt_handle* h);
int ensure_matrices(sosrt_handle* h, hipStream_t s);
// api_columns.hip: groups the cache of combined matrices may hold
int mix_group_cap(const sosrt_handle* h, bool sets);
// api_phasefn.hip, shared with the builders at view lanes (api_view.hip): the checks of a phase function by kind, and the
// function as the builders' kernels take it (the table of sosrt_phase_table, if any: cosines, then values); the checks of a mode
// range, and the upload of cos(phi_q) and the weights of modes [mf, mf + mc) into pf.d_modetab (synchronises the handle's stream
// first); the job of a builder on the handle's grid (phasefn.hpp): with mc == 0 the reference's 25-node ring, else the modes
// [mf, mf + mc) on the table modes_table uploaded for them.  The caller adds what selects the builder (mu0, B, V2, ...) and out.
int phase_check(sosrt_handle* h, int kind, double g);
PhaseFn phase_fn(const sosrt_handle* h, int kind, double g);
PhaseJob phase_job(const sosrt_handle* h, int kind, double g, int mf = 0, int mc = 0, int nphi = 0);
int modes_check(sosrt_handle* h, int kind, double g, int m_first, int m_count, int nphi);
int modes_table(sosrt_handle* h, int nphi, int mf, int mc);

}  // namespace sosrt
