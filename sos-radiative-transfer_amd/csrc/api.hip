// C ABI of libsosrt.so (see include/sosrt.h).  Host logic only: argument checks, device
// buffers, the order loop with lagged convergence polling, HIP-event profiling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/sosrt.h"
#include "comm.hpp"
#include "kernels.hpp"
#include "plan.hpp"

using namespace sosrt;

namespace {
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

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return fail(SOSRT_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                           \
    } while (0)

constexpr int kProfPool = 8192;
constexpr int kNPhi = 25;                // phase:81  nb_phi

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
}  // namespace

struct sosrt_handle {
    int device = -1, L = 0, N = 0, D = 0, max_batch = 0, max_orders = 0;
    int order_budget = 0;                // orders a solve runs at most (sosrt_set_order_budget; <= max_orders, the default)
    int saved_slots = 0;                 // orders per column in I_saved_out (sosrt_set_saved_orders; default max_orders)
    bool gpu = false;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // Column groups of the order loop: a large batch is solved as two halves, the second on an internal stream, so
    // that the MFMA-bound contraction of one half overlaps the HBM-bound transport of the other (SOSRT_GROUPS)
    static constexpr int kMaxGroups = 2;
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
    int diag_ks_mult = 1;               // SOSRT_GEMM_KS_MULT (diagnostic builds)
    int coresident_slots = 3;           // SOSRT_GROUP_RING_SLOTS: ring depth of the transport under two groups
    double stagger = 1.0;                // a group starts when the previous one is down to this fraction of live columns (SOSRT_STAGGER; 1: together)
    int gb[kMaxGroups + 1] = {0, 0, 0};                    // column range of group g: [gb[g], gb[g+1])
    int main_off[kMaxGroups + 1] = {0, 0, 0};              // its plain rows in d_mainrows
    int slab_off[kMaxGroups + 1] = {0, 0, 0};              // its slab rows in d_slabrows (tile-aligned when grouped by coefficient pair)
    Plan plan;
    bool have_grid = false, have_phase = false, have_aer = false, have_cols = false;
    int B = 0, geom = 0, surface = 0;
    std::vector<double> Wa_h, Wr_h;
    Grid g{};
    // device: grid / phase
    double *d_mu = nullptr, *d_Wa = nullptr, *d_Wr = nullptr, *d_wfdn = nullptr, *d_wfup = nullptr;
    double *d_w = nullptr;               // [D] np.trapz weights on the whole grid
    int first_order_mode = SOSRT_FIRST_ORDER_CODED;   // sosrt_set_first_order
    double *d_phi = nullptr;             // [2][kNPhi] cos(phi), trapz weights of phi = linspace(0, pi, kNPhi) (phase:81-82)
    double *d_z = nullptr;               // [L] altitude grid of the host epilogue
    double *d_tab = nullptr;             // [2][ntab] table of SOSRT_PHASE_TABLE
    double *d_modetab = nullptr;         // cos(phi_q) [nphi] and w_q cos(m phi_q) [1 + m_count][nphi] of the last mode builder
    size_t modetab_cap = 0;
    const int* d_targets = nullptr;      // sosrt_set_order_targets (caller's device array [B]); null: the spec:309 test
    int ntab = 0;
    // Mie tables (sosrt_mie_ensembles): device arena and pinned staging of the per-call parameters, both grow-only; the
    // event orders a refill of the staging buffer behind the copy out of it; mie_t: events around the three kernels
    char* d_mie = nullptr;
    char* h_mie = nullptr;
    size_t mie_cap = 0, mie_hcap = 0;
    hipEvent_t mie_ev = nullptr, mie_t[4] = {nullptr, nullptr, nullptr, nullptr};
    bool mie_timed = false;
    bool resident = false;               // d_tau / d_I hold the inputs / result of the last sosrt_solve (of resident_B columns)
    int resident_B = 0;
    FixTab* d_fix = nullptr;
    int* d_small = nullptr;
    // device: columns
    int *d_idx_up = nullptr, *d_idx_down = nullptr;
    int *d_nz = nullptr, *d_zr0 = nullptr, *d_zmix = nullptr;     // zone tables [max_batch][kMaxZones]
    double *d_zwr = nullptr, *d_zdtr = nullptr;
    int max_nz = 1;                      // most zones of any column (beyond three: the ring / chunk-parallel kernels' zone-table instantiation; general kernel where the register-streaming one would run)
    bool simple_zones = true;            // every column is (clear, slab, clear): the live-column tilings of the contraction apply
    double* d_scal = nullptr;            // 7 arrays of max_batch
    ColDesc* d_desc = nullptr;
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
    bool wr_on_device = false;           // the sets were folded on the device (sosrt_set_phase_sets_dev): Wr_h / Wrx_h are filled on demand
    int nsets = 1;                       // aerosol phase sets of the last sosrt_set_phase* (1 also when there is no P_aer)
    std::vector<std::vector<double>> Wrx_h;   // folds of the sets 1 .. nsets-1 (set 0 is Wr_h)
    double* d_Wrsets = nullptr;          // [nsets][Dp][Wld] folds of all sets (nsets > 1 only; set 0 is in d_Wr as well)
    size_t wrsets_capacity = 0;
    double* d_Wrsets_s = nullptr;        // their flip-symmetric folds (symmetric contraction)
    size_t wrsets_s_capacity = 0;
    int* d_mixset = nullptr;             // [kMaxMixGroupsSets] set of a group
    int max_set_used = 0;                // largest set index the current columns name (sosrt_set_aerosol_sets)
    // Atmosphere phase sets (sosrt_set_atm_phase_sets): natm folded matrices, each certified low-rank, and
    // which one a column reads (sosrt_set_atmosphere_sets).  Set 0 is W_atm itself (d_Wa, d_lrU / d_lrV); the stacks below exist
    // from the first call on and are read only while a column is off set 0 (max_atm_used > 0).
    int natm = 1;                        // atmosphere sets of the last sosrt_set_atm_phase_sets (1 after every sosrt_set_phase*)
    int max_atm_used = 0;                // largest atmosphere set the current columns name
    std::vector<int> c_atmset;           // [B] atmosphere set of a column
    double* d_Wasets = nullptr;          // [natm][Dp][Wld] folds of all sets
    double *d_lrUsets = nullptr, *d_lrVsets = nullptr;   // [natm][kLowRankMax][D] their factors
    int* d_lrranks = nullptr;            // [natm] their ranks
    int atm_capacity = 0;                // sets the four stacks hold
    int* d_colatm = nullptr;             // [max_batch] atmosphere set of a column
    int* d_mixatm = nullptr;             // [kMaxMixGroupsSets] atmosphere set of a group
    int p0_zones = 0;                    // > 0: P0_aer of the first order is [B][p0_zones][2N], one row per zone of the caller's table
    double* d_P0rz = nullptr;            // staging of such a P0_aer for the host entry points
    size_t p0rz_capacity = 0;
    // host copy of the current columns' zone tables: sosrt_set_aerosol_sets groups the slab rows again
    std::vector<int> c_nz, c_zr0, c_zmix, c_zset;
    std::vector<double> c_zwr, c_zdtr, c_alb_atm, c_dtau_atm;
    int mix_groups = 0;                  // 0: disabled (too many distinct pairs, or no slab)
    bool mix_dirty = true;
    double *d_Wmix = nullptr, *d_mixca = nullptr, *d_mixcr = nullptr;
    int* d_mixgroup = nullptr;
    int* d_slabtilegroup = nullptr;      // [tiles] group of every 32-row slab tile of the dense contraction
    int contraction = SOSRT_CONTRACT_F64;
    // flip-symmetric contraction (jn_gemm.hip, SYM): folded copies [k][S | A] of W_atm, W_aer and the combined matrices
    double asymmetry = 0;                // max |W[k][m] - W[D-1-k][D-1-m]| / max |W| of the last sosrt_set_phase
    bool sym_ok = false;                 // asymmetry <= SOSRT_SYMMETRY_TOL
    bool sym_dirty = true, symmix_dirty = true, symsets_dirty = true;
    double *d_Wa_s = nullptr, *d_Wr_s = nullptr, *d_Wmix_s = nullptr;
    // low-rank form of the plain rows (jn_gemm_tile.hpp, lowrank_rows): W_atm = U V by cross approximation in sosrt_set_phase
    int lr_rank = -1;                    // terms of the accepted factorisation; -1: none within SOSRT_LOWRANK_TOL
    double lr_residual = 0;              // max |W_atm - U V| / max |W_atm| after the last step taken
    double *d_lrU = nullptr, *d_lrV = nullptr;   // [kLowRankMax][D] each: U transposed, V
    size_t mixs_capacity = 0;
    float *d_Wa32 = nullptr, *d_Wmix32 = nullptr;   // float copies of W_atm and of the combined slab matrices (SOSRT_CONTRACT_F32)
    size_t mix32_capacity = 0;
    bool w32_dirty = true;
    int* d_livelist = nullptr;           // [max_batch] live columns of the current order, written by the source-function launch
    size_t mix_capacity = 0;
    // device: fields (internal)
    double *d_tau = nullptr, *d_P0a = nullptr, *d_P0r = nullptr;
    double *d_Jn = nullptr, *d_InA = nullptr, *d_InB = nullptr, *d_I = nullptr, *d_E = nullptr;
    int use_etab = 1;
    // convergence
    int *d_active = nullptr, *d_norders = nullptr, *d_status = nullptr, *d_redo = nullptr, *d_erep = nullptr;
    // live columns per group + "some column needs k_smallmu": two sets used by alternate solves, the first kernel of a solve
    // zeroes the other set (no memset launch at the head of a solve); d_nactive points at the set of the current solve
    int *d_nactive_sets = nullptr, *d_nactive = nullptr;
    int nactive_set = 0;
    unsigned long long* d_tauhash = nullptr;
    // 0: general kernel, 1: wave-independent fast kernel (+ repair), 2: LDS-ring kernel, 3 (default): the ring kernel for
    // launches with many live columns (HBM-bound) and the chunk-parallel kernel (transport_scan.hip) for launches with at
    // most scan_cols (latency-bound), 4: the chunk-parallel kernel always.  The ring and the chunk-parallel kernel share
    // their arithmetic (chunk-local recurrence), so the choice follows the live count without touching a column's bits.
    int transport_mode = 3;
    int scan_cols = 200;                 // SOSRT_SCAN_COLS
    bool ring_ok = false, scan_ok = false, scan_split_ok = false;
    int scan_split = 1;                  // SOSRT_SCAN_SPLIT: two workgroups per column when at most half as many columns are live as the device has CUs
    int cu_count = 0;
    double* d_scan_scratch = nullptr;    // [max_batch][transport_scan_scratch_doubles()] exchange rows of the split form
    int* d_scan_sync = nullptr;          // [max_batch][2] {arrivals, flags}, zero between launches
    int gemm_tail_cols = 1 << 30;        // at or below this many live columns (and below the batch) tiles are laid over live columns (SOSRT_GEMM_TAIL)
    double gemm_tail_frac = 0.6;         // ... and at or below this fraction of the group's columns (SOSRT_GEMM_TAIL_FRAC): above it the dense
                                         // tiling, skipping the tiles of converged columns, is the faster one (contraction -3 % per step at 512 ... 4096 columns)
    int gemm_small_cols = 200;           // at or below this many, 32-row tiles (SOSRT_GEMM_SMALL)
    int dense_live_list = 1;             // the dense tiling writes the transport's live list (SOSRT_DENSE_LIVE_LIST=0: A/B)
    int gemm_regs_cols = -1;             // at or below this many (symmetric form), 16-row tiles with the matrix fragments in registers
                                         // (-1: while its workgroups, one per CU, are at most 1.5 rounds of the CUs; 0: never -- SOSRT_GEMM_REGS)
    bool fast_ok = false;
    double* d_ratio = nullptr;
    int* h_pub = nullptr;                // pinned [groups][2 slots][4]: {live count, tag, needs k_smallmu, -} published from the device
    bool need_small = true;              // some column keeps a k_smallmu value (known from the second order on)
    int pub_seq = 0;                     // tags are unique across solves
    int last_max_orders = 0;
    long long last_sum_orders = 0;
    Prof prof[kMaxGroups];               // per column group (= per stream)
    // order-loop kernel (order_loop.hip): the last orders of a few live columns in one launch
    // (OFF by default: measured on MI355X it is bit-identical and slower -- a lone column 54.6 us per order against 47.0 with two
    // launches, 64 columns 137 against 50: the chain sweep -> tile of the next source function -> sweep is the same either way,
    // what the launches cost (~8 us per order) the polls and the write-through hand-offs cost too, and the contraction role has one
    // four-wave team per CU; profiles/r04_order_loop_ab_v0.txt)
    int order_loop = 0;                  // sosrt_set_order_loop / SOSRT_ORDER_LOOP: 0 never (default), 1 where the launch plan says so
    double ol_frac = 0.5;                // ... while the transport workgroups of the live columns are at most this share of the grid
    int* d_olsync = nullptr;             // [kMaxGroups][order_loop_sync_ints(kOrderLoopMaxCols)] words of a launch
    int* h_oldone = nullptr;             // pinned [kMaxGroups][2]: {state, tag} reported by the launch's last workgroup
    unsigned long long* d_ollog = nullptr;   // diagnostic builds (-DSOSRT_OL_STAMPS): event log of an order-loop launch
    int ol_launches = 0, ol_refused = 0; // launches of the last solve; launches that found their grid not resident
    bool ol_group_used[kMaxGroups] = {false, false};      // column groups of the last solve that ran (to the end) in an order-loop launch
    // RCCL communicator of the sharded solve (sosrt_comm_init)
    Rccl::comm_t comm = nullptr;
    int comm_rank = -1, comm_world = 0;
};

namespace {

size_t field_elems(const sosrt_handle* h) { return (size_t)h->max_batch * h->L * h->D; }

template <class T>
int dalloc(T** p, size_t n) {
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(SOSRT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    return 0;
}

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

// the pools grow on demand (a long profiled run must not end up with timings of its first steps only)
bool prof_room(Prof& p) {
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
hipStream_t group_stream(sosrt_handle* h, int grp) { return grp == 0 ? h->stream : h->stream2; }
void prof_begin(sosrt_handle* h, int kind, int grp = 0) {
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
void prof_end(sosrt_handle* h, int kind, int grp = 0) {
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
void prof_break(sosrt_handle* h) { for (auto& p : h->prof) p.adjacent = -1; }

int need_gpu(sosrt_handle* h) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->gpu) return fail(SOSRT_E_STATE, "handle was created host-only (device < 0)");
    return 0;
}

// Live columns after the order whose tag is `tag`, as published by the source-function launch of the
// next order (publish_live in kernels.hpp).  Spins on pinned memory; negative = error code.
int wait_published(sosrt_handle* h, int grp, int tag) {
    volatile int* slot = h->h_pub + 8 * grp + 4 * (tag & 1);
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::milliseconds(20);
    for (unsigned it = 1;; ++it) {
        if (__atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) == tag) {
            h->need_small = slot[2] != 0;
            return slot[0];
        }
        // The stream is asked only when the wait is far longer than any order takes (an error has happened, or the GPU is shared):
        // hipStreamQuery puts a marker into the queue, and the kernel behind a marker starts ~6 us late (measured: a query every
        // 0.3 ms of waiting cost every dense order of the headline sweep that gap).
        if ((it & 0x3fff) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (now >= next_query) {
                next_query = now + std::chrono::milliseconds(20);
                const hipError_t q = hipStreamQuery(group_stream(h, grp));
                if (q != hipSuccess && q != hipErrorNotReady) return fail(SOSRT_E_HIP, "order loop: %s", hipGetErrorString(q));
                if (q == hipSuccess && __atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) != tag)
                    return fail(SOSRT_E_HIP, "order loop: the stream drained without publishing order tag %d", tag);
                if (now - t0 > std::chrono::seconds(120))
                    return fail(SOSRT_E_HIP, "order loop: no progress for 120 s");
            }
        }
        __builtin_ia32_pause();
    }
}

Conv make_conv(sosrt_handle* h, double tol) {
    Conv c;
    c.active = h->d_active; c.norders = h->d_norders; c.status = h->d_status;
    c.nactive = h->d_nactive; c.ratio = h->d_ratio; c.tol = tol; c.redo = h->d_redo;
    c.target = nullptr;                 // (the solve sets its own: sosrt_set_order_targets)
    return c;
}

int check_ready(sosrt_handle* h, int B, bool need_phase) {
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

ColScalars scalars_of(sosrt_handle* h) {
    ColScalars sc;
    const size_t mb = h->max_batch;
    sc.idx_up = h->d_idx_up; sc.idx_down = h->d_idx_down;
    sc.nz = h->d_nz; sc.zr0 = h->d_zr0; sc.zmix = h->d_zmix; sc.zwr = h->d_zwr; sc.zdtr = h->d_zdtr;
    sc.mu0 = h->d_scal + 0 * mb; sc.rho = h->d_scal + 1 * mb; sc.alb_atm = h->d_scal + 2 * mb;
    sc.alb_aer = h->d_scal + 3 * mb; sc.dtau_atm = h->d_scal + 4 * mb; sc.dtau_aer = h->d_scal + 5 * mb;
    sc.T = h->d_scal + 6 * mb;
    return sc;
}

// buffers of the float contraction (SOSRT_CONTRACT_F32)
int ensure_w32(sosrt_handle* h) {
    if (h->contraction != SOSRT_CONTRACT_F32) return 0;
    if (h->nslab > 0 && h->mix_groups == 0)
        return fail(SOSRT_E_INVALID, "the float contraction needs at most %d distinct slab coefficient pairs in a batch", sosrt_handle::kMaxMixGroups);
    const size_t need = (size_t)h->g.Dp * h->g.Wld * (size_t)(h->mix_groups > 0 ? h->mix_groups : 1);
    if (need > h->mix32_capacity) {
        if (h->d_Wmix32) hipFree(h->d_Wmix32);
        h->d_Wmix32 = nullptr; h->mix32_capacity = 0;
        if (int e = dalloc(&h->d_Wmix32, need)) return e;
        h->mix32_capacity = need;
        h->w32_dirty = true;
    }
    return 0;
}

bool use_sym(const sosrt_handle* h) {
    return (h->contraction == SOSRT_CONTRACT_F64 || h->contraction == SOSRT_CONTRACT_F64_DENSE) && h->sym_ok;
}
bool use_lowrank(const sosrt_handle* h) { return h->contraction == SOSRT_CONTRACT_F64 && h->lr_rank >= 0; }

// Cross approximation of a folded matrix W [D][D] (row k, column m): up to kLowRankMax steps of Gaussian elimination with
// complete pivoting, U[k][q] = R[k][j] / R[i][j], V[q][m] = R[i][m] for the largest |R[i][j]| of the Schur complement R, which
// then loses that term.  The rank is the first step count whose complement is at most SOSRT_LOWRANK_TOL of max |W|, and the
// certificate is then computed from the factors themselves: max |W - U V| <= SOSRT_LOWRANK_TOL max |W|.  A NaN anywhere, or no
// such count, gives -1.  Ut [kLowRankMax][D] = U transposed, V [kLowRankMax][D], zero beyond the rank.
int lowrank_factor(const std::vector<double>& W, int D, std::vector<double>& Ut, std::vector<double>& V, double* residual) {
    Ut.assign((size_t)kLowRankMax * D, 0.0);
    V.assign((size_t)kLowRankMax * D, 0.0);
    auto absmax = [](const std::vector<double>& X, size_t* at) {
        double amax = 0;
        bool nan = false;
        for (size_t e = 0; e < X.size(); ++e) {
            const double ax = std::fabs(X[e]);
            nan |= std::isnan(ax);
            if (ax > amax) { amax = ax; if (at) *at = e; }
        }
        return nan ? std::nan("") : amax;
    };
    std::vector<double> R(W);
    const double wmax = absmax(W, nullptr);
    *residual = wmax;
    if (!std::isfinite(wmax)) return -1;
    int rank = -1;
    for (int r = 0; r <= kLowRankMax; ++r) {
        size_t at = 0;
        const double amax = absmax(R, &at);
        *residual = wmax > 0 ? amax / wmax : amax;
        if (std::isnan(amax)) return -1;
        if (amax <= SOSRT_LOWRANK_TOL * wmax) { rank = r; break; }
        if (r == kLowRankMax) return -1;
        const int i = (int)(at / D), j = (int)(at % D);
        const long double piv = R[at];
        for (int k = 0; k < D; ++k) Ut[(size_t)r * D + k] = (double)(R[(size_t)k * D + j] / piv);
        for (int m = 0; m < D; ++m) V[(size_t)r * D + m] = R[(size_t)i * D + m];
        for (int k = 0; k < D; ++k) {
            const long double u = Ut[(size_t)r * D + k];
            double* row = &R[(size_t)k * D];
            const double* v = &V[(size_t)r * D];
            for (int m = 0; m < D; ++m) row[m] = (double)(row[m] - u * v[m]);
        }
    }
    // the certificate, from the factors the device will use
    double res = 0;
    for (int k = 0; k < D; ++k)
        for (int m = 0; m < D; ++m) {
            long double uv = 0;
            for (int q = 0; q < rank; ++q) uv += (long double)Ut[(size_t)q * D + k] * V[(size_t)q * D + m];
            const double d = std::fabs((double)(W[(size_t)k * D + m] - uv));
            if (!(d <= res)) res = d;                   // (a NaN ends up here and refuses the factors below)
        }
    *residual = wmax > 0 ? res / wmax : res;
    return (res <= SOSRT_LOWRANK_TOL * wmax) ? rank : -1;
}

// combined slab matrices and, for the symmetric contraction, the folded copies of every matrix (on stream s)
int ensure_matrices(sosrt_handle* h, hipStream_t s) {
    const Grid& g = h->g;
    const size_t per = (size_t)g.Dp * g.Wld;
    const bool mixed = h->mix_groups > 0 && h->mix_dirty;
    if (mixed) {
        prof_break(h);
        const bool sets = h->max_set_used > 0, atm = h->max_atm_used > 0;
        launch_wmix(s, per, h->mix_groups, atm ? h->d_Wasets : h->d_Wa, sets ? h->d_Wrsets : h->d_Wr, h->d_mixca, h->d_mixcr,
                    h->d_Wmix, sets ? h->d_mixset : nullptr, atm ? h->d_mixatm : nullptr);
        h->mix_dirty = false;
        h->symmix_dirty = true;
    }
    if (!use_sym(h)) return 0;
    if (h->sym_dirty) {
        prof_break(h);
        if (!h->d_Wa_s) { if (int e = dalloc(&h->d_Wa_s, per)) return e; }
        if (!h->d_Wr_s) { if (int e = dalloc(&h->d_Wr_s, per)) return e; }
        launch_symfold(s, 1, g.N, g.D, g.Dp, g.Wld, h->d_Wa, h->d_Wa_s);
        launch_symfold(s, 1, g.N, g.D, g.Dp, g.Wld, h->d_Wr, h->d_Wr_s);
        h->sym_dirty = false;
        h->symsets_dirty = true;
    }
    // the folded copies of every set: only the two-pass form with sets reads them
    if (h->symsets_dirty && h->nsets > 1 && h->mix_groups == 0 && h->max_set_used > 0) {
        prof_break(h);
        {
            if (per * h->nsets > h->wrsets_s_capacity) {
                if (h->d_Wrsets_s) hipFree(h->d_Wrsets_s);
                h->d_Wrsets_s = nullptr; h->wrsets_s_capacity = 0;
                if (int e = dalloc(&h->d_Wrsets_s, per * h->nsets)) return e;
                h->wrsets_s_capacity = per * h->nsets;
            }
            launch_symfold(s, h->nsets, g.N, g.D, g.Dp, g.Wld, h->d_Wrsets, h->d_Wrsets_s);
        }
        h->symsets_dirty = false;
    }
    if (h->mix_groups > 0 && h->symmix_dirty) {
        prof_break(h);
        const size_t need = per * h->mix_groups;
        if (need > h->mixs_capacity) {
            // (the stream may still read the old buffer: hipFree synchronises)
            if (h->d_Wmix_s) hipFree(h->d_Wmix_s);
            h->d_Wmix_s = nullptr; h->mixs_capacity = 0;
            if (int e = dalloc(&h->d_Wmix_s, need)) return e;
            h->mixs_capacity = need;
        }
        launch_symfold(s, h->mix_groups, g.N, g.D, g.Dp, g.Wld, h->d_Wmix, h->d_Wmix_s);
        h->symmix_dirty = false;
    }
    return 0;
}

// Jn for every row of a column group (grp < 0: the whole batch) in one launch: plain rows against W_atm, slab rows
// against the combined matrix of their coefficient pair (or W_atm and W_aer in two passes)
void run_source(sosrt_handle* h, const double* In_1, double* Jn, const int* active, int tail_cols = 0, int pub_tag = 0,
                int grp = -1, bool all_live = false, bool regs_tile = false, int dense_live_cap = 0) {
    const int g0 = grp < 0 ? 0 : grp, g1 = grp < 0 ? h->ngroups : grp + 1;
    const int pg = grp < 0 ? 0 : grp;
    hipStream_t s = group_stream(h, pg);
    GemmArgs ga;
    ga.A = In_1; ga.Wa = h->d_Wa; ga.Wr = h->d_Wr; ga.ca = h->d_rca; ga.cr = h->d_rcr;
    if (h->nslab > 0) {
        ga.rows_main = h->d_mainrows + h->main_off[g0];
        ga.n_main = h->main_off[g1] - h->main_off[g0];
    } else {                                           // no slab rows: the identity list, offset by the group's first row
        ga.rows_main = nullptr;
        ga.n_main = (h->gb[g1] - h->gb[g0]) * h->L;
        ga.A = In_1 + (size_t)h->gb[g0] * h->L * h->D;
        Jn += (size_t)h->gb[g0] * h->L * h->D;
        ga.ca = h->d_rca + (size_t)h->gb[g0] * h->L;
        ga.cr = h->d_rcr + (size_t)h->gb[g0] * h->L;
        if (active) active += h->gb[g0];
    }
    ga.rows_slab = h->d_slabrows + h->slab_off[g0]; ga.n_slab = h->slab_off[g1] - h->slab_off[g0];
    ga.D = h->g.D; ga.Dp = h->g.Dp; ga.Wld = h->g.Wld; ga.L = h->L; ga.C = Jn; ga.active = active;
    // Two column groups: the large tilings of the contraction are capped at two workgroups per CU (unused LDS up to a
    // third of the CU's) so that a transport workgroup of the other group -- 53 KB with a two-slot ring -- runs beside
    // them: the MFMA-bound contraction of one group then overlaps the HBM-bound transport of the other
    if (grp >= 0 && h->ngroups > 1) ga.pad_lds = h->coresident_pad;
    if (pub_tag) {
        ga.nactive = h->d_nactive + pg; ga.need_small = h->d_nactive + sosrt_handle::kMaxGroups;
        ga.host_pub = h->h_pub + 8 * pg; ga.tag = pub_tag;
    }
    // The dense tiling skips the tiles whose columns have all converged -- two barriers and a dependent load per tile.  When the
    // host knows every column of the launch to be live (its count lags by one order: at most the columns that converged in the
    // last order are multiplied once more, and the transport ignores them) the check is dropped: 160 -> 157 us per 512-column launch.
    ga.check_tiles = all_live ? 0 : 1;
    if (ensure_matrices(h, s)) return;                 // (allocation failure: reported by the caller's hipGetLastError / next call)
    if (h->mix_groups > 0) {
        ga.Wmix = h->d_Wmix; ga.mix_group = h->d_mixgroup; ga.slab_tile_group = h->d_slabtilegroup + h->slab_off[g0] / 32;
    }
    const bool two_pass_sets = h->mix_groups == 0 && h->max_set_used > 0 && h->nslab > 0;
    if (two_pass_sets) {                               // the second pass picks the W_aer of a tile's / a column's set
        ga.Wr = h->d_Wrsets; ga.mix_group = h->d_mixgroup; ga.slab_tile_group = h->d_slabtilegroup + h->slab_off[g0] / 32;
    }
    if (use_lowrank(h)) { ga.lr_rank = h->lr_rank; ga.lrU = h->d_lrU; ga.lrV = h->d_lrV; }
    // atmosphere sets in use: the launches' twins that pick a plain row's factors by its column's set (every set is low-rank, the
    // contraction is the symmetric f64 one: sosrt_set_atm_phase_sets / sosrt_set_atmosphere_sets refuse anything else)
    AtmSets at;
    const AtmSets* atp = nullptr;
    if (h->max_atm_used > 0) {
        at.col_atm = h->d_colatm + (h->nslab > 0 ? 0 : h->gb[g0]);
        at.lr_ranks = h->d_lrranks;
        ga.lrU = h->d_lrUsets; ga.lrV = h->d_lrVsets;
        atp = &at;
    }
    if (use_sym(h)) {
        ga.sym = 1; ga.Ks = (h->g.N + GEMM_KC - 1) / GEMM_KC * GEMM_KC;
#ifdef SOSRT_DIAG
        // diagnostic builds (timing only; the results do not change: the extra chunks multiply zeros): SOSRT_GEMM_KS_MULT=2 doubles
        // the chunks per tile at the same prologue / epilogue, which separates the two (tile time = P + chunks * C); read once,
        // at sosrt_create
        if (h->diag_ks_mult > 1 && ga.Ks * h->diag_ks_mult <= h->g.Dp) ga.Ks *= h->diag_ks_mult;
#endif
        ga.Wa = h->d_Wa_s; ga.Wr = two_pass_sets ? h->d_Wrsets_s : h->d_Wr_s;
        if (ga.Wmix) ga.Wmix = h->d_Wmix_s;
    }
    if (h->contraction == SOSRT_CONTRACT_F32) {
        // float operands, float accumulator: the dense tiling over the row lists for every order (tiles of converged
        // columns leave at once)
        if (h->w32_dirty) {
            prof_break(h);
            const size_t per = (size_t)h->g.Dp * h->g.Wld;
            launch_to_float(s, per, h->d_Wa, h->d_Wa32);
            if (h->mix_groups > 0) launch_to_float(s, per * h->mix_groups, h->d_Wmix, h->d_Wmix32);
            h->w32_dirty = false;
        }
        prof_begin(h, SOSRT_K_GEMM, pg);
        launch_gemm_f32(s, ga, h->d_Wa32, h->d_Wmix32);
        prof_end(h, SOSRT_K_GEMM, pg);
        return;
    }
    prof_begin(h, SOSRT_K_GEMM, pg);
    if (tail_cols > 0 && active && h->nslab >= 0) {
        ga.col0 = h->nslab > 0 ? h->gb[g0] : 0; ga.B = h->gb[g1] - h->gb[g0];
        ga.max_main = h->max_main; ga.max_slab = h->max_slab;
        ga.idx_up = h->nslab > 0 ? h->d_idx_up : nullptr; ga.idx_down = h->nslab > 0 ? h->d_idx_down : nullptr;
        ga.live_list = h->d_livelist + h->gb[g0]; ga.live_cap = tail_cols;
        launch_gemm_tail(s, ga, tail_cols, tail_cols <= h->gemm_small_cols, regs_tile, atp);
    } else {
        if (dense_live_cap > 0 && active && h->nslab >= 0) {     // the dense tiling writes the transport's live list too
            ga.col0 = h->nslab > 0 ? h->gb[g0] : 0; ga.B = h->gb[g1] - h->gb[g0];
            ga.live_list = h->d_livelist + h->gb[g0]; ga.live_cap = dense_live_cap;
        }
        launch_gemm(s, ga, atp);
    }
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
    int ring_mode = 1;                   // 3: ring-class kernels, 1: the register-streaming kernel
};
SolveShape solve_shape(const sosrt_handle* h, int max_nz) {
    SolveShape sh;
    // The ring / chunk-parallel kernels take columns of any zone count (an instantiation that tests every boundary of the zone
    // table, chosen when the batch holds such a column); the register-streaming kernel knows three zones, so a batch with more
    // goes to the general kernel where that one would run (odd N, N > 256).
    sh.ring_like = h->transport_mode >= 2 && h->ring_ok && (max_nz <= kRingZones || transport_ring_fits(h->g, max_nz));
    sh.fast = h->transport_mode >= 1 && h->fast_ok && (max_nz <= kRingZones || sh.ring_like);
    sh.nzcap = max_nz > kRingZones ? max_nz : kRingZones;
    sh.ring_mode = (h->transport_mode >= 2 && h->ring_ok) ? 3 : 1;
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
};
struct LaunchPlan {
    int tail_cols = 0;                   // contraction over the live columns: capacity of the launch (0: dense tiling over the row lists)
    int live_cap = 0;                    // transport over the live list: its capacity (0: over all columns of the group)
    int gemm = SOSRT_PLAN_GEMM_DENSE;
    int transport = SOSRT_PLAN_TRANSPORT_GENERAL;
    int parts = 1;                       // chunk-parallel kernel: workgroups per column
    int repair = 0;                      // register-streaming kernel: the general kernel behind it for searches that leave wave 0
    int order_loop = 0;                  // this and every later order of the group in ONE order-loop launch
    int ol_parts = 0;                    // ... workgroups per column of its transport role
    int ol_grid = 0;                     // ... workgroups of the launch
};
LaunchPlan plan_order(const sosrt_handle* h, const SolveShape& sh, const OrderInputs& in) {
    LaunchPlan pl;
    const Grid& g = h->g;
    // contraction: the tilings over the live columns whenever some column has converged -- and for a small batch from the
    // start: their 32-row tiles put a few columns on more CUs than the dense tiling's 64-row tiles; same bits either way.
    // (the float contraction has the dense tiling only: no live list for the transport either)
    const bool live_tiling = h->contraction != SOSRT_CONTRACT_F32 && in.simple_zones && in.known <= h->gemm_tail_cols &&
                             (in.known <= h->gemm_tail_frac * in.nb || in.nb <= h->gemm_small_cols) &&
                             (in.known < in.nb || in.nb <= h->gemm_small_cols);
    pl.tail_cols = live_tiling ? in.known : 0;
    pl.gemm = !live_tiling ? SOSRT_PLAN_GEMM_DENSE
                           : (pl.tail_cols <= h->gemm_small_cols ? ((use_sym(h) && pl.tail_cols <= 32) ? SOSRT_PLAN_GEMM_LIVE32_DEEP : SOSRT_PLAN_GEMM_LIVE32)
                                                                 : SOSRT_PLAN_GEMM_LIVE64);
    // The last few columns: a tile's latency is the launch's, and the register-resident 16-row tile (jn_gemm_tile.hpp:
    // gemm_tile_lone) has half the staged tile's -- a lone column's launch 12.6 -> 10.0 us at N = 128, 4.7 of which an empty launch
    // takes (profiles/r04_gemm_regs_ab.txt).  Its workgroups are alone on their CUs and each fetches its own share of the matrix:
    // it wins while they make at most about a round and a half (13 columns at L = 200, N = 128; 6 at N = 256), measured break-even
    // at 16 / 8 -- and loses where a lone column is already more than that: L = 800, N = 501, 133 -> 144 us per order (profiles/r04_gemm_regs_ab.txt).  (Its tile's rows of In_1 must fit the LDS, and N rounded up to the k-chunk must be whole register blocks of 64.)
    {
        const int nct = (g.D + GEMM_BN - 1) / GEMM_BN;
        const int auto_cap = (3 * h->cu_count / 2) / (((g.L + 15) / 16 + 1) * nct);
        const int cap = h->gemm_regs_cols >= 0 ? h->gemm_regs_cols : auto_cap;       // (0 at the reference's shipped size: 408 workgroups for a lone column)
        if (live_tiling && use_sym(h) && pl.tail_cols <= cap && 16 * (g.D + 2) * 8 <= 150 * 1024 &&
            ((g.N + GEMM_KC - 1) / GEMM_KC * GEMM_KC) % 64 == 0) pl.gemm = SOSRT_PLAN_GEMM_LIVE16_REGS;
    }
    // The transport takes its columns from the live list whenever some column has converged: the live-column tilings write the
    // list, and so does the dense tiling (one more workgroup) -- the ring-class kernels then run over the live columns, dealt to
    // the CUs one by one, instead of over a batch whose live columns sit where they were put.  (Not the float contraction.)
    pl.live_cap = live_tiling ? pl.tail_cols : ((h->contraction != SOSRT_CONTRACT_F32 && h->dense_live_list && in.known < in.nb) ? in.known : 0);
    // transport
    {
        const int cols_now = pl.live_cap > 0 ? pl.live_cap : in.nb;
        // chunk-parallel kernel: a column on ceil(N / 64) CUs (two at N = 128, four at N = 256) while that many workgroups per
        // live column fit the device at once (the reflection must stay inside a part)
        // (where the shape has no ring kernel -- odd N, N > 256: the split form's WIDE instantiation -- the alternative is the
        // register-streaming kernel, one workgroup per column and 650 us per order at the shipped size against 133 for a round of
        // split workgroups: up to four rounds of them are the faster way)
        const int split_cap = sh.ring_mode == 3 ? h->cu_count : 4 * h->cu_count;
        const bool can_split = h->scan_split && h->scan_split_ok && transport_scan_parts(g) * cols_now <= split_cap &&
                               (in.surface == SOSRT_SURFACE_SPECULAR || in.surface == SOSRT_SURFACE_NONE);
        const bool want_scan = h->transport_mode == 4 || (h->transport_mode == 3 && cols_now <= h->scan_cols);
        // (the split form also takes the shapes no wave-independent kernel does -- the rewritten directions straddle two waves of a
        // half row, e.g. N = 70, 129, 257: sh.fast is false -- as long as the attenuation tables are built)
        const bool split = can_split && transport_scan_fits(g, sh.nzcap, true) && (sh.fast || (h->use_etab && h->transport_mode >= 3));
        const bool scan = want_scan && ((sh.fast && sh.ring_mode == 3 && h->scan_ok && transport_scan_fits(g, sh.nzcap, false)) || split);
        pl.transport = scan ? SOSRT_PLAN_TRANSPORT_SCAN
                            : (!sh.fast ? SOSRT_PLAN_TRANSPORT_GENERAL : (sh.ring_mode == 3 ? SOSRT_PLAN_TRANSPORT_RING : SOSRT_PLAN_TRANSPORT_FAST));
        if (scan && split) pl.parts = transport_scan_parts(g);
        pl.repair = (h->N - 3 > 61 && pl.transport == SOSRT_PLAN_TRANSPORT_FAST) ? 1 : 0;
    }
    // order-loop kernel: the remaining orders in one launch once the live columns' transport workgroups are a small share of the
    // CUs it may take (the other workgroups contract).  It holds the chunk-parallel transport (three zones, no kept k_smallmu
    // lane) and the symmetric contraction's live-column tiles; the default transport policy only (a forced kernel stays forced).
    if (h->order_loop && in.cu_share > 0 && h->transport_mode == 3 && sh.fast && sh.ring_mode == 3 && sh.nzcap <= kRingZones &&
        use_sym(h) && in.simple_zones && in.slabs_mixed && !in.saving && !in.need_small && in.orders_left >= 1 &&
        in.known <= kOrderLoopMaxCols) {
        Grid gt = g;
        gt.nsmall = 0;
        const bool split_ok = h->scan_split && (in.surface == SOSRT_SURFACE_SPECULAR || in.surface == SOSRT_SURFACE_NONE) && order_loop_ok(gt, true);
        const int sp = order_loop_parts(gt, true);
        if (split_ok && sp * in.known <= h->ol_frac * in.cu_share) {
            pl.order_loop = 1; pl.ol_parts = sp;
        } else if (order_loop_ok(gt, false) && in.known <= h->ol_frac * in.cu_share) {
            pl.order_loop = 1; pl.ol_parts = 1;
        }
        if (pl.order_loop) pl.ol_grid = in.cu_share;
    }
    return pl;
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

}  // namespace

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
    if (const char* ev = getenv("SOSRT_ETAB")) h->use_etab = atoi(ev);
    if (const char* ev = getenv("SOSRT_CONTRACT"))            // "full": the D x D product whatever the symmetry of the matrices
        if (strcmp(ev, "full") == 0) h->contraction = SOSRT_CONTRACT_F64_FULL;
    if (const char* ev = getenv("SOSRT_TRANSPORT"))
        h->transport_mode = strcmp(ev, "general") == 0 ? 0 : (strcmp(ev, "ring") == 0 ? 2 : (strcmp(ev, "scan") == 0 ? 4 : (strcmp(ev, "auto") == 0 ? 3 : 1)));
    if (const char* ev = getenv("SOSRT_SCAN_COLS")) h->scan_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_SCAN_SPLIT")) h->scan_split = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_TAIL")) h->gemm_tail_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_TAIL_FRAC")) h->gemm_tail_frac = atof(ev);
    if (const char* ev = getenv("SOSRT_GEMM_SMALL")) h->gemm_small_cols = atoi(ev);
    if (const char* ev = getenv("SOSRT_DENSE_LIVE_LIST")) h->dense_live_list = atoi(ev) != 0;
    if (const char* ev = getenv("SOSRT_GEMM_REGS")) h->gemm_regs_cols = atoi(ev);           // (A/B: 0 = the staged tilings for every live count)
    if (const char* ev = getenv("SOSRT_GROUPS")) h->want_groups = atoi(ev) >= 2 ? 2 : (atoi(ev) == 1 ? 1 : 0);      // column groups of the order loop (0: auto)
    if (const char* ev = getenv("SOSRT_SPLIT_MIN")) h->split_min = atoi(ev);                  // smallest batch that is split
    if (const char* ev = getenv("SOSRT_MIX_GROUPS")) h->mix_groups_max = atoi(ev);          // (tests, A/B: fewer combined matrices than the cache would hold -- the two-pass form sooner)
#ifdef SOSRT_DIAG   // measurement knobs of DESIGN section 5 (items 1, 5, 8): diagnostic builds only (-DSOSRT_DIAG), never in the product library
    if (const char* ev = getenv("SOSRT_STAGGER")) h->stagger = atof(ev);
    if (const char* ev = getenv("SOSRT_GROUP_SPLIT")) h->split_at = atoi(ev);
    if (const char* ev = getenv("SOSRT_GROUP_PRIO")) h->prio2 = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_PAD_LDS")) h->coresident_pad = atoi(ev);
    if (const char* ev = getenv("SOSRT_GEMM_KS_MULT")) h->diag_ks_mult = atoi(ev);
#endif
    if (const char* ev = getenv("SOSRT_GROUP_RING_SLOTS")) h->coresident_slots = atoi(ev);
    if (const char* ev = getenv("SOSRT_ORDER_LOOP")) h->order_loop = atoi(ev) != 0;           // (A/B: 0 = every order as two launches)
    if (const char* ev = getenv("SOSRT_RING_SLOTS")) g_ring_slots = atoi(ev);
#ifdef SOSRT_RING_DEBUG   // diagnostic builds only: the switches make the ring kernel skip work, its results are wrong
    if (const char* ev = getenv("SOSRT_RING_DEBUG")) g_ring_debug = atoi(ev);
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
            HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
            const size_t mb = max_batch, fe = field_elems(h);
            if ((e = dalloc(&h->d_mu, g.D))) return e;
            if ((e = dalloc(&h->d_Wa, (size_t)g.Dp * g.Wld))) return e;
            if ((e = dalloc(&h->d_Wr, (size_t)g.Dp * g.Wld))) return e;
            if ((e = dalloc(&h->d_lrU, (size_t)kLowRankMax * g.D))) return e;
            if ((e = dalloc(&h->d_lrV, (size_t)kLowRankMax * g.D))) return e;
            if ((e = dalloc(&h->d_wfdn, N))) return e;
            if ((e = dalloc(&h->d_wfup, N))) return e;
            if ((e = dalloc(&h->d_w, g.D))) return e;
            if ((e = dalloc(&h->d_phi, 2 * kNPhi))) return e;
            if ((e = dalloc(&h->d_z, L))) return e;
            if ((e = dalloc(&h->d_fix, 4))) return e;
            if ((e = dalloc(&h->d_small, N))) return e;
            if ((e = dalloc(&h->d_idx_up, mb))) return e;
            if ((e = dalloc(&h->d_idx_down, mb))) return e;
            if ((e = dalloc(&h->d_nz, mb))) return e;
            if ((e = dalloc(&h->d_zr0, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->d_zmix, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->d_zwr, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->d_zdtr, mb * kMaxZones))) return e;
            if ((e = dalloc(&h->d_scal, 7 * mb))) return e;
            if ((e = dalloc(&h->d_desc, mb))) return e;
            if ((e = dalloc(&h->d_rca, mb * L))) return e;
            if ((e = dalloc(&h->d_rcr, mb * L))) return e;
            if ((e = dalloc(&h->d_slabrows, mb * L + 64 * (size_t)sosrt_handle::kMaxMixGroupsSets * sosrt_handle::kMaxGroups))) return e;   // + padding
            if ((e = dalloc(&h->d_slabtilegroup, mb * L / 32 + 2 * sosrt_handle::kMaxMixGroupsSets * sosrt_handle::kMaxGroups + 2))) return e;
            if ((e = dalloc(&h->d_mainrows, mb * L))) return e;
            if ((e = dalloc(&h->d_tau, mb * L))) return e;
            if ((e = dalloc(&h->d_P0a, mb * g.D))) return e;
            if ((e = dalloc(&h->d_P0r, mb * g.D))) return e;
            if ((e = dalloc(&h->d_Jn, fe))) return e;
            if ((e = dalloc(&h->d_InA, fe))) return e;
            if ((e = dalloc(&h->d_InB, fe))) return e;
            if ((e = dalloc(&h->d_I, fe))) return e;
            if ((e = dalloc(&h->d_E, fe))) return e;
            if ((e = dalloc(&h->d_active, mb))) return e;
            if ((e = dalloc(&h->d_norders, mb))) return e;
            if ((e = dalloc(&h->d_status, mb))) return e;
            if ((e = dalloc(&h->d_nactive_sets, 2 * (sosrt_handle::kMaxGroups + 1)))) return e;   // live columns per group; any column needs k_smallmu
            HIPCHK(hipMemset(h->d_nactive_sets, 0, 2 * (sosrt_handle::kMaxGroups + 1) * sizeof(int)));
            h->d_nactive = h->d_nactive_sets;
            if ((e = dalloc(&h->d_redo, mb))) return e;
            if ((e = dalloc(&h->d_erep, mb))) return e;
            if ((e = dalloc(&h->d_mixgroup, mb))) return e;
            if ((e = dalloc(&h->d_livelist, mb))) return e;
            if ((e = dalloc(&h->d_mixca, sosrt_handle::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->d_mixcr, sosrt_handle::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->d_mixset, sosrt_handle::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->d_mixatm, sosrt_handle::kMaxMixGroupsSets))) return e;
            if ((e = dalloc(&h->d_colatm, mb))) return e;
            if ((e = dalloc(&h->d_tauhash, mb))) return e;
            if ((e = dalloc(&h->d_ratio, mb))) return e;
            if ((e = dalloc(&h->d_scan_scratch, mb * transport_scan_scratch_doubles()))) return e;
            if ((e = dalloc(&h->d_scan_sync, 2 * mb))) return e;
            if ((e = dalloc(&h->d_olsync, sosrt_handle::kMaxGroups * order_loop_sync_ints(kOrderLoopMaxCols)))) return e;
            HIPCHK(hipHostMalloc((void**)&h->h_oldone, 2 * sosrt_handle::kMaxGroups * sizeof(int), hipHostMallocCoherent));
            memset(h->h_oldone, 0, 2 * sosrt_handle::kMaxGroups * sizeof(int));
            HIPCHK(hipMemset(h->d_scan_sync, 0, 2 * mb * sizeof(int)));
            HIPCHK(hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, device));
            // + 2 ints at the end: {needs k_smallmu, tag} published at the start of a solve
            HIPCHK(hipHostMalloc((void**)&h->h_pub, (8 * sosrt_handle::kMaxGroups + 2) * sizeof(int), hipHostMallocCoherent));
            memset(h->h_pub, 0, (8 * sosrt_handle::kMaxGroups + 2) * sizeof(int));

            HIPCHK(hipMemset(h->d_Wa, 0, (size_t)g.Dp * g.Wld * sizeof(double)));
            HIPCHK(hipMemset(h->d_Wr, 0, (size_t)g.Dp * g.Wld * sizeof(double)));
            HIPCHK(hipMemset(h->d_status, 0, mb * sizeof(int)));
            HIPCHK(hipMemset(h->d_redo, 0, mb * sizeof(int)));
            HIPCHK(hipMemset(h->d_tau, 0, mb * L * sizeof(double)));
            return 0;
        };
        if ((e = body())) { sosrt_destroy(h); return e; }
        g.mu = h->d_mu; g.Wa = h->d_Wa; g.Wr = h->d_Wr; g.fix = h->d_fix; g.small_lanes = h->d_small;
        g.wflux_dn = h->d_wfdn; g.wflux_up = h->d_wfup; g.nsmall = 0;
    }
    *out = h;
    return 0;
}

int sosrt_destroy(sosrt_t* h) {
    if (!h) return 0;
    if (h->gpu) {
        hipSetDevice(h->device);
        if (h->comm) { rccl().CommDestroy(h->comm); h->comm = nullptr; }
        if (h->own_stream) hipStreamSynchronize(h->own_stream);
        void* ptrs[] = {h->d_mu, h->d_Wa, h->d_Wr, h->d_wfdn, h->d_wfup, h->d_fix, h->d_small, h->d_idx_up,
                        h->d_idx_down, h->d_scal, h->d_desc, h->d_rca, h->d_rcr, h->d_slabrows, h->d_mainrows, h->d_tau, h->d_P0a,
                        h->d_P0r, h->d_Jn, h->d_InA, h->d_InB, h->d_I, h->d_E, h->d_active, h->d_norders, h->d_status,
                        h->d_nactive_sets, h->d_ratio, h->d_redo, h->d_erep, h->d_tauhash, h->d_Wmix, h->d_mixca, h->d_mixcr,
                        h->d_mixgroup, h->d_Wa_s, h->d_Wr_s, h->d_Wmix_s, h->d_scan_scratch, h->d_scan_sync, h->d_w, h->d_phi, h->d_z, h->d_tab, h->d_slabtilegroup, h->d_livelist, h->d_Wa32, h->d_Wmix32, h->d_nz, h->d_zr0, h->d_zmix, h->d_zwr, h->d_zdtr, h->d_olsync, h->d_ollog, h->d_modetab, h->d_lrU, h->d_lrV, h->d_Wrsets, h->d_Wrsets_s, h->d_mixset, h->d_P0rz,
                        h->d_Wasets, h->d_lrUsets, h->d_lrVsets, h->d_lrranks, h->d_colatm, h->d_mixatm};
        for (void* p : ptrs)
            if (p) hipFree(p);
        if (h->h_pub) hipHostFree(h->h_pub);
        if (h->h_oldone) hipHostFree(h->h_oldone);
        if (h->d_mie) hipFree(h->d_mie);
        if (h->h_mie) hipHostFree(h->h_mie);
        if (h->mie_ev) hipEventDestroy(h->mie_ev);
        for (auto& e : h->mie_t)
            if (e) hipEventDestroy(e);

        for (auto& p : h->prof)
            for (auto& e : p.ev) hipEventDestroy(e);
        if (h->stream2) { hipStreamSynchronize(h->stream2); hipStreamDestroy(h->stream2); }
        if (h->ev_fork) hipEventDestroy(h->ev_fork);
        if (h->ev_join) hipEventDestroy(h->ev_join);
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
    if (mode == SOSRT_FIRST_ORDER_README && (h->nsets > 1 || h->p0_zones > 0))
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one aerosol matrix: it cannot be combined with several phase sets");
    if (mode == SOSRT_FIRST_ORDER_README && (h->natm > 1 || h->max_atm_used > 0))
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with atmosphere phase sets");
    if (mode == SOSRT_FIRST_ORDER_README && h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "the README's Lambertian first order needs the three-zone geometry (it has a surface)");
    h->first_order_mode = mode;
    return 0;
}

int sosrt_set_contraction(sosrt_t* h, int mode) {
    if (int e = need_gpu(h)) return e;
    if (mode != SOSRT_CONTRACT_F64 && mode != SOSRT_CONTRACT_F32 && mode != SOSRT_CONTRACT_F64_FULL && mode != SOSRT_CONTRACT_F64_DENSE) return fail(SOSRT_E_INVALID, "unknown contraction mode %d", mode);
    if (mode != SOSRT_CONTRACT_F64 && (h->natm > 1 || h->max_atm_used > 0))
        return fail(SOSRT_E_INVALID, "atmosphere phase sets are in use: their plain rows exist in the low-rank form of SOSRT_CONTRACT_F64 only "
                                     "(the other contractions tile row lists that straddle columns)");
    if (mode == SOSRT_CONTRACT_F32) {
        HIPCHK(hipSetDevice(h->device));
        const size_t per = (size_t)h->g.Dp * h->g.Wld;
        if (!h->d_Wa32) { if (int e = dalloc(&h->d_Wa32, per)) return e; }
        h->w32_dirty = true;
    }
    h->contraction = mode;
    return 0;
}

int sosrt_set_order_loop(sosrt_t* h, int mode) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (mode < 0 || mode > 2) return fail(SOSRT_E_INVALID, "order-loop mode must be 0, 1 or 2 (got %d)", mode);
    h->order_loop = mode;
    return 0;
}

int sosrt_order_loop_stats(sosrt_t* h, int* launches, int* refused, long long* column_orders) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (launches) *launches = h->ol_launches;
    if (refused) *refused = h->ol_refused;
    if (column_orders) {
        *column_orders = 0;
        if (h->gpu && h->ol_launches > 0) {             // every launch of the last solve left its count in its group's words
            HIPCHK(hipSetDevice(h->device));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
            for (int k = 0; k < sosrt_handle::kMaxGroups; ++k) {
                if (!h->ol_group_used[k]) continue;
                int v = 0;
                HIPCHK(hipMemcpy(&v, h->d_olsync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols) + kOlOrders, sizeof v, hipMemcpyDeviceToHost));
                *column_orders += v;
            }
        }
    }
    return 0;
}

int sosrt_plan_launch(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int* out) {
    if (!h || !out) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (batch < 1 || live < 0 || live > batch) return fail(SOSRT_E_INVALID, "need 0 <= live <= batch, batch >= 1");
    if (zones < 1 || zones > kMaxZones) return fail(SOSRT_E_INVALID, "zones must be in 1..%d", kMaxZones);
    // as sosrt_set_columns and the order loop of sosrt_solve_dev see a batch of `batch` (clear, slab, clear)-like columns with up to
    // `zones` zones: the column groups, then the plan of an order of the first group with `live` columns of it live
    int want = h->want_groups;
    if (want == 0) want = batch > h->split_min ? 2 : 1;
    const int ng = (want >= 2 && batch >= h->split_min && batch >= 2) ? 2 : 1;
    const int nb = ng == 2 ? batch / 2 : batch;
    const int saved_cus = h->cu_count;
    if (cus > 0) h->cu_count = cus;
    const SolveShape sh = solve_shape(h, zones);
    OrderInputs oi;
    oi.nb = nb; oi.known = live < nb ? live : nb; oi.surface = surface;
    oi.simple_zones = zones == 3 || zones == 1;
    oi.cu_share = h->cu_count / ng;
    const bool saved_sym = h->sym_ok;
    if (!h->have_phase) h->sym_ok = true;            // (no matrices yet: plan for flip-symmetric ones, what every phase function of the scattering angle gives)
    const LaunchPlan pl = plan_order(h, sh, oi);
    h->sym_ok = saved_sym;
    h->cu_count = saved_cus;
    out[0] = ng; out[1] = pl.gemm; out[2] = pl.tail_cols; out[3] = pl.transport; out[4] = pl.parts; out[5] = pl.repair;
    out[6] = pl.order_loop; out[7] = pl.ol_parts; out[8] = pl.ol_grid;
    return 0;
}

int sosrt_phase_asymmetry(sosrt_t* h, double* asymmetry, int* uses_symmetry) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (asymmetry) *asymmetry = h->asymmetry;
    if (uses_symmetry) *uses_symmetry = use_sym(h) ? 1 : 0;
    return 0;
}

int sosrt_phase_rank(sosrt_t* h, int* rank, double* residual, int* uses) {
    if (!h) return fail(SOSRT_E_INVALID, "null handle");
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (rank) *rank = h->lr_rank;
    if (residual) *residual = h->lr_residual;
    if (uses) *uses = use_lowrank(h) ? 1 : 0;
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
    h->fast_ok = transport_fast_ok(h->plan);
    if (h->gpu) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpy(h->d_mu, mu, h->D * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_wfdn, h->plan.wflux_dn.data(), h->N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_wfup, h->plan.wflux_up.data(), h->N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_w, h->plan.w.data(), h->D * sizeof(double), hipMemcpyHostToDevice));
        {   // phi = np.linspace(0, pi, 25) (phase:81-82): cos(phi0 - phi) and the trapezoid weights of np.trapz(., phi)
            double phi[kNPhi], tab[2 * kNPhi];
            const double step = 3.141592653589793 / (kNPhi - 1);
            for (int q = 0; q < kNPhi; ++q) phi[q] = q * step;
            phi[kNPhi - 1] = 3.141592653589793;
            for (int q = 0; q < kNPhi; ++q) {
                tab[q] = std::cos(0 - phi[q]);
                tab[kNPhi + q] = ((q > 0 ? phi[q] - phi[q - 1] : 0.0) + (q + 1 < kNPhi ? phi[q + 1] - phi[q] : 0.0)) / 2;
            }
            HIPCHK(hipMemcpy(h->d_phi, tab, sizeof tab, hipMemcpyHostToDevice));
        }
        std::vector<FixTab> ft(4);
        for (int b = 0; b < 4; ++b) {
            const FixTable& t = h->plan.fix[b];
            memset(&ft[b], 0, sizeof(FixTab));
            ft[b].idx = t.idx; ft[b].s0 = t.s0; ft[b].ns = t.ns;
            for (size_t i = 0; i < t.C.size(); ++i) ft[b].C[i] = t.C[i];
        }
        HIPCHK(hipMemcpy(h->d_fix, ft.data(), 4 * sizeof(FixTab), hipMemcpyHostToDevice));
        h->g.nsmall = (int)h->plan.small_lanes.size();
        if (h->g.nsmall)
            HIPCHK(hipMemcpy(h->d_small, h->plan.small_lanes.data(), h->g.nsmall * sizeof(int), hipMemcpyHostToDevice));
    }
    // which kernels take this shape (pure functions of the grid: a host-only handle answers sosrt_plan_launch with them)
    h->g.nsmall = (int)h->plan.small_lanes.size();
    h->ring_ok = h->fast_ok && transport_ring_ok(h->g);
    h->scan_ok = h->ring_ok && transport_scan_ok(h->g);
    // (N in (128, 256]: the chunk-parallel kernel has this form only; it does not need the ring kernel's shape -- odd N, N up to
    // 512 and L up to 1024 take its WIDE instantiation: the reference's shipped N = 501, L = 800)
    // (nor the condition of the wave-independent kernels that the rewritten mu -> 0- directions and their sources sit in the last
    // wave of a half row: part 0 of the split form holds the downward directions N-64 .. N-1 in ONE wave whatever N is)
    h->scan_split_ok = transport_scan_split_ok(h->g);
    return 0;
}

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

static int mix_group_cap(const sosrt_handle* h, bool sets);
// Common part of sosrt_set_phase / sosrt_set_phase_sets[_dev]: S aerosol matrices [S][2N][2N] (S = 0: none), host (P_aer) or
// device (d_P_aer: folded and measured on the device, in the handle's stream order; the host keeps no copy of their folds
// until sosrt_plan_fold asks for one)
static int set_phase_impl(sosrt_handle* h, const double* P_atm, int S, const double* P_aer, const double* d_P_aer = nullptr) {
    if (!h || !P_atm) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (h->have_cols && h->max_set_used >= (S > 0 ? S : 1))
        return fail(SOSRT_E_INVALID, "the current columns use aerosol set %d, but only %d set(s) are given (sosrt_set_columns resets them to set 0)",
                    h->max_set_used, S > 0 ? S : 1);
    if (S > 1 && h->first_order_mode == SOSRT_FIRST_ORDER_README)
        return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one aerosol matrix: it cannot be combined with %d phase sets", S);
    if (h->have_cols && h->max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "the current columns use atmosphere set %d, and sosrt_set_phase leaves one atmosphere set (sosrt_set_columns resets them to set 0)",
                    h->max_atm_used);
    const size_t DD = (size_t)h->D * h->D;
    h->plan.fold(P_atm, h->Wa_h);
    h->have_aer = S > 0;
    h->wr_on_device = d_P_aer != nullptr;
    if (S > 0 && !d_P_aer) h->plan.fold(P_aer, h->Wr_h);
    else h->Wr_h.clear();
    h->Wrx_h.clear();
    h->Wrx_h.resize(S > 1 ? S - 1 : 0);
    for (int q = 1; q < S && !d_P_aer; ++q) h->plan.fold(P_aer + (size_t)q * DD, h->Wrx_h[q - 1]);
    h->nsets = S > 1 ? S : 1;
    h->natm = 1;
    h->have_phase = true;
    h->mix_dirty = true;
    h->w32_dirty = true;
    h->sym_dirty = true; h->symmix_dirty = true; h->symsets_dirty = true;
    {   // flip symmetry of the folded matrices (see sosrt.h, sosrt_set_contraction): the maximum over W_atm and every set
        const int D = h->D;
        h->asymmetry = 0;
        std::vector<const std::vector<double>*> all = {&h->Wa_h, &h->Wr_h};
        for (const auto& W : h->Wrx_h) all.push_back(&W);
        for (const std::vector<double>* W : all) {
            if (W->empty()) continue;
            const double r = flip_asymmetry(*W, D);
            if (!(r <= h->asymmetry)) h->asymmetry = r;
        }
        // (a compile-time constant: nothing in the environment can put the symmetric form on a matrix without the symmetry)
        h->sym_ok = h->asymmetry <= SOSRT_SYMMETRY_TOL;      // (device sets: their measure joins below)
    }
    // low rank of W_atm (see sosrt.h, sosrt_phase_rank): from the matrix alone, never from the batch
    std::vector<double> lrU, lrV;
    h->lr_rank = lowrank_factor(h->Wa_h, h->D, lrU, lrV, &h->lr_residual);
    if (h->gpu) {
        HIPCHK(hipSetDevice(h->device));
        const Grid& g = h->g;
        HIPCHK(hipMemcpy2D(h->d_Wa, g.Wld * sizeof(double), h->Wa_h.data(), g.D * sizeof(double), g.D * sizeof(double),
                           g.D, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_lrU, lrU.data(), lrU.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_lrV, lrV.data(), lrV.size() * sizeof(double), hipMemcpyHostToDevice));
        if (S > 0 && !d_P_aer)
            HIPCHK(hipMemcpy2D(h->d_Wr, g.Wld * sizeof(double), h->Wr_h.data(), g.D * sizeof(double),
                               g.D * sizeof(double), g.D, hipMemcpyHostToDevice));
        if (d_P_aer) {
            // fold and asymmetry measure on the device: the matrices never visit the host, two partial maxima per block do
            constexpr int kAsymBlocks = 32;
            const size_t per = (size_t)g.Dp * g.Wld, scratch = (size_t)2 * kAsymBlocks * S;
            if (per * S + scratch > h->wrsets_capacity) {
                if (h->d_Wrsets) hipFree(h->d_Wrsets);       // (hipFree synchronises: no launch still reads it)
                h->d_Wrsets = nullptr; h->wrsets_capacity = 0;
                if (int e = dalloc(&h->d_Wrsets, per * S + scratch)) return e;
                h->wrsets_capacity = per * S + scratch;
            }
            hipStream_t s = h->stream;
            double* d_part = h->d_Wrsets + per * S;
            HIPCHK(hipMemsetAsync(h->d_Wrsets, 0, per * S * sizeof(double), s));       // the padding rows and columns stay zero
            launch_fold_sets(s, S, g.D, g.Wld, per, h->d_w, d_P_aer, h->d_Wrsets);
            launch_fold_asymmetry(s, S, kAsymBlocks, g.D, g.Wld, per, h->d_Wrsets, d_part);
            HIPCHK(hipMemcpyAsync(h->d_Wr, h->d_Wrsets, per * sizeof(double), hipMemcpyDeviceToDevice, s));
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
                if (!(r <= h->asymmetry)) h->asymmetry = r;
            }
            h->sym_ok = h->asymmetry <= SOSRT_SYMMETRY_TOL;
        } else if (S > 1) {
            const size_t per = (size_t)g.Dp * g.Wld;
            if (per * S > h->wrsets_capacity) {
                if (h->d_Wrsets) hipFree(h->d_Wrsets);       // (hipFree synchronises: no launch still reads it)
                h->d_Wrsets = nullptr; h->wrsets_capacity = 0;
                if (int e = dalloc(&h->d_Wrsets, per * S)) return e;
                h->wrsets_capacity = per * S;
            }
            HIPCHK(hipMemset(h->d_Wrsets, 0, per * S * sizeof(double)));       // the padding rows and columns stay zero
            for (int q = 0; q < S; ++q)
                HIPCHK(hipMemcpy2D(h->d_Wrsets + q * per, g.Wld * sizeof(double), (q ? h->Wrx_h[q - 1] : h->Wr_h).data(),
                                   g.D * sizeof(double), g.D * sizeof(double), g.D, hipMemcpyHostToDevice));
        }
    }
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
    out[0] = h->nsets;
    out[1] = h->have_cols ? h->mix_groups : 0;
    out[2] = (h->have_cols && (h->nslab == 0 || h->mix_groups > 0)) ? 1 : 0;
    out[3] = h->have_grid ? mix_group_cap(h, true) : 0;
    return 0;
}

// Combined-matrix groups of the current columns: the distinct (atmosphere set, aerosol set, ca, cr) of their aerosol zones
// (spec:321: (w_atm/4) f_atm on W_atm, (w_aer/4) f_aer on W_aer), per (column, slab).
struct MixGroups {
    std::vector<double> ca, cr;
    std::vector<int> set, gid /*[B][kMaxZones], -1: clear zone*/, gcol /*[B]: the live-column tilings, one slab per column*/;
    std::vector<int> atm;                // atmosphere set of a group (sosrt_set_atmosphere_sets; all 0 otherwise)
};
// groups the cache may hold: kMaxMixGroups while every column uses set 0 (what it always held), more with several sets in use
static int mix_group_cap(const sosrt_handle* h, bool sets) {
    if (h->mix_groups_max < sosrt_handle::kMaxMixGroups) return h->mix_groups_max < 0 ? 0 : h->mix_groups_max;
    if (!sets) return sosrt_handle::kMaxMixGroups;
    const size_t per = (size_t)h->g.Dp * h->g.Wld * sizeof(double);
    size_t n = per ? sosrt_handle::kMixCacheBytes / per : 0;
    if (n > (size_t)sosrt_handle::kMaxMixGroupsSets) n = sosrt_handle::kMaxMixGroupsSets;
    if (n < (size_t)sosrt_handle::kMaxMixGroups) n = sosrt_handle::kMaxMixGroups;
    if (n > (size_t)h->mix_groups_max) n = h->mix_groups_max;
    return (int)n;
}
// false: more than `cap` groups
static bool collect_mix_groups(const sosrt_handle* h, int B, const std::vector<int>& zset, const std::vector<int>& aset, int cap,
                               MixGroups& mg) {
    mg.gid.assign((size_t)B * kMaxZones, -1);
    mg.gcol.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        for (int z = 0; z < h->c_nz[b]; ++z) {
            if (!h->c_zmix[b * kMaxZones + z]) continue;
            const double da = h->c_dtau_atm[b], dr = h->c_zdtr[b * kMaxZones + z];
            const double ca = (h->c_alb_atm[b] / 4) * (da / (da + dr)), cr = (h->c_zwr[b * kMaxZones + z] / 4) * (dr / (da + dr));
            const int st = zset[b * kMaxZones + z], at = aset[b];
            int k = 0;
            while (k < (int)mg.ca.size() && !(mg.ca[k] == ca && mg.cr[k] == cr && mg.set[k] == st && mg.atm[k] == at)) ++k;
            if (k == (int)mg.ca.size()) {
                if (k == cap) return false;
                mg.ca.push_back(ca); mg.cr.push_back(cr); mg.set.push_back(st); mg.atm.push_back(at);
            }
            mg.gid[b * kMaxZones + z] = k;
            mg.gcol[b] = k;
        }
    }
    return true;
}
// uploads the groups and lists the slab rows of the dense contraction group by group.  A failed allocation of the cache leaves
// the two-pass form (mix_groups = 0) over the row lists as sosrt_set_columns wrote them -- a choice that is only open while
// every column uses set 0, so with sets in use it is an error.
static int apply_mix_groups(sosrt_handle* h, int B, const MixGroups& mg) {
    const int L = h->L;
    const std::vector<int>&nz = h->c_nz, &zr0 = h->c_zr0;
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    const size_t per = (size_t)h->g.Dp * h->g.Wld, need = per * mg.ca.size();
    if (need > h->mix_capacity) {
        if (h->d_Wmix) hipFree(h->d_Wmix);
        h->d_Wmix = nullptr; h->mix_capacity = 0;
        if (hipMalloc((void**)&h->d_Wmix, need * sizeof(double)) == hipSuccess) h->mix_capacity = need;
        else (void)hipGetLastError();
    }
    if (h->mix_capacity < need) {
        if (h->max_set_used > 0 || h->max_atm_used > 0) {
            h->have_cols = false;
            return fail(SOSRT_E_NOMEM, "no memory for the %zu combined matrices of a batch with several phase sets", mg.ca.size());
        }
        return 0;
    }
    HIPCHK(hipMemcpy(h->d_mixca, mg.ca.data(), mg.ca.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mixcr, mg.cr.data(), mg.cr.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mixset, mg.set.data(), mg.set.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mixatm, mg.atm.data(), mg.atm.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mixgroup, mg.gcol.data(), B * sizeof(int), hipMemcpyHostToDevice));
    h->mix_groups = (int)mg.ca.size();
    // slab rows of the dense contraction listed, per column group of the order loop, group by group, every group padded
    // to whole 32-row tiles
    std::vector<int> grouped, tilegroup;
    for (int cg = 0; cg < h->ngroups; ++cg) {
        for (int k = 0; k < h->mix_groups; ++k) {
            for (int b = h->gb[cg]; b < h->gb[cg + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    if (mg.gid[b * kMaxZones + z] == k)
                        for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) grouped.push_back(b * L + t);
            while (grouped.size() % 64) grouped.push_back(-1);   // whole 64-row tiles (two 32-row tiles of the same group)
            while (tilegroup.size() < grouped.size() / 32) tilegroup.push_back(k);
        }
        h->slab_off[cg + 1] = (int)grouped.size();
    }
    HIPCHK(hipMemcpy(h->d_slabrows, grouped.data(), grouped.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_slabtilegroup, tilegroup.data(), tilegroup.size() * sizeof(int), hipMemcpyHostToDevice));
    h->nslab = (int)grouped.size();
    h->mix_dirty = true;
    h->w32_dirty = true;
    return 0;
}

// Common part of sosrt_set_columns / sosrt_set_columns_zones: zone tables [B][kMaxZones] (host), per-column scalars.
static int set_columns_impl(sosrt_handle* h, int B, int geometry, int surface, const std::vector<int>& nz,
                            const std::vector<int>& zr0, const std::vector<int>& zmix, const std::vector<double>& zwr,
                            const std::vector<double>& zdtr, const double* mu0, const double* grd_alb, const double* alb_atm,
                            const double* dtau_atm, const double* tauStar_tot) {
    const size_t mb = h->max_batch;
    const int L = h->L;
    h->resident = false;                     // the descriptors of the resident field's columns are about to change
    std::vector<double> sc(7 * mb, 0.0);
    std::vector<int> slab, plain, iup(B, 0), idn(B, 0);
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    // column groups of the order loop: two contiguous halves for a large batch
    // (auto: two groups for a batch of more than SPLIT_MIN columns (48; 256 in round 3).  Round 3, EVA / wildfire sweeps with one and two groups
    // alternating on one box: 288 x (200, 128) 3.65 -> 3.33 ms, 320 x 3.89 -> 3.50, 512 x 5.03 -> 4.75, 1024 x 9.2 -> 8.15,
    // 2048 x 16.6 -> 15.5, 4096 x 32.4 -> 30.3; 512 x (200, 64) 3.02 -> 2.94, 1024 x (200, 64) 5.10 -> 4.69; 512 x (200, 256)
    // 13.1 -> 12.65, 512 x (400, 256) 13.5 -> 12.8, 4096 x (400, 256) 106 -> 103.7; 256 x (200, 128) unchanged.  The gain is the
    // MFMA-bound contraction of one half running beside the HBM-bound transport of the other; the HBM bytes of a solve are the same
    // either way: 17.6 vs 18.0 GB by PMC)
    int want = h->want_groups;
    if (want == 0) want = B > h->split_min ? 2 : 1;
    h->ngroups = (want >= 2 && B >= h->split_min && B >= 2) ? 2 : 1;
    if (h->ngroups > 1 && !h->stream2) {
        HIPCHK(hipSetDevice(h->device));
        if (h->prio2) {
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, h->prio2 > 0 ? greatest : least));
        } else {
            HIPCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        }
    }
    h->gb[0] = 0; h->gb[1] = h->ngroups == 2 ? ((h->split_at > 0 && h->split_at < B) ? h->split_at : B / 2) : B; h->gb[2] = B;
    for (int k = 0; k <= sosrt_handle::kMaxGroups; ++k) { h->main_off[k] = 0; h->slab_off[k] = 0; }
    h->max_nz = 1;
    h->simple_zones = true;                  // every column is (clear, slab, clear): the live-column tilings apply
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        for (int b = 0; b < B; ++b) {
            h->max_nz = nz[b] > h->max_nz ? nz[b] : h->max_nz;
            const int* m = &zmix[b * kMaxZones];
            if (!(nz[b] == 3 && m[0] == 0 && m[1] == 1 && m[2] == 0)) h->simple_zones = false;
            if (nz[b] == 3) { iup[b] = zr0[b * kMaxZones + 1]; idn[b] = zr0[b * kMaxZones + 2] - 1; }
        }
        for (int k = 0; k < h->ngroups; ++k) {
            for (int b = h->gb[k]; b < h->gb[k + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) (zmix[b * kMaxZones + z] ? slab : plain).push_back(b * L + t);
            h->main_off[k + 1] = (int)plain.size();
            h->slab_off[k + 1] = (int)slab.size();
        }
    }
    for (int b = 0; b < B; ++b) {
        if (!(mu0[b] > 0)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be > 0", b);
        sc[0 * mb + b] = mu0[b];
        sc[1 * mb + b] = grd_alb ? grd_alb[b] : 0.0;
        sc[2 * mb + b] = alb_atm[b];
        sc[4 * mb + b] = dtau_atm ? dtau_atm[b] : 1.0;
        sc[6 * mb + b] = tauStar_tot[b];
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_scal, sc.data(), 7 * mb * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        HIPCHK(hipMemcpyAsync(h->d_nz, nz.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_zr0, zr0.data(), (size_t)B * kMaxZones * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_zmix, zmix.data(), (size_t)B * kMaxZones * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_zwr, zwr.data(), (size_t)B * kMaxZones * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_zdtr, zdtr.data(), (size_t)B * kMaxZones * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_idx_up, iup.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_idx_down, idn.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!slab.empty())
            HIPCHK(hipMemcpyAsync(h->d_slabrows, slab.data(), slab.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!plain.empty())
            HIPCHK(hipMemcpyAsync(h->d_mainrows, plain.data(), plain.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // the staging vectors go out of scope
    h->nslab = (int)slab.size();
    h->nmain = (int)plain.size();
    h->max_main = L; h->max_slab = 0;
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        h->max_main = 0;
        for (int b = 0; b < B; ++b) {
            int ns = 0;
            for (int z = 0; z < nz[b]; ++z)
                if (zmix[b * kMaxZones + z]) ns += zone_end(b, z) - zr0[b * kMaxZones + z] + 1;
            h->max_slab = ns > h->max_slab ? ns : h->max_slab;
            h->max_main = L - ns > h->max_main ? L - ns : h->max_main;
        }
    }
    h->mix_groups = 0;
    h->mix_dirty = true;
    h->w32_dirty = true;
    // every column starts on aerosol set 0 (sosrt_set_aerosol_sets changes that), P0_aer is one row per column
    h->max_set_used = 0;
    h->max_atm_used = 0;                     // ... and on atmosphere set 0 (sosrt_set_atmosphere_sets)
    h->c_atmset.assign(B, 0);
    h->p0_zones = 0;
    h->c_nz = nz; h->c_zr0 = zr0; h->c_zmix = zmix; h->c_zwr = zwr; h->c_zdtr = zdtr;
    h->c_zset.assign((size_t)B * kMaxZones, 0);
    h->c_alb_atm.assign(alb_atm, alb_atm + B);
    h->c_dtau_atm.assign(B, 1.0);
    if (dtau_atm) h->c_dtau_atm.assign(dtau_atm, dtau_atm + B);
    if (geometry == SOSRT_GEOM_THREE_ZONE && h->nslab > 0) {
        MixGroups mg;
        if (collect_mix_groups(h, B, h->c_zset, h->c_atmset, mix_group_cap(h, false), mg))
            if (int e = apply_mix_groups(h, B, mg)) return e;
    }
    h->B = B; h->geom = geometry; h->surface = surface;
    h->have_cols = true;
    return 0;
}

int sosrt_set_columns(sosrt_t* h, int B, int geometry, int surface, const int* idx_up, const int* idx_down,
                      const double* mu0, const double* grd_alb, const double* alb_atm, const double* alb_aer,
                      const double* dtau_atm, const double* dtau_aer, const double* tauStar_tot) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || B > h->max_batch) return fail(SOSRT_E_INVALID, "B=%d outside 1..max_batch=%d", B, h->max_batch);
    if (!mu0 || !alb_atm || !tauStar_tot) return fail(SOSRT_E_INVALID, "mu0, alb_atm and tauStar_tot are required");
    std::vector<int> nz(B, 1), zr0((size_t)B * kMaxZones, 0), zmix((size_t)B * kMaxZones, 0);
    std::vector<double> zwr((size_t)B * kMaxZones, 0.0), zdtr((size_t)B * kMaxZones, 0.0);
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        if (!idx_up || !idx_down || !grd_alb || !alb_aer || !dtau_atm || !dtau_aer)
            return fail(SOSRT_E_INVALID, "three-zone geometry needs idx_up, idx_down, grd_alb, alb_aer, dtau_atm, dtau_aer");
        if (surface != SOSRT_SURFACE_SPECULAR && surface != SOSRT_SURFACE_LAMBERTIAN && surface != SOSRT_SURFACE_LAMBERTIAN_README)
            return fail(SOSRT_E_INVALID, "three-zone geometry needs a specular or lambertian surface");
        for (int b = 0; b < B; ++b) {
            if (idx_up[b] < 1 || idx_down[b] < idx_up[b] || idx_down[b] > h->L - 2)
                return fail(SOSRT_E_INVALID, "column %d: need 1 <= idx_up <= idx_down <= nb_layers-2 (got %d, %d)", b,
                            idx_up[b], idx_down[b]);
            // above / inside / below the aerosol slab (spec:113-449)
            nz[b] = 3;
            zr0[b * kMaxZones + 1] = idx_up[b]; zr0[b * kMaxZones + 2] = idx_down[b] + 1;
            zmix[b * kMaxZones + 1] = 1;
            zwr[b * kMaxZones + 1] = alb_aer[b];
            zdtr[b * kMaxZones + 1] = dtau_aer[b];
        }
    } else if (geometry == SOSRT_GEOM_SINGLE_SLAB) {
        surface = SOSRT_SURFACE_NONE;
    } else {
        return fail(SOSRT_E_INVALID, "unknown geometry %d", geometry);
    }
    return set_columns_impl(h, B, geometry, surface, nz, zr0, zmix, zwr, zdtr, mu0, grd_alb, alb_atm, dtau_atm, tauStar_tot);
}

int sosrt_set_columns_zones(sosrt_t* h, int B, int surface, int nzmax, const int* nz_in, const int* zone_r0, const int* zone_mix,
                            const double* mu0, const double* grd_alb, const double* alb_atm, const double* dtau_atm,
                            const double* zone_alb_aer, const double* zone_dtau_aer, const double* tauStar_tot) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || B > h->max_batch) return fail(SOSRT_E_INVALID, "B=%d outside 1..max_batch=%d", B, h->max_batch);
    if (!nz_in || !zone_r0 || !zone_mix || !mu0 || !grd_alb || !alb_atm || !dtau_atm || !zone_alb_aer || !zone_dtau_aer || !tauStar_tot)
        return fail(SOSRT_E_INVALID, "null argument");
    if (nzmax < 1 || nzmax > kMaxZones) return fail(SOSRT_E_INVALID, "nzmax must be in 1..%d (got %d)", kMaxZones, nzmax);
    if (surface != SOSRT_SURFACE_SPECULAR && surface != SOSRT_SURFACE_LAMBERTIAN && surface != SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "a zone table needs a specular or lambertian surface");
    std::vector<int> nz(B), zr0((size_t)B * kMaxZones, 0), zmix((size_t)B * kMaxZones, 0);
    std::vector<double> zwr((size_t)B * kMaxZones, 0.0), zdtr((size_t)B * kMaxZones, 0.0);
    for (int b = 0; b < B; ++b) {
        nz[b] = nz_in[b];
        if (nz[b] < 1 || nz[b] > nzmax) return fail(SOSRT_E_INVALID, "column %d: %d zones, expected 1..%d", b, nz[b], nzmax);
        for (int z = 0; z < nz[b]; ++z) {
            const int r0 = zone_r0[b * nzmax + z], mix = zone_mix[b * nzmax + z] != 0;
            if (z == 0 ? r0 != 0 : !(r0 > zr0[b * kMaxZones + z - 1] && r0 < h->L))
                return fail(SOSRT_E_INVALID, "column %d: zone %d starts at row %d (zones start at 0 and ascend, below nb_layers)", b, z, r0);
            if (z > 0 && mix && zmix[b * kMaxZones + z - 1]) return fail(SOSRT_E_INVALID, "column %d: two adjacent aerosol zones (%d, %d): merge them", b, z - 1, z);
            // the reference's slab lies strictly inside the column (idx_up >= 1, idx_down <= L-2, spec:40): its formulas
            // read the rows either side of a slab
            if (mix && (z == 0 || z == nz[b] - 1)) return fail(SOSRT_E_INVALID, "column %d: an aerosol zone must have a clear zone above and below it", b);
            zr0[b * kMaxZones + z] = r0; zmix[b * kMaxZones + z] = mix;
            zwr[b * kMaxZones + z] = mix ? zone_alb_aer[b * nzmax + z] : 0.0;
            zdtr[b * kMaxZones + z] = mix ? zone_dtau_aer[b * nzmax + z] : 0.0;
            if (mix && !(zdtr[b * kMaxZones + z] >= 0)) return fail(SOSRT_E_INVALID, "column %d zone %d: dtau_aer must be >= 0", b, z);
        }
    }
    return set_columns_impl(h, B, SOSRT_GEOM_THREE_ZONE, surface, nz, zr0, zmix, zwr, zdtr, mu0, grd_alb, alb_atm, dtau_atm, tauStar_tot);
}

// The slab rows of a batch with more groups than the cache, for the two passes (W_atm, then W_aer).  Every column on set 0:
// column by column, as sosrt_set_columns lists them.  With sets in use: per column group of the order loop set by set, every
// set padded to whole 64-row tiles, so that a tile of the dense tiling has ONE set (d_slabtilegroup: the set of every 32 rows)
// and its second pass reads that set's W_aer; the live-column tilings (columns with one slab) read the set of their column
// (d_mixgroup).
static int apply_two_pass_rows(sosrt_handle* h, int B) {
    const int L = h->L;
    const std::vector<int>&nz = h->c_nz, &zr0 = h->c_zr0;
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    const bool sets = h->max_set_used > 0;
    std::vector<int> slab, tileset, colset(B, 0);
    for (int k = 0; k < h->ngroups; ++k) {
        for (int st = 0; st < (sets ? h->nsets : 1); ++st) {
            for (int b = h->gb[k]; b < h->gb[k + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    if (h->c_zmix[b * kMaxZones + z] && (!sets || h->c_zset[b * kMaxZones + z] == st)) {
                        for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) slab.push_back(b * L + t);
                        colset[b] = st;
                    }
            if (sets) {
                while (slab.size() % 64) slab.push_back(-1);
                while (tileset.size() < slab.size() / 32) tileset.push_back(st);
            }
        }
        h->slab_off[k + 1] = (int)slab.size();
    }
    if (!slab.empty()) HIPCHK(hipMemcpy(h->d_slabrows, slab.data(), slab.size() * sizeof(int), hipMemcpyHostToDevice));
    if (sets) {
        if (!tileset.empty()) HIPCHK(hipMemcpy(h->d_slabtilegroup, tileset.data(), tileset.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_mixgroup, colset.data(), B * sizeof(int), hipMemcpyHostToDevice));
    }
    h->nslab = (int)slab.size();
    h->mix_groups = 0;
    h->mix_dirty = true;
    h->w32_dirty = true;
    return 0;
}

int sosrt_set_aerosol_sets(sosrt_t* h, int B, int nzmax, const int* zone_set) {
    if (!h || !zone_set) return fail(SOSRT_E_INVALID, "null argument");
    if (nzmax < 1 || nzmax > kMaxZones) return fail(SOSRT_E_INVALID, "nzmax must be in 1..%d (got %d)", kMaxZones, nzmax);
    if (B < 1) return fail(SOSRT_E_INVALID, "B=%d must be >= 1", B);
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (int e = need_gpu(h)) return e;
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (B != h->B) return fail(SOSRT_E_INVALID, "B=%d does not match sosrt_set_columns (B=%d)", B, h->B);
    if (h->geom != SOSRT_GEOM_THREE_ZONE) return fail(SOSRT_E_INVALID, "aerosol sets need the three-zone geometry (a single slab has no aerosol)");
    // nzmax = 1: one set per column, for each of its aerosol zones; else one per zone of the caller's table
    std::vector<int> zset((size_t)B * kMaxZones, 0);
    int top = 0;
    for (int b = 0; b < B; ++b) {
        if (nzmax > 1 && h->c_nz[b] > nzmax) return fail(SOSRT_E_INVALID, "column %d has %d zones, nzmax is %d", b, h->c_nz[b], nzmax);
        for (int z = 0; z < h->c_nz[b]; ++z) {
            if (!h->c_zmix[b * kMaxZones + z]) continue;           // entries of clear zones are ignored
            const int st = nzmax == 1 ? zone_set[b] : zone_set[b * nzmax + z];
            if (st < 0 || st >= h->nsets)
                return fail(SOSRT_E_INVALID, "column %d zone %d: aerosol set %d outside 0..%d (sosrt_set_phase_sets)", b, z, st, h->nsets - 1);
            zset[b * kMaxZones + z] = st;
            top = st > top ? st : top;
        }
    }
    MixGroups mg;
    const int cap = mix_group_cap(h, top > 0 || h->max_atm_used > 0);
    // (beyond the cache the slab rows take two passes, W_atm and then the W_aer of their set: apply_two_pass_rows)
    const bool fits = collect_mix_groups(h, B, zset, h->c_atmset, cap, mg);
    if (!fits && h->max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "more than %d distinct (atmosphere set, aerosol set, ca, cr) groups: the two-pass form that a batch beyond the "
                                     "cache takes reads one W_atm, and the current columns use atmosphere sets", cap);
    const bool regroup = top > 0 || h->max_set_used > 0;      // (all on set 0 before and after: the groups sosrt_set_columns built stand)
    h->c_zset = zset;
    h->max_set_used = top;
    h->p0_zones = nzmax > 1 ? nzmax : 0;
    if (regroup && (!fits || !mg.ca.empty())) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (int e = fits ? apply_mix_groups(h, B, mg) : apply_two_pass_rows(h, B)) return e;
    }
    return 0;
}

int sosrt_set_atm_phase_sets(sosrt_t* h, int S_atm, const double* P_atm_sets) {
    if (!h || !P_atm_sets) return fail(SOSRT_E_INVALID, "null argument");
    if (int e = need_gpu(h)) return e;
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called (it defines the aerosol matrices; the atmosphere sets follow it)");
    if (S_atm < 1 || S_atm > SOSRT_MAX_PHASE_SETS)
        return fail(SOSRT_E_INVALID, "S_atm=%d outside 1..SOSRT_MAX_PHASE_SETS=%d", S_atm, SOSRT_MAX_PHASE_SETS);
    if (h->have_cols && h->max_atm_used >= S_atm)
        return fail(SOSRT_E_INVALID, "the current columns use atmosphere set %d, but only %d set(s) are given (sosrt_set_columns resets them to set 0)",
                    h->max_atm_used, S_atm);
    if (S_atm > 1) {
        if (h->contraction != SOSRT_CONTRACT_F64)
            return fail(SOSRT_E_INVALID, "atmosphere phase sets need SOSRT_CONTRACT_F64: their plain rows exist in its low-rank form only "
                                         "(the other contractions tile row lists that straddle columns)");
        if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with %d atmosphere sets", S_atm);
        if (!h->sym_ok)
            return fail(SOSRT_E_INVALID, "atmosphere phase sets need the flip-symmetric contraction, and the matrices of the last sosrt_set_phase "
                                         "are not symmetric (asymmetry %.3g > %.3g)", h->asymmetry, (double)SOSRT_SYMMETRY_TOL);
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
        ranks[q] = lowrank_factor(W[q], D, u, v, &res[q]);
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
    if (S_atm > h->atm_capacity) {                       // (the new stacks first: a failure leaves the old ones in place)
        double *nW = nullptr, *nU = nullptr, *nV = nullptr;
        int* nR = nullptr;
        int e = dalloc(&nW, per * S_atm);
        if (!e) e = dalloc(&nU, LR * S_atm);
        if (!e) e = dalloc(&nV, LR * S_atm);
        if (!e) e = dalloc(&nR, (size_t)S_atm);
        if (e) {
            for (void* p : {(void*)nW, (void*)nU, (void*)nV, (void*)nR})
                if (p) hipFree(p);
            return e;
        }
        for (void* p : {(void*)h->d_Wasets, (void*)h->d_lrUsets, (void*)h->d_lrVsets, (void*)h->d_lrranks})
            if (p) hipFree(p);                           // (hipFree synchronises: no launch still reads them)
        h->d_Wasets = nW; h->d_lrUsets = nU; h->d_lrVsets = nV; h->d_lrranks = nR;
        h->atm_capacity = S_atm;
    }
    HIPCHK(hipStreamSynchronize(h->stream));             // a solve in flight still reads W_atm
    HIPCHK(hipMemset(h->d_Wasets, 0, per * S_atm * sizeof(double)));       // the padding rows and columns stay zero
    for (int q = 0; q < S_atm; ++q)
        HIPCHK(hipMemcpy2D(h->d_Wasets + q * per, g.Wld * sizeof(double), W[q].data(), g.D * sizeof(double), g.D * sizeof(double),
                           g.D, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lrUsets, U.data(), U.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lrVsets, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lrranks, ranks.data(), ranks.size() * sizeof(int), hipMemcpyHostToDevice));
    // set 0 is the handle's W_atm: what sosrt_set_phase would have left for this matrix
    h->Wa_h = W[0];
    HIPCHK(hipMemcpy2D(h->d_Wa, g.Wld * sizeof(double), h->Wa_h.data(), g.D * sizeof(double), g.D * sizeof(double), g.D,
                       hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lrU, U.data(), LR * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lrV, V.data(), LR * sizeof(double), hipMemcpyHostToDevice));
    h->lr_rank = ranks[0]; h->lr_residual = res[0];
    if (asym > h->asymmetry) h->asymmetry = asym;        // (still within the tolerance: the choice of the symmetric form stands)
    h->natm = S_atm;
    h->mix_dirty = true; h->w32_dirty = true;
    h->sym_dirty = true; h->symmix_dirty = true;
    return 0;
}

int sosrt_set_atmosphere_sets(sosrt_t* h, int B, const int* col_set) {
    if (!h || !col_set) return fail(SOSRT_E_INVALID, "null argument");
    if (B < 1) return fail(SOSRT_E_INVALID, "B=%d must be >= 1", B);
    if (int e = need_gpu(h)) return e;
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (B != h->B) return fail(SOSRT_E_INVALID, "B=%d does not match sosrt_set_columns (B=%d)", B, h->B);
    std::vector<int> aset(col_set, col_set + B);
    int top = 0;
    for (int b = 0; b < B; ++b) {
        if (aset[b] < 0 || aset[b] >= h->natm)
            return fail(SOSRT_E_INVALID, "column %d: atmosphere set %d outside 0..%d (sosrt_set_atm_phase_sets)", b, aset[b], h->natm - 1);
        top = aset[b] > top ? aset[b] : top;
    }
    if (top == 0 && h->max_atm_used == 0) return 0;      // all on set 0 before and after: nothing to do
    if (top > 0) {
        // (what sosrt_set_atm_phase_sets accepted S_atm > 1 under; sosrt_set_contraction / sosrt_set_first_order keep it so)
        if (!use_lowrank(h) || !use_sym(h))
            return fail(SOSRT_E_INVALID, "atmosphere sets need the low-rank plain rows and the flip-symmetric form of SOSRT_CONTRACT_F64");
        if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with atmosphere sets");
    }
    const bool slabs = h->geom == SOSRT_GEOM_THREE_ZONE && h->nslab > 0;
    MixGroups mg;
    bool fits = true;
    if (slabs) {
        const int cap = mix_group_cap(h, top > 0 || h->max_set_used > 0);
        fits = collect_mix_groups(h, B, h->c_zset, aset, cap, mg);
        if (!fits && top > 0)
            return fail(SOSRT_E_INVALID, "more than %d distinct (atmosphere set, aerosol set, ca, cr) groups: the two-pass form that a batch beyond the "
                                         "cache takes reads one W_atm, so it is not available with atmosphere sets", cap);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_colatm, aset.data(), B * sizeof(int), hipMemcpyHostToDevice));
    h->c_atmset = aset;
    h->max_atm_used = top;
    h->resident = false;
    if (slabs)
        if (int e = fits ? apply_mix_groups(h, B, mg) : apply_two_pass_rows(h, B)) return e;
    return 0;
}

int sosrt_atm_sets_info(sosrt_t* h, int* out) {
    if (!h || !out) return fail(SOSRT_E_INVALID, "null argument");
    out[0] = h->natm;
    out[1] = (h->have_cols && h->max_atm_used > 0) ? 1 : 0;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// step level
// ---------------------------------------------------------------------------------------------
// host P0_aer -> device: [B][2N], or [B][p0_zones][2N] when the zone table carries aerosol sets (sosrt_set_aerosol_sets)
static int stage_p0_aer(sosrt_handle* h, int B, const double* P0_aer, hipStream_t s, const double** d_out) {
    *d_out = nullptr;
    if (!P0_aer) return 0;
    if (h->p0_zones == 0) {
        HIPCHK(hipMemcpyAsync(h->d_P0r, P0_aer, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, s));
        *d_out = h->d_P0r;
        return 0;
    }
    const size_t need = (size_t)B * h->p0_zones * h->D;
    if (need > h->p0rz_capacity) {
        if (h->d_P0rz) hipFree(h->d_P0rz);
        h->d_P0rz = nullptr; h->p0rz_capacity = 0;
        if (int e = dalloc(&h->d_P0rz, need)) return e;
        h->p0rz_capacity = need;
    }
    HIPCHK(hipMemcpyAsync(h->d_P0rz, P0_aer, need * sizeof(double), hipMemcpyHostToDevice, s));
    *d_out = h->d_P0rz;
    return 0;
}

int sosrt_first_order(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer,
                      double* I1_out) {
    if (int e = check_ready(h, B, false)) return e;
    if (!tau || !P0_atm || !I1_out) return fail(SOSRT_E_INVALID, "null argument");
    if (h->geom == SOSRT_GEOM_THREE_ZONE && !P0_aer) return fail(SOSRT_E_INVALID, "three-zone geometry needs P0_aer");
    HIPCHK(hipSetDevice(h->device));
    h->resident = false;                     // d_tau is overwritten
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_P0a, P0_atm, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const double* d_p0r = nullptr;
    if (int e = stage_p0_aer(h, B, P0_aer, h->stream, &d_p0r)) return e;
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->d_tau, h->d_desc, h->d_rca, h->d_rcr);
    prof_begin(h, SOSRT_K_FIRST);
    if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
        launch_first_order_readme(h->stream, h->g, h->d_w, B, h->d_tau, h->d_P0a, d_p0r, h->d_desc, h->d_InA,
                                  nullptr, nullptr, 0, make_conv(h, 0), 0);
    else
        launch_first_order(h->stream, h->g, B, h->d_tau, h->d_P0a, d_p0r, h->d_desc, h->d_InA, nullptr,
                           nullptr, 0, make_conv(h, 0), 0, h->p0_zones);
    prof_end(h, SOSRT_K_FIRST);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(I1_out, h->d_InA, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int sosrt_source(sosrt_t* h, int B, const double* In_1, double* Jn_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!In_1 || !Jn_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (int e = ensure_w32(h)) return e;
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->d_InA, In_1, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // the row coefficients depend on tau only through the zone bounds; prepare needs a tau buffer
    // for the a4b buckets, which the source function does not use
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->d_tau, h->d_desc, h->d_rca, h->d_rcr);
    run_source(h, h->d_InA, h->d_Jn, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Jn_out, h->d_Jn, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int sosrt_transport(sosrt_t* h, int B, const double* tau, const double* Jn, double* In_out, int* status_out) {
    if (int e = check_ready(h, B, false)) return e;
    if (!tau || !Jn || !In_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    h->resident = false;                     // d_tau is overwritten
    const size_t n = (size_t)B * h->L * h->D;
    HIPCHK(hipMemcpyAsync(h->d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_Jn, Jn, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    launch_prepare(h->stream, h->g, B, h->geom, h->surface, scalars_of(h), h->d_tau, h->d_desc, h->d_rca, h->d_rcr);
    HIPCHK(hipMemsetAsync(h->d_InB, 0, n * sizeof(double), h->stream));
    prof_begin(h, SOSRT_K_SMALLMU);
    launch_smallmu(h->stream, h->g, B, h->d_tau, h->d_Jn, h->d_InB, h->d_desc, nullptr);
    prof_end(h, SOSRT_K_SMALLMU);
    prof_begin(h, SOSRT_K_TRANSPORT);
    const bool ring_like = h->transport_mode >= 2 && h->ring_ok && (h->max_nz <= kRingZones || transport_ring_fits(h->g, h->max_nz));
    const int nzcap = h->max_nz > kRingZones ? h->max_nz : kRingZones;
    if (h->transport_mode >= 1 && h->fast_ok && (h->max_nz <= kRingZones || ring_like)) {
        launch_attenuation(h->stream, h->g, B, h->d_tau, h->d_E, nullptr);
        HIPCHK(hipMemsetAsync(h->d_redo, 0, B * sizeof(int), h->stream));
        launch_transport(h->stream, h->g, B, h->d_tau, h->d_Jn, h->d_InB, nullptr, nullptr, 0, h->d_desc, make_conv(h, 0), 0, 0, h->d_E,
                         (h->transport_mode == 4 && h->scan_ok && transport_scan_fits(h->g, nzcap, false)) ? 4 : (ring_like ? 3 : 1),
                         nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nzcap);
        if (h->N - 3 > 61 && !(h->transport_mode >= 2 && h->ring_ok))
            launch_transport(h->stream, h->g, B, h->d_tau, h->d_Jn, h->d_InB, nullptr, nullptr, 0, h->d_desc, make_conv(h, 0), 0, 0, h->d_E, 2);
    } else {
        launch_transport(h->stream, h->g, B, h->d_tau, h->d_Jn, h->d_InB, nullptr, nullptr, 0, h->d_desc, make_conv(h, 0), 0, 0, nullptr, 0);
    }
    prof_end(h, SOSRT_K_TRANSPORT);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(In_out, h->d_InB, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status_out) HIPCHK(hipMemcpyAsync(status_out, h->d_status, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

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

int sosrt_solve_dev(sosrt_t* h, int B, const double* d_tau, const double* d_P0_atm, const double* d_P0_aer, double tol,
                    const double* d_I1_in, double* d_I_out, double* d_I_saved_out, int* d_n_orders_out,
                    int* d_status_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!d_tau || !d_I_out) return fail(SOSRT_E_INVALID, "null argument");
    if (!d_I1_in && !d_P0_atm) return fail(SOSRT_E_INVALID, "P0_atm is required unless I1 is supplied");
    if (!d_I1_in && h->geom == SOSRT_GEOM_THREE_ZONE && !d_P0_aer) return fail(SOSRT_E_INVALID, "three-zone geometry needs P0_aer");
    if (h->max_orders >= 65536) return fail(SOSRT_E_INVALID, "max_orders must be < 65536");
    HIPCHK(hipSetDevice(h->device));
    if (int e = ensure_w32(h)) return e;
    hipStream_t s = h->stream;
    const Grid& g = h->g;
    const size_t LD = (size_t)h->L * h->D;
    const size_t saved_stride = (size_t)h->saved_slots * LD;
    const int NG = h->ngroups;

    prof_break(h);
    // per-sweep setup on the caller's stream: zone tables, shared attenuation tables, combined slab matrices
    // this solve's counters were zeroed by the previous solve's first kernel (or at sosrt_create); its own first kernel zeroes
    // the other set, clears the redo flags and hashes the optical-depth profiles -- one launch instead of four
    h->nactive_set ^= 1;
    h->d_nactive = h->d_nactive_sets + h->nactive_set * (sosrt_handle::kMaxGroups + 1);
    SolveSetup su;
    su.zero_next = h->d_nactive_sets + (h->nactive_set ^ 1) * (sosrt_handle::kMaxGroups + 1);
    su.n_zero = sosrt_handle::kMaxGroups + 1;
    su.redo = h->d_redo;
    su.hash = h->d_tauhash;
    su.scan_sync = h->d_scan_sync;
    launch_prepare(s, g, B, h->geom, h->surface, scalars_of(h), d_tau, h->d_desc, h->d_rca, h->d_rcr,
                   h->d_nactive + sosrt_handle::kMaxGroups, su);
    h->need_small = true;
    const int small_tag = ((++h->pub_seq) & 0x3fffffff) | 0x40000000;       // never equals an order tag
    bool small_published = false;
    const SolveShape shape = solve_shape(h, h->max_nz);
    const bool fast = shape.fast;
    const int nzcap = shape.nzcap;
    if (h->use_etab || fast) {
        // one attenuation table per distinct optical-depth profile
        launch_tau_groups(s, g, B, d_tau, h->d_tauhash, h->d_erep, h->d_nactive + sosrt_handle::kMaxGroups,
                          h->h_pub + 8 * sosrt_handle::kMaxGroups, small_tag);
        launch_attenuation(s, g, B, d_tau, h->d_E, h->d_erep);
        small_published = true;
    }
    if (int e = ensure_matrices(h, s)) return e;
    bool forked = false;
    // an error return after the fork still joins the internal stream back onto the caller's
    int ol_held[sosrt_handle::kMaxGroups] = {0, 0};          // CUs this solve's order-loop launches hold (ol_acquire)
    auto bail = [&](int code) {
        if (forked && hipEventRecord(h->ev_join, h->stream2) == hipSuccess) (void)hipStreamWaitEvent(s, h->ev_join, 0);
        for (int k = 0; k < NG; ++k)
            if (ol_held[k]) {                                 // (a launch still running keeps its CUs until its stream has drained)
                (void)hipStreamSynchronize(group_stream(h, k));
                ol_release(h->device, ol_held[k]);
                ol_held[k] = 0;
            }
        return code;
    };

    // Order loop (spec:309-458), per column group.  Converged columns are masked on the device (every kernel of an
    // order returns at once for them).  r_k = number of live columns of the group after order k is written to a
    // pinned slot by the first workgroup of order k+1's source-function launch; before launching order k+1 the
    // host checks r_{k-1}, which is there as soon as order k has started, so a stream never drains inside the loop
    // and at most one launch group runs on a fully converged group.  With two groups the host feeds them in turn:
    // each stream always holds the next order of its group, and the GPU overlaps the contraction of one group
    // (MFMA-bound) with the transport of the other (HBM-bound).
    struct GroupState {
        int b0 = 0, nb = 0, n = 1, known = 0;
        bool done = false, started = false;
        bool ol_pending = false, ol_off = false;             // an order-loop launch is running; one was refused: no more in this solve
        int ol_tag = 0;
        unsigned ol_polls = 0;
        double *In_1 = nullptr, *In = nullptr;
        Conv cv;
    } gs[sosrt_handle::kMaxGroups];
    h->ol_launches = 0; h->ol_refused = 0;
    for (bool& u : h->ol_group_used) u = false;
    bool used_order_loop = false;
    const int tagbase = ((++h->pub_seq) & 0x3fff) << 16;      // tag of order n = tagbase + n
    for (int k = 0; k < NG; ++k) {
        GroupState& q = gs[k];
        q.b0 = h->gb[k]; q.nb = h->gb[k + 1] - h->gb[k]; q.known = q.nb;
        q.In_1 = h->d_InA; q.In = h->d_InB;                   // whole-batch buffers; every kernel gets its group's offset
        // The coded first order writes I = I1 only: the second order's contraction reads its operand there (the same numbers),
        // and the first order is bound by its stores (one 8 L D array instead of two: 91 -> 50 us for 512 columns)
        if (!d_I1_in && h->first_order_mode != SOSRT_FIRST_ORDER_README) q.In_1 = d_I_out;
        q.cv = make_conv(h, tol);
        q.cv.active += q.b0; q.cv.norders += q.b0; q.cv.status += q.b0; q.cv.ratio += q.b0; q.cv.redo += q.b0;
        q.cv.nactive = h->d_nactive + k;
        if (h->d_targets) q.cv.target = h->d_targets + q.b0;
    }
    auto start_group = [&](int k) {
        GroupState& q = gs[k];
        q.started = true;
        hipStream_t sg = group_stream(h, k);
        const size_t fo = (size_t)q.b0 * LD;
        prof_begin(h, SOSRT_K_FIRST, k);
        if (d_I1_in)
            hipLaunchKernelGGL(k_init_from_I1, dim3(q.nb), dim3(256), 0, sg, g, d_I1_in + fo, q.In_1 + fo, d_I_out + fo,
                               d_I_saved_out ? d_I_saved_out + (size_t)q.b0 * saved_stride : nullptr, saved_stride, q.cv);
        else if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            launch_first_order_readme(sg, g, h->d_w, q.nb, d_tau + (size_t)q.b0 * h->L, d_P0_atm + (size_t)q.b0 * g.D,
                                      d_P0_aer ? d_P0_aer + (size_t)q.b0 * g.D : nullptr, h->d_desc + q.b0, q.In_1 + fo,
                                      d_I_out + fo, d_I_saved_out ? d_I_saved_out + (size_t)q.b0 * saved_stride : nullptr,
                                      saved_stride, q.cv, 1);
        else
            launch_first_order(sg, g, q.nb, d_tau + (size_t)q.b0 * h->L, d_P0_atm + (size_t)q.b0 * g.D,
                               d_P0_aer ? d_P0_aer + (size_t)q.b0 * g.D * (h->p0_zones > 0 ? h->p0_zones : 1) : nullptr, h->d_desc + q.b0,
                               d_I_out + fo, nullptr, d_I_saved_out ? d_I_saved_out + (size_t)q.b0 * saved_stride : nullptr, saved_stride,
                               q.cv, 1, h->p0_zones);
        prof_end(h, SOSRT_K_FIRST, k);
    };
    start_group(0);
    if (NG > 1) {
        // The second column group runs on the internal stream from here on.  The fork comes BEHIND the first group's first order:
        // the two calls cost the host ~25 us, which the GPU -- 20 us of setup kernels ahead of the host at this point -- would
        // otherwise wait for; the second group starts half a cycle after the first anyway.
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        forked = true;
    }
    if (small_published && g.nsmall > 0) {
        // k_prepare's verdict on k_smallmu, published by the second kernel of the solve: by now it has long run
        volatile int* slot = h->h_pub + 8 * sosrt_handle::kMaxGroups;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 1; __atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) != small_tag; ++it) {
            if ((it & 0x3fff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return bail(fail(SOSRT_E_HIP, "order loop: no progress for 120 s"));
            __builtin_ia32_pause();
        }
        h->need_small = slot[0] != 0;
    }
    int live_groups = NG, n_max = 1;
    while (live_groups > 0) {
        bool progressed = false;
        for (int k = 0; k < NG; ++k) {
            GroupState& q = gs[k];
            if (q.done) continue;
            if (q.ol_pending) {
                // the group's remaining orders run in one launch; its last workgroup reports {state, tag} to pinned memory
                volatile int* dw = h->h_oldone + 2 * k;
                if (__atomic_load_n(&dw[1], __ATOMIC_ACQUIRE) != q.ol_tag) {
                    if ((++q.ol_polls & 0x3fff) != 0) continue;
                    const hipError_t qe = hipStreamQuery(group_stream(h, k));
                    if (qe != hipSuccess && qe != hipErrorNotReady) return bail(fail(SOSRT_E_HIP, "order loop: %s", hipGetErrorString(qe)));
                    if (qe == hipSuccess && __atomic_load_n(&dw[1], __ATOMIC_ACQUIRE) != q.ol_tag)
                        return bail(fail(SOSRT_E_HIP, "order loop: the order-loop launch ended without reporting"));
                    continue;
                }
                const int state = dw[0];
                q.ol_pending = false;
                ol_release(h->device, ol_held[k]);
                ol_held[k] = 0;
                progressed = true;
#ifdef SOSRT_OL_STAMPS
                if (h->d_ollog && getenv("SOSRT_OL_LOG")) {
                    std::vector<unsigned long long> lg(65001);
                    (void)hipStreamSynchronize(group_stream(h, k));
                    (void)hipMemcpy(lg.data(), h->d_ollog, lg.size() * 8, hipMemcpyDeviceToHost);
                    if (FILE* f = fopen(getenv("SOSRT_OL_LOG"), "a")) {
                        fprintf(f, "# launch columns<=%d order0=%d events=%llu\n", q.known, q.n + 1, lg[0]);
                        for (unsigned long long i = 0; i < lg[0] && i < 65000; ++i)
                            fprintf(f, "%llu %llu %llu %llu\n", lg[1 + i] >> 48, (lg[1 + i] >> 40) & 0xff, (lg[1 + i] >> 32) & 0xff, lg[1 + i] & 0xffffffffull);
                        fclose(f);
                    }
                }
#endif
                if (state == kOlReady) { q.done = true; --live_groups; h->ol_group_used[k] = true; continue; }
                if (state == kOlAborted) {
                    // never expected: say where the launch stood (the words of the launch, first columns)
                    std::vector<int> w(order_loop_sync_ints(q.known < 6 ? q.known : 6));
                    (void)hipStreamSynchronize(group_stream(h, k));
                    (void)hipMemcpy(w.data(), h->d_olsync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols), w.size() * sizeof(int), hipMemcpyDeviceToHost);
                    std::string cols;
                    for (int c = 0; c < (q.known < 6 ? q.known : 6); ++c) {
                        char buf[96];
                        const int* cs = w.data() + kOlCols + c * kOlColStride;
                        snprintf(buf, sizeof buf, " [%d: orders %d stop %d tiles %d]", c, cs[kOlOrdDone], cs[kOlColStop], cs[kOlJnDone]);
                        cols += buf;
                    }
                    return bail(fail(SOSRT_E_HIP, "order loop: a workgroup of the order-loop launch gave up waiting (arrived %d, left %d, order %d on, %d columns:%s)",
                                     w[kOlArrive], w[kOlLeft], q.n + 1, q.known, cols.c_str()));
                }
                // not resident (another process's kernels held CUs): nothing was touched; the one-order kernels take over
                q.ol_off = true;
                ++h->ol_refused;
            }
            if (!q.started) {
                // Staggered start: the dense orders of this group (they fill the GPU) run beside the long tail of the
                // previous one (a few workgroups per order, latency-bound), instead of both being dense, then both in
                // their tails, together.
                const GroupState& p = gs[k - 1];
                if (!(p.done || (p.n >= 2 && p.known <= h->stagger * p.nb))) continue;
                start_group(k);
            }
            progressed = true;
            if (q.n >= h->order_budget) { q.done = true; --live_groups; continue; }
            if (q.n >= 2) {
                const int live = wait_published(h, k, tagbase + q.n - 1);
                if (live < 0) return bail(live);
                if (live == 0) { q.done = true; --live_groups; continue; }
                q.known = live;
            }
            hipStream_t sg = group_stream(h, k);
            const size_t fo = (size_t)q.b0 * LD;
            const double* tau_g = d_tau + (size_t)q.b0 * h->L;
            const int* erep_g = h->d_erep + q.b0;     // values are whole-batch column ids; the table base is not offset
            // ---- the plan of this order (plan_order: one place for the whole policy) ----
            OrderInputs oi;
            oi.nb = q.nb; oi.known = q.known; oi.surface = h->surface;
            oi.simple_zones = h->simple_zones; oi.slabs_mixed = h->nslab == 0 || h->mix_groups > 0;
            oi.need_small = g.nsmall > 0 && h->need_small; oi.saving = d_I_saved_out != nullptr;
            oi.orders_left = h->order_budget - q.n;
            oi.cu_share = (q.ol_off || h->d_targets || h->max_atm_used > 0) ? 0 : h->cu_count / NG;   // (no order-loop launch with order targets, or atmosphere sets)
            LaunchPlan pl = plan_order(h, shape, oi);
            if (pl.order_loop) {
                // its workgroups wait for each other: they must all fit the CUs no other order-loop launch of this process holds
                const int got = ol_acquire(h->device, h->cu_count, pl.ol_grid, (int)(pl.ol_parts * q.known / h->ol_frac));
                if (got == 0) { oi.cu_share = 0; pl = plan_order(h, shape, oi); }
                else { pl.ol_grid = got; ol_held[k] = got; }
            }
            // (mode 2, for the tests of the refusal path: a grid of twice the CUs can never be resident -- the handshake times out,
            // nothing has been touched, and the order is run as two launches)
            if (pl.order_loop && h->order_loop == 2) pl.ol_grid = 2 * h->cu_count;
            if (pl.order_loop) {
                OrderLoopArgs oa;
                Grid gt = g;
                gt.nsmall = 0;
                oa.t = TransportArgs{gt, tau_g, h->d_Jn + fo, nullptr, d_I_out + fo, nullptr, 0, h->d_desc + q.b0, q.cv, 0, 1, h->d_E, erep_g, nullptr};
                oa.t.nzcap = kRingZones;
                oa.t.scan_split = pl.ol_parts > 1 ? 1 : 0;
                oa.t.scan_scratch = h->d_scan_scratch + (size_t)q.b0 * transport_scan_scratch_doubles();
                oa.t.scan_sync = h->d_scan_sync + 2 * q.b0;
                GemmArgs& ga = oa.gm;
                ga.A = nullptr; ga.Wa = h->d_Wa_s; ga.Wr = h->d_Wr_s; ga.ca = h->d_rca; ga.cr = h->d_rcr;
                ga.D = g.D; ga.Dp = g.Dp; ga.Wld = g.Wld; ga.L = h->L; ga.C = h->d_Jn;
                ga.sym = 1; ga.Ks = (g.N + GEMM_KC - 1) / GEMM_KC * GEMM_KC;
                if (use_lowrank(h)) { ga.lr_rank = h->lr_rank; ga.lrU = h->d_lrU; ga.lrV = h->d_lrV; }
                ga.max_main = h->max_main; ga.max_slab = h->max_slab;
                ga.idx_up = h->nslab > 0 ? h->d_idx_up : nullptr; ga.idx_down = h->nslab > 0 ? h->d_idx_down : nullptr;
                if (h->mix_groups > 0) { ga.Wmix = h->d_Wmix_s; ga.mix_group = h->d_mixgroup; }
                oa.in0 = q.In_1;
                oa.gbufP = q.In;
                oa.gbufQ = (q.In_1 == d_I_out) ? h->d_InA : q.In_1;   // (after the second order: the buffer the first order left unused)
                oa.bufP = oa.gbufP + fo; oa.bufQ = oa.gbufQ + fo;
                oa.order0 = q.n + 1; oa.kmax = h->order_budget - q.n;
                oa.B = q.nb; oa.col0 = q.b0;
                oa.fixcap = (int)(0.06 * g.N) + 1;
                oa.sync = h->d_olsync + (size_t)k * order_loop_sync_ints(kOrderLoopMaxCols);
                oa.host_done = h->h_oldone + 2 * k;
                oa.tag = q.ol_tag = ((++h->pub_seq) & 0x3fffffff) | 0x40000000;
#ifdef SOSRT_OL_STAMPS   // diagnostic builds: SOSRT_OL_LOG=<file> receives the launch's event log (tools/ol_timeline.py)
                if (getenv("SOSRT_OL_LOG")) {
                    if (!h->d_ollog) { if (int e = dalloc(&h->d_ollog, 65001)) return bail(e); }
                    HIPCHK(hipMemsetAsync(h->d_ollog, 0, 8, sg));
                    oa.log = h->d_ollog;
                }
#endif
                prof_break(h);
                HIPCHK(hipMemsetAsync(oa.sync, 0, order_loop_sync_ints(q.known) * sizeof(int), sg));
                prof_begin(h, SOSRT_K_ORDER_LOOP, k);
                const hipError_t le = launch_order_loop(sg, pl.ol_grid, pl.ol_parts > 1, oa);
                prof_end(h, SOSRT_K_ORDER_LOOP, k);
                if (le != hipSuccess) return bail(fail(SOSRT_E_HIP, "order-loop launch failed: %s", hipGetErrorString(le)));
                q.ol_pending = true;
                used_order_loop = true;
                ++h->ol_launches;
                continue;
            }
            const int n = ++q.n;
            n_max = n > n_max ? n : n_max;
            // this launch also publishes the group's live count after order n-1
            const int tail_cols = pl.tail_cols;
            run_source(h, q.In_1, h->d_Jn, h->d_active, tail_cols, tagbase + n - 1, k, q.known == q.nb, pl.gemm == SOSRT_PLAN_GEMM_LIVE16_REGS,
                       tail_cols > 0 ? 0 : pl.live_cap);
            if (g.nsmall > 0 && h->need_small) {      // skipped once the device has reported that every such lane is rewritten anyway
                prof_begin(h, SOSRT_K_SMALLMU, k);
                launch_smallmu(sg, g, q.nb, tau_g, h->d_Jn + fo, q.In + fo, h->d_desc + q.b0, q.cv.active);
                prof_end(h, SOSRT_K_SMALLMU, k);
            }
            prof_begin(h, SOSRT_K_TRANSPORT, k);
            double* sv_n = (d_I_saved_out && n <= h->saved_slots) ? d_I_saved_out + (size_t)q.b0 * saved_stride + (size_t)(n - 1) * LD : nullptr;
            if (pl.transport != SOSRT_PLAN_TRANSPORT_GENERAL) {
                // once the device has reported that no |mu| < 0.01 lane keeps its k_smallmu value, the ring kernel
                // need not stage those rows either
                Grid gt = g;
                if (pl.transport >= SOSRT_PLAN_TRANSPORT_RING && !h->need_small) gt.nsmall = 0;
                launch_transport(sg, gt, q.nb, tau_g, h->d_Jn + fo, q.In + fo, d_I_out + fo, sv_n, saved_stride, h->d_desc + q.b0, q.cv, n, 1,
                                 h->d_E, pl.transport, erep_g, pl.live_cap, h->d_livelist + q.b0, NG > 1 ? h->coresident_slots : 0,
                                 pl.parts > 1 ? 1 : 0, h->d_scan_scratch + (size_t)q.b0 * transport_scan_scratch_doubles(),
                                 h->d_scan_sync + 2 * q.b0, nzcap);
                if (pl.repair)                           // register-streaming kernel: a search that leaves wave 0 is redone by the
                    launch_transport(sg, g, q.nb, tau_g, h->d_Jn + fo, q.In + fo, d_I_out + fo, sv_n, saved_stride, h->d_desc + q.b0, q.cv, n, 1,
                                     h->d_E, 2, erep_g);         // general kernel (flag cv.redo); the ring kernel redoes it itself
            } else {
                launch_transport(sg, g, q.nb, tau_g, h->d_Jn + fo, q.In + fo, d_I_out + fo, sv_n, saved_stride, h->d_desc + q.b0, q.cv, n, 1,
                                 h->use_etab ? h->d_E : nullptr, 0, erep_g);
            }
            prof_end(h, SOSRT_K_TRANSPORT, k);
            if (q.In_1 == d_I_out) { q.In_1 = q.In; q.In = h->d_InA; }      // (after the second order: the buffer the first order left unused)
            else { double* tmp = q.In_1; q.In_1 = q.In; q.In = tmp; }
        }
        if (!progressed) __builtin_ia32_pause();      // (every live group is inside its order-loop launch)
    }
    if (NG > 1) {                                    // back onto the caller's stream
        HIPCHK(hipEventRecord(h->ev_join, h->stream2));
        HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
    }
    prof_break(h);
    launch_finalize(s, B, make_conv(h, tol), h->order_budget, d_n_orders_out, d_status_out);
    HIPCHK(hipGetLastError());
    h->last_max_orders = used_order_loop ? -1 : n_max;      // (orders run inside an order-loop launch: read back with the counts)
    h->last_sum_orders = -1;
    return 0;
}

int sosrt_solve(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer, double tol,
                const double* I1_in, double* I_out, double* I_saved_out, int* n_orders_out, int* status_out) {
    if (int e = check_ready(h, B, true)) return e;
    if (!tau) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->resident = false;
    const size_t LD = (size_t)h->L * h->D, n = (size_t)B * LD;
    HIPCHK(hipMemcpyAsync(h->d_tau, tau, (size_t)B * h->L * sizeof(double), hipMemcpyHostToDevice, s));
    if (P0_atm) HIPCHK(hipMemcpyAsync(h->d_P0a, P0_atm, (size_t)B * h->D * sizeof(double), hipMemcpyHostToDevice, s));
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
        if (int e = sosrt_solve_dev(h, B, h->d_tau, P0_atm ? h->d_P0a : nullptr, d_p0r, tol, d_I1,
                                    h->d_I, d_saved, nullptr, nullptr))
            return e;
        if (I_out) HIPCHK(hipMemcpyAsync(I_out, h->d_I, n * sizeof(double), hipMemcpyDeviceToHost, s));
        if (I_saved_out)
            HIPCHK(hipMemcpyAsync(I_saved_out, d_saved, (size_t)B * h->saved_slots * LD * sizeof(double), hipMemcpyDeviceToHost, s));
        std::vector<int> no(B);
        HIPCHK(hipMemcpyAsync(no.data(), h->d_norders, B * sizeof(int), hipMemcpyDeviceToHost, s));
        if (status_out) HIPCHK(hipMemcpyAsync(status_out, h->d_status, B * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        long long sum = 0;
        int mx = 1;
        for (int b = 0; b < B; ++b) { sum += no[b] - 1; mx = no[b] > mx ? no[b] : mx; if (n_orders_out) n_orders_out[b] = no[b]; }
        h->last_sum_orders = sum;
        if (h->last_max_orders < 0) h->last_max_orders = mx;
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
    if ((h->last_sum_orders < 0 || h->last_max_orders < 0) && h->B > 0) {
        std::vector<int> no(h->B);
        HIPCHK(hipMemcpyAsync(no.data(), h->d_norders, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        long long sum = 0;
        int mx = 1;
        for (int v : no) { sum += v - 1; mx = v > mx ? v : mx; }
        h->last_sum_orders = sum;
        if (h->last_max_orders < 0) h->last_max_orders = mx;
    }
    if (max_orders_run) *max_orders_run = h->last_max_orders;
    if (sum_orders) *sum_orders = h->last_sum_orders;
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
    HIPCHK(hipMemcpyAsync(h->d_tau, tau, r * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_I, I, n * sizeof(double), hipMemcpyHostToDevice, s));
    launch_prepare(s, h->g, B, h->geom, h->surface, scalars_of(h), h->d_tau, h->d_desc, h->d_rca, h->d_rcr);
    launch_fluxes(s, h->g, B, h->d_tau, h->d_I, h->d_desc, beam_norm, h->d_rca, h->d_rcr);   // row-sized scratch
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(flux_down, h->d_rca, r * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flux_up, h->d_rcr, r * sizeof(double), hipMemcpyDeviceToHost, s));
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
    launch_prepare(s, h->g, B, h->geom, h->surface, scalars_of(h), d_tau, h->d_desc, h->d_rca, h->d_rcr);
    EpilogueOut out{d_flux_down, d_flux_up, d_diffusivity, d_heating_rate, d_net_toa};
    launch_epilogue(s, h->g, h->d_w, B, d_tau, d_I, h->d_desc, beam_norm, d_z_profile, out);
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
    if (z_profile) HIPCHK(hipMemcpyAsync(h->d_z, z_profile, h->L * sizeof(double), hipMemcpyHostToDevice, s));
    double* o = h->d_Jn;                                     // scratch: the source function of the last order is dead
    if (int e = sosrt_epilogue_dev(h, B, h->d_tau, h->d_I, beam_norm, z_profile ? h->d_z : nullptr, flux_down ? o : nullptr,
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
// phase functions on the device
// ---------------------------------------------------------------------------------------------
int sosrt_phase_table(sosrt_t* h, const double* tab_mu, const double* tab_p, int ntab) {
    if (int e = need_gpu(h)) return e;
    if (!tab_mu || !tab_p || ntab < 2) return fail(SOSRT_E_INVALID, "a table needs at least two points");
    for (int i = 1; i < ntab; ++i)
        if (!(tab_mu[i] > tab_mu[i - 1])) return fail(SOSRT_E_INVALID, "tab_mu must be strictly ascending (index %d)", i);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_tab) { hipFree(h->d_tab); h->d_tab = nullptr; h->ntab = 0; }
    if (int e = dalloc(&h->d_tab, 2 * (size_t)ntab)) return e;
    HIPCHK(hipMemcpy(h->d_tab, tab_mu, ntab * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_tab + ntab, tab_p, ntab * sizeof(double), hipMemcpyHostToDevice));
    h->ntab = ntab;
    return 0;
}

int sosrt_phase_table_dev(sosrt_t* h, const double* d_tab_mu, const double* d_tab_p, int ntab) {
    if (int e = need_gpu(h)) return e;
    if (!d_tab_p || ntab < 2) return fail(SOSRT_E_INVALID, "a table needs at least two points");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (h->ntab != ntab || !h->d_tab) {                      // (a table of the same length is overwritten in stream order)
        HIPCHK(hipStreamSynchronize(s));
        if (h->d_tab) { hipFree(h->d_tab); h->d_tab = nullptr; h->ntab = 0; }
        if (int e = dalloc(&h->d_tab, 2 * (size_t)ntab)) return e;
        h->ntab = ntab;
    }
    if (d_tab_mu) {
        HIPCHK(hipMemcpyAsync(h->d_tab, d_tab_mu, ntab * sizeof(double), hipMemcpyDeviceToDevice, s));
    } else {
        std::vector<double> mu(ntab);
        mie_linspace(-1.0, 1.0, ntab, mu.data());
        HIPCHK(hipMemcpyAsync(h->d_tab, mu.data(), ntab * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                     // (mu leaves scope)
    }
    HIPCHK(hipMemcpyAsync(h->d_tab + ntab, d_tab_p, ntab * sizeof(double), hipMemcpyDeviceToDevice, s));
    return 0;
}

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
    if (!h->mie_ev) {
        HIPCHK(hipEventCreateWithFlags(&h->mie_ev, hipEventDisableTiming));
        for (auto& e : h->mie_t) HIPCHK(hipEventCreate(&e));
    }
    if (p.bytes > h->mie_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_mie) { hipFree(h->d_mie); h->d_mie = nullptr; h->mie_cap = 0; }
        if (int e = dalloc(&h->d_mie, p.bytes)) return e;
        h->mie_cap = p.bytes;
    }
    HIPCHK(hipEventSynchronize(h->mie_ev));                  // (never recorded: returns at once)
    if (p.in_bytes > h->mie_hcap) {
        if (h->h_mie) { hipHostFree(h->h_mie); h->h_mie = nullptr; h->mie_hcap = 0; }
        HIPCHK(hipHostMalloc((void**)&h->h_mie, p.in_bytes, hipHostMallocDefault));
        h->mie_hcap = p.in_bytes;
    }
    return 0;
}

// stages the inputs, copies them and launches the coefficient kernel (with `tables`, the other two as well)
int mie_run(sosrt_handle* h, const MiePlan& p, bool tables) {
    hipStream_t s = h->stream;
    double* tn = (double*)(h->h_mie + p.o_tn);
    tn[0] = 0;
    for (int n = 1; n <= p.n_cap; ++n) tn[n] = (n + 1.0) / n;
    HIPCHK(hipMemcpyAsync(h->d_mie, h->h_mie, p.in_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->mie_ev, s));
    char* d = h->d_mie;
    auto D = [&](size_t off) { return (double*)(d + off); };
    const int n = p.S * p.R;
    HIPCHK(hipEventRecord(h->mie_t[0], s));
    launch_mie_coefficients(s, n, p.R, p.n_cap, D(p.o_x), (const int*)(d + p.o_nmax), (const int*)(d + p.o_nstart), D(p.o_mre),
                            D(p.o_mim), tables ? D(p.o_radii) : nullptr, D(p.o_rm), D(p.o_sig), D(p.o_ab), D(p.o_qw));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->mie_t[1], s));
    if (tables) {
        launch_mie_angles(s, p.S, p.R, p.ntab, p.n_cap, D(p.o_mu), D(p.o_ab), (const int*)(d + p.o_nmax), D(p.o_tn), D(p.o_qw),
                          D(p.o_part));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->mie_t[2], s));
        launch_mie_integrate(s, p.S, p.R, p.ntab, D(p.o_part), D(p.o_radii), D(p.o_qw), D(p.o_p), D(p.o_bulk));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->mie_t[3], s));
    }
    h->mie_timed = tables;
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
    char* hm = h->h_mie;
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
    HIPCHK(hipMemcpyAsync(p_out, h->d_mie + p.o_p, (size_t)S * ntab * 8, kind, st));
    if (bulk_out) HIPCHK(hipMemcpyAsync(bulk_out, h->d_mie + p.o_bulk, (size_t)S * 3 * 8, kind, st));
    if (!dev) HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

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
    char* hm = h->h_mie;
    memcpy(hm + p.o_x, x, (size_t)K * 8);
    memcpy(hm + p.o_mre, m_re, (size_t)K * 8);
    memcpy(hm + p.o_mim, m_im, (size_t)K * 8);
    memcpy(hm + p.o_nmax, nmax.data(), (size_t)K * 4);
    memcpy(hm + p.o_nstart, nstart.data(), (size_t)K * 4);
    if (int e = mie_run(h, p, false)) return e;
    hipStream_t st = h->stream;
    std::vector<double> q((size_t)K * kMieQ);
    HIPCHK(hipMemcpyAsync(q.data(), h->d_mie + p.o_qw, q.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) memcpy(out + 4 * (size_t)k, q.data() + (size_t)k * kMieQ, 4 * sizeof(double));
    return 0;
}

int sosrt_mie_timing(sosrt_t* h, double* ms) {
    if (int e = need_gpu(h)) return e;
    if (!ms) return fail(SOSRT_E_INVALID, "null argument");
    if (!h->mie_timed) return fail(SOSRT_E_STATE, "sosrt_mie_ensembles has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->mie_t[3]));
    for (int k = 0; k < 3; ++k) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, h->mie_t[k], h->mie_t[k + 1]));
        ms[k] = t;
    }
    return 0;
}

static int phase_check(sosrt_handle* h, int kind, double g) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_grid) return fail(SOSRT_E_STATE, "sosrt_set_grid has not been called");
    if (kind < SOSRT_PHASE_ISO || kind > SOSRT_PHASE_TABLE) return fail(SOSRT_E_INVALID, "unknown phase-function kind %d", kind);
    if (kind == SOSRT_PHASE_TABLE && !h->d_tab) return fail(SOSRT_E_STATE, "sosrt_phase_table has not been called");
    if (kind == SOSRT_PHASE_HG && !(std::fabs(g) < 1)) return fail(SOSRT_E_INVALID, "|g| must be < 1 (got %g)", g);
    return 0;
}

int sosrt_phase_p0_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, double* d_P0_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (B < 1 || !d_mu0 || !d_P0_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    launch_phase_p0(h->stream, h->g, h->d_w, B, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                    h->d_phi + kNPhi, kNPhi, d_mu0, d_P0_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0(sosrt_t* h, int B, int kind, double g, const double* mu0, double* P0_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (B < 1 || B > h->max_batch || !mu0 || !P0_out) return fail(SOSRT_E_INVALID, "bad argument (B must be 1..max_batch)");
    for (int b = 0; b < B; ++b)
        if (!(mu0[b] > 0 && mu0[b] <= 1)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be in (0, 1]", b);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->d_ratio, mu0, B * sizeof(double), hipMemcpyHostToDevice, s));
    if (int e = sosrt_phase_p0_dev(h, B, kind, g, h->d_ratio, h->d_P0a)) return e;
    HIPCHK(hipMemcpyAsync(P0_out, h->d_P0a, (size_t)B * h->D * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int sosrt_phase_matrix_dev(sosrt_t* h, int kind, double g, double* d_P_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (!d_P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    launch_phase_matrix(h->stream, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                        h->d_phi + kNPhi, kNPhi, d_P_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_matrix(sosrt_t* h, int kind, double g, double* P_out) {
    if (int e = phase_check(h, kind, g)) return e;
    if (!P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    double* dP = nullptr;
    const size_t n = (size_t)h->D * h->D;
    if (int e = dalloc(&dP, n)) return e;
    int rc = 0;
    auto body = [&]() -> int {
        launch_phase_matrix(s, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                            h->d_phi + kNPhi, kNPhi, dP);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(P_out, dP, n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    rc = body();
    hipFree(dP);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Fourier modes in azimuth
// ---------------------------------------------------------------------------------------------
static int modes_check(sosrt_handle* h, int kind, double g, int m_first, int m_count, int nphi) {
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
static int modes_table(sosrt_handle* h, int nphi, int mf, int mc) {
    const size_t need = (size_t)(2 + mc) * nphi;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (need > h->modetab_cap) {
        if (h->d_modetab) { hipFree(h->d_modetab); h->d_modetab = nullptr; h->modetab_cap = 0; }
        if (int e = dalloc(&h->d_modetab, need)) return e;
        h->modetab_cap = need;
    }
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
    HIPCHK(hipMemcpy(h->d_modetab, t.data(), need * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int sosrt_phase_modes(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, double* P_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (!P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t DD = (size_t)h->D * h->D;
    const int mf = m_first > 0 ? m_first : 1, mc = m_first > 0 ? m_count : m_count - 1;   // modes m >= 1 of the request
    if (mc > 0)
        if (int e = modes_table(h, nphi, mf, mc)) return e;
    double* dP = nullptr;
    if (int e = dalloc(&dP, m_count * DD)) return e;
    auto body = [&]() -> int {
        if (m_first == 0)                                  // mode 0 is the existing builder's output, bit for bit (25-point ring)
            launch_phase_matrix(s, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                                h->d_phi + kNPhi, kNPhi, dP);
        if (mc > 0)
            launch_phase_modes(s, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_modetab,
                               h->d_modetab + nphi, nphi, mf, mc, dP + (m_count - mc) * DD);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(P_out, dP, m_count * DD * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    hipFree(dP);
    return rc;
}

int sosrt_phase_modes_dev(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, double* d_P_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (!d_P_out) return fail(SOSRT_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t DD = (size_t)h->D * h->D;
    const int mf = m_first > 0 ? m_first : 1, mc = m_first > 0 ? m_count : m_count - 1;   // modes m >= 1 of the request
    if (mc > 0)
        if (int e = modes_table(h, nphi, mf, mc)) return e;
    if (m_first == 0)
        launch_phase_matrix(s, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                            h->d_phi + kNPhi, kNPhi, d_P_out);
    if (mc > 0)
        launch_phase_modes(s, h->g, h->d_w, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_modetab,
                           h->d_modetab + nphi, nphi, mf, mc, d_P_out + (m_count - mc) * DD);
    if (sign_odd) launch_negate_odd_modes(s, DD, m_first, m_count, d_P_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0_modes_dev(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* d_mu0,
                             double* d_P0_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (B < 1 || !d_mu0 || !d_P0_out) return fail(SOSRT_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const int mf = m_first > 0 ? m_first : 1, mc = m_first > 0 ? m_count : m_count - 1;
    if (mc > 0)
        if (int e = modes_table(h, nphi, mf, mc)) return e;
    if (m_first == 0)
        launch_phase_p0(h->stream, h->g, h->d_w, B, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab, h->d_phi,
                        h->d_phi + kNPhi, kNPhi, d_mu0, d_P0_out);
    if (mc > 0)
        launch_phase_p0_modes(h->stream, h->g, h->d_w, B, kind, g, h->d_tab, h->d_tab ? h->d_tab + h->ntab : nullptr, h->ntab,
                              h->d_modetab, h->d_modetab + nphi, nphi, mf, mc, d_mu0, d_P0_out + (size_t)(m_count - mc) * B * h->D);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_phase_p0_modes(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* mu0,
                         double* P0_out) {
    if (int e = modes_check(h, kind, g, m_first, m_count, nphi)) return e;
    if (B < 1 || B > h->max_batch || !mu0 || !P0_out) return fail(SOSRT_E_INVALID, "bad argument (B must be 1..max_batch)");
    for (int b = 0; b < B; ++b)
        if (!(mu0[b] > 0 && mu0[b] <= 1)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be in (0, 1]", b);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t n = (size_t)m_count * B * h->D;
    double* dP = nullptr;
    if (int e = dalloc(&dP, n + B)) return e;
    auto body = [&]() -> int {
        HIPCHK(hipMemcpyAsync(dP + n, mu0, B * sizeof(double), hipMemcpyHostToDevice, s));
        if (int e = sosrt_phase_p0_modes_dev(h, B, kind, g, m_first, m_count, nphi, dP + n, dP)) return e;
        HIPCHK(hipMemcpyAsync(P0_out, dP, n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    (void)hipStreamSynchronize(s);
    hipFree(dP);
    return rc;
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
    if (h->comm) return fail(SOSRT_E_STATE, "the handle already has a communicator");
    if (const char* e = rccl().load()) return fail(SOSRT_E_STATE, "%s", e);
    HIPCHK(hipSetDevice(h->device));
    Rccl::UniqueId id;
    memcpy(&id, unique_id, sizeof id);
    NCCLCHK(rccl().CommInitRank(&h->comm, world, id, rank));
    h->comm_rank = rank; h->comm_world = world;
    return 0;
}

int sosrt_gather(sosrt_t* h, int root, const long long* counts, const double* d_send, double* d_recv) {
    if (int e = need_gpu(h)) return e;
    if (!h->comm) return fail(SOSRT_E_STATE, "sosrt_comm_init has not been called");
    if (!counts || root < 0 || root >= h->comm_world) return fail(SOSRT_E_INVALID, "bad root / counts");
    for (int r = 0; r < h->comm_world; ++r)
        if (counts[r] < 0) return fail(SOSRT_E_INVALID, "counts[%d] < 0", r);
    const int me = h->comm_rank;
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
        for (int r = 0; r < h->comm_world && !nrc && hrc == hipSuccess; ++r) {
            if (counts[r] > 0) {
                if (r == me) {
                    if (d_recv + off != d_send)
                        hrc = hipMemcpyAsync(d_recv + off, d_send, (size_t)counts[r] * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
                } else {
                    nrc = rccl().Recv(d_recv + off, (size_t)counts[r], kF64, r, h->comm, h->stream);
                }
            }
            off += (size_t)counts[r];
        }
    } else if (counts[me] > 0) {
        nrc = rccl().Send(d_send, (size_t)counts[me], kF64, root, h->comm, h->stream);
    }
    const int erc = rccl().GroupEnd();
    if (hrc != hipSuccess) rc = fail(SOSRT_E_HIP, "sosrt_gather: copy of the root's own block failed: %s", hipGetErrorString(hrc));
    else if (nrc) rc = fail(SOSRT_E_HIP, "sosrt_gather: ncclSend/ncclRecv failed: %s", rccl().GetErrorString(nrc));
    else if (erc) rc = fail(SOSRT_E_HIP, "sosrt_gather: ncclGroupEnd failed: %s", rccl().GetErrorString(erc));
    return rc;
}

int sosrt_comm_destroy(sosrt_t* h) {
    if (int e = need_gpu(h)) return e;
    if (h->comm) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        NCCLCHK(rccl().CommDestroy(h->comm));
        h->comm = nullptr; h->comm_rank = -1; h->comm_world = 0;
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
    HIPCHK(hipMemcpyAsync(h->d_Jn, rows, (size_t)R * h->N * sizeof(double), hipMemcpyHostToDevice, s));
    launch_limit_rows(s, h->g, R, table, h->d_Jn, h->d_InB);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_InB, (size_t)R * idx * sizeof(double), hipMemcpyDeviceToHost, s));
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
    double* dJ = h->d_Jn; double* dT = h->d_Jn + n;
    double* dtt = h->d_InB; double* dmu = h->d_InB + R; double* dout = h->d_InB + 2 * (size_t)R;
    int* dlen = (int*)(h->d_InA);
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
    if (which < 0 || which > h->nsets) return fail(SOSRT_E_INVALID, "which=%d: 0 is W_atm, 1 + s the aerosol set s of %d", which, h->nsets);
    std::vector<double>& W = which > 1 ? h->Wrx_h[which - 2] : (which ? h->Wr_h : h->Wa_h);
    if (which >= 1 && h->wr_on_device && h->have_aer && W.empty()) {       // a fold made on the device: fetched when asked for
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        W.assign((size_t)h->D * h->D, 0.0);
        HIPCHK(hipMemcpy2D(W.data(), h->D * sizeof(double), h->d_Wrsets + (size_t)(which - 1) * h->g.Dp * h->g.Wld,
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
// diagnostics: cycle stamps of k_transport_fast ([B][2 waves][8] clock64 values; pass NULL to stop)
// ---------------------------------------------------------------------------------------------
int sosrt_debug_stamps(sosrt_t* h, unsigned long long* d_stamps) {
    if (int e = need_gpu(h)) return e;
    sosrt::g_transport_stamps = d_stamps;
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
    if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
    for (Prof& p : h->prof) { p.used = 0; p.nint = 0; p.adjacent = -1; p.open = -1; }
    return 0;
}

int sosrt_profile_get(sosrt_t* h, int kernel, double* total_ms, long long* launches, double* work) {
    if (int e = need_gpu(h)) return e;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
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
