// Device-side data structures and kernel launchers (gfx950).
#pragma once
#include <hip/hip_runtime.h>

#include "plan.hpp"

namespace sosrt {

constexpr int kMaxZones = 8;       // zones of a column, top to bottom: clear / slab / clear / slab ... (up to four aerosol slabs)
constexpr int kRingZones = 3;      // zones the register-streaming kernel (fast) handles, and the zones the ring / chunk-parallel kernels keep in scalars

// One independent SOS problem as the kernels see it: a zone table instead of the reference's
// three copies of every formula (spec:113-449).
struct alignas(16) ColDesc {
    int nz;                    // zones, top to bottom
    int r0[kMaxZones];         // first / last row of each zone
    int r1[kMaxZones];
    int mix[kMaxZones];        // 1: aerosol slab (phase mix of spec:149,321)
    int nfix[kMaxZones];       // rewritten downward angles next to mu=0- (spec:342-345,361-364,380-383)
    int fixtab[kMaxZones];     // which extrapolation table
    int surface;               // SOSRT_SURFACE_*
    int geom;
    double mu0, rho, T, tau_bottom;
    double wa;                 // single-scattering albedo of the molecules
    double wr[kMaxZones];      // per zone: single-scattering albedo of its aerosol, slab mixing fractions (spec:50-53,149)
    double fa[kMaxZones];
    double fr[kMaxZones];
    double ca[kMaxZones];      // Jn coefficient on In_1 @ W_atm per zone (spec:321,323)
    double cr[kMaxZones];      // Jn coefficient on In_1 @ W_aer per zone
};

struct FixTab {
    int idx, s0, ns, pad;
    double C[kFixMaxIdx * kFixMaxSrc];
};

// per-column scalars as uploaded by sosrt_set_columns (structure of arrays)
struct ColScalars {
    // zone table of every column ([max_batch][kMaxZones]; filled from idx_up / idx_down by sosrt_set_columns, or given by
    // the caller through sosrt_set_columns_zones): first row of each zone, 1 for an aerosol slab, the slab's aerosol
    // single-scattering albedo and optical-depth step
    const int* nz;
    const int* zr0;
    const int* zmix;
    const double* zwr;
    const double* zdtr;
    const int* idx_up;
    const int* idx_down;
    const double* mu0;
    const double* rho;
    const double* alb_atm;
    const double* alb_aer;
    const double* dtau_atm;
    const double* dtau_aer;
    const double* T;
};

struct Grid {
    int L, N, D;
    int Dp;                    // D rounded up to the GEMM k-chunk
    int Wld;                   // leading dimension of the folded matrices (multiple of the GEMM column tile)
    const double* mu;          // [D]
    const double* Wa;          // [Dp][Wld]
    const double* Wr;          // [Dp][Wld]
    const FixTab* fix;         // [4]
    const int* small_lanes;
    int nsmall;
    const double* wflux_dn;    // [N]
    const double* wflux_up;    // [N]
};

struct Conv {
    int* active;               // [B] 1 while the column still iterates
    int* norders;              // [B] n of spec:307
    int* status;               // [B]
    int* nactive;              // [1]
    double* ratio;             // [B] last value of the spec:309 test
    int* redo;                 // [B] set by k_transport_fast when the column needs the general upward sweep
    const int* target;         // [B] or null: fixed order counts (sosrt_set_order_targets), the ratio is written but not tested
    double tol;
};

// The stop decision of every order: go on while the spec:309 ratio is >= tol, or -- with order targets -- while the column
// has run fewer orders than its target.  Without targets the expression is the one it always was (same bits).
__device__ __forceinline__ bool conv_go(const Conv& cv, int b, int order, double r) {
    return cv.target ? order < cv.target[b] : r >= cv.tol;
}

constexpr int GEMM_BM = 64, GEMM_BN = 128, GEMM_KC = 16;
#ifndef SOSRT_GEMM_RT
#define SOSRT_GEMM_RT 4
#endif
#ifndef SOSRT_GEMM_WPS
#define SOSRT_GEMM_WPS 3
#endif
constexpr int GEMM_RT = SOSRT_GEMM_RT;     // MFMA row tiles per wave of the plain-row workgroups
constexpr int GEMM_WPS = SOSRT_GEMM_WPS;   // waves per SIMD the register budget is set for

// Transport rows are processed in chunks of TC: the loads of the next chunks are in flight while
// the current one is computed, the per-row source terms of a chunk are independent
// (instruction-level parallelism for the one wave per SIMD a column gives), only the TC fused
// multiply-adds of the recurrence are sequential.
constexpr int TC = 8;

// The transport kernels by name; the values are the public SOSRT_PLAN_TRANSPORT_* of sosrt_plan_launch (tied in solve.hip).
// Repair: the general kernel behind the register-streaming one, for the columns whose search left wave 0 (flag cv.redo).
enum class TransportKernel { General = 0, Fast = 1, Repair = 2, Ring = 3, Scan = 4 };

// What a transport launch is given: a by-value kernel argument, and the whole interface of launch_transport.  The host fills it in
// one place (solve.hip: transport_args), by name; the launchers size and dispatch and leave every field as it came.
struct TransportArgs {
    Grid g;
    const double* tau;
    const double* Jn;
    double* In;
    double* I;
    double* saved;
    size_t saved_col_stride;
    const ColDesc* desc;
    Conv cv;
    int order;
    int accumulate;
    const double* Etab;
    const int* erep;           // [B] column whose attenuation table this column uses (same tau profile); null: its own
    unsigned long long* stamps;   // diagnostic builds only: [B][8] cycle stamps of the sweeps (nullable)
    // ring kernel, some columns converged: `live` > 0 launches workgroups for (an upper bound of) the live columns only;
    // workgroup i takes column live_list[i], the list the source-function launch of the same order wrote (the flags
    // themselves change while the transport runs).  Besides skipping the idle workgroups this spreads the live
    // columns evenly over the XCDs (workgroups are dealt round-robin over them, and the slow-converging columns of a
    // sweep tend to share their index modulo 8).
    int live = 0;
    const int* live_list = nullptr;
    // host side, ring kernel: the ring depth of this launch in the low byte (ring_slots_word; the launcher takes at least two and
    // as many as fit), above it the timing switches of a diagnostic build (-DSOSRT_RING_DEBUG), which reach the kernel as dbg_arg
    int slots = 0;
    // most zones of any column of the batch (>= kRingZones): sizes the per-zone tables of the ring / chunk-parallel kernels and
    // selects their instantiation (beyond three zones: the one that tests the other boundaries too)
    int nzcap = kRingZones;
    // chunk-parallel kernel, ceil(N / 64) workgroups per column (transport_scan.hip): exchange rows and {arrivals, flags} per column
    int scan_split = 0;
    double* scan_scratch = nullptr;
    int* scan_sync = nullptr;
    // ring kernel and chunk-parallel kernel, moment mode (plan_order: LaunchPlan::moments / ::scan_moments): the plain rows' source comes as moment records
    // [B][L][kMomDoubles] (jn_gemm_tile.hpp, lowrank_rows) and is expanded with the factor V of W_atm = U V; Jn then holds
    // the slab rows only.  Null: every row of Jn is read, as always.
    const double* mom = nullptr;
    const double* lrV = nullptr;   // [kLowRankMax][D]
    int lr_rank = 0;
};
void launch_transport_fast(hipStream_t s, dim3 grid, dim3 block, const TransportArgs& a);
// transport_ring.hip: same sweeps, rows streamed through an LDS ring by loader waves
bool transport_ring_ok(const Grid& g);
bool transport_ring_fits(const Grid& g, int nzcap);            // ... with the per-zone tables of up to nzcap zones
constexpr int ring_slots_word(int depth, int debug) { return (depth < 0 ? 0 : (depth > 255 ? 255 : depth)) | (debug << 8); }
void launch_transport_ring(hipStream_t s, dim3 grid, const TransportArgs& a, int slots, int debug);
// transport_scan.hip: the chunks of a sweep dealt to several waves (chunk-local recurrence + carried values)
bool transport_scan_ok(const Grid& g);
bool transport_scan_split_ok(const Grid& g);
bool transport_scan_wide(const Grid& g);                       // ... of which the shapes that take the split form's WIDE instantiation
bool transport_scan_fits(const Grid& g, int nzcap, bool split);
int transport_scan_parts(const Grid& g);                       // workgroups per column of the split form: ceil(N / 64)
size_t transport_scan_scratch_doubles();                       // per column
void launch_transport_scan(hipStream_t s, dim3 grid, const TransportArgs& a);
// order_loop.hip: the last orders of a few live columns in ONE launch (transport and contraction as roles of its workgroups)
constexpr int kOrderLoopMaxCols = 256;                 // live columns a launch takes at most
// words of the launch in global memory (ints, zeroed before the launch): launch-wide ones on lines of their own, then per live column
constexpr int kOlArrive = 0, kOlState = 32, kOlLeft = 64, kOlAbort = 96, kOlOrders = 100, kOlCols = 128;
constexpr int kOlColStride = 64, kOlOrdDone = 0, kOlColStop = 1, kOlJnDone = 32;
constexpr int kOlReady = 1, kOlNotResident = 2, kOlAborted = 3;            // state of a launch, as reported to the host
inline size_t order_loop_sync_ints(int cols) { return (size_t)kOlCols + (size_t)cols * kOlColStride; }

// what the first kernel of a solve does besides the zone tables (all null: nothing)
struct SolveSetup {
    int* zero_next = nullptr;            // [n_zero] counters of the next solve
    int n_zero = 0;
    int* redo = nullptr;                 // [B] per-column redo flags, cleared
    unsigned long long* hash = nullptr;  // [B] hash of the column's optical-depth profile
    int* scan_sync = nullptr;            // [B][2] exchange words of the chunk-parallel transport's split form, cleared
};
void launch_prepare(hipStream_t s, const Grid& g, int B, int geom, int surface, ColScalars sc, const double* tau,
                    ColDesc* desc, double* rowcoef_a, double* rowcoef_r, int* need_small = nullptr, SolveSetup su = SolveSetup());
void launch_first_order_readme(hipStream_t s, const Grid& g, const double* w, int B, const double* tau, const double* P0a,
                               const double* P0r, const ColDesc* desc, double* I1_out, double* I_out, double* saved,
                               size_t saved_col_stride, Conv cv, int do_conv);
void launch_first_order(hipStream_t s, const Grid& g, int B, const double* tau, const double* P0a, const double* P0r,
                        const ColDesc* desc, double* I1_out, double* I_out, double* saved, size_t saved_col_stride,
                        Conv cv, int do_conv, int p0r_zones = 0 /* > 0: P0r is [B][p0r_zones][D], zone z of a column reads its row z */);
// Jn = diag(ca) A Wa for the rows of `rows_main`, and diag(ca) A Wa + diag(cr) A Wr for the rows of
// `rows_slab` (spec:321), in one launch.  Row lists hold global row ids; rows_main == nullptr means
// the identity list 0..n_main-1.
struct GemmArgs {
    const double* A;
    const double* Wa;
    const double* Wr;
    const double* ca;      // per-row coefficients
    const double* cr;
    const int* rows_main;
    int n_main;
    const int* rows_slab;
    int n_slab;
    int D, Dp, Wld, L;
    double* C;
    const int* active;     // nullable: skip tiles whose columns have all converged
    // k_jn_gemm_tail only: tiles are laid over the live columns (the i-th group of workgroups finds the
    // i-th live column itself), not over the row lists
    int B = 0;
    int col0 = 0;                    // the launch covers the columns [col0, col0 + B) of the batch (all per-column arrays are whole-batch)
    const int* idx_up = nullptr;     // [batch] first / last slab row of a column; null: no slab rows
    const int* idx_down = nullptr;
    int max_main = 0, max_slab = 0;  // most plain / slab rows any column has
    const double* Wmix = nullptr;    // [groups][Dp][Wld] ca W_atm + cr W_aer per distinct slab coefficient pair; null: two passes
    const int* mix_group = nullptr;  // [B] group of a column
    int pad_lds = 0;                 // host side: unused dynamic LDS added to the launch (caps the workgroups per CU)
    int* live_list = nullptr;        // live-column tilings: [live_cap] the i-th live column (relative to col0), -1 beyond the live count
    int live_cap = 0;
    const int* slab_tile_group = nullptr;   // dense kernel: group of every 32-row tile of rows_slab (listed group by group, padded with -1)
    // The order loop's view of the batch: the first workgroup of the source-function launch of order
    // n+1 (which starts when order n has finished) writes {live columns after order n, tag} to pinned
    // host memory, where the host spins on the tag -- no copy, no event, no stream drain.
    const int* nactive = nullptr;    // [1]: live columns of this column group
    const int* need_small = nullptr; // [1]: whether any column of the batch needs k_smallmu (set by k_prepare)
    int* host_pub = nullptr;         // pinned [2 slots][4] = {live, tag, needs k_smallmu, -}; slot = tag & 1
    int tag = 0;
    // flip-symmetric contraction (jn_gemm.hip, SYM): Wa / Wr / Wmix then hold the folded matrices [k < Ks][S | A]
    int sym = 0;
    int Ks = 0;                      // N rounded up to the k-chunk
    int check_tiles = 1;             // dense kernel: skip the tiles whose columns have all converged (two barriers and a dependent load per tile)
    // low-rank form of the plain rows (jn_gemm_tile.hpp, lowrank_rows): W_atm = U V with lr_rank <= kLowRankMax terms; -1: the
    // plain rows are tiles of the MFMA product like the slab rows
    int lr_rank = -1;
    const double* lrU = nullptr;     // [kLowRankMax][D]: lrU[q][k] = U[k][q]
    const double* lrV = nullptr;     // [kLowRankMax][D]: lrV[q][m] = V[q][m]
    // Moment records of the plain rows, [rows][kMomDoubles] indexed like C's rows: {M_0 .. M_3, ca, padding}.  Set: lowrank_rows
    // writes a row's record and NOT its row of C (the ring transport expands the record itself, transport_util.hpp: lr_expand).
    // Null: rows of C, as always.  Never set for the order loop's contraction role or with atmosphere sets.
    double* mom = nullptr;
    // dense launch, low-rank plain rows without atmosphere sets: rows of the plain list a stream workgroup takes (launch_gemm sets it)
    int lr_run = 0;
};
// Atmosphere phase sets in use (sosrt_set_atmosphere_sets): a plain row takes the factors of its column's set.  The launches
// that read this are kernels of their own (jn_gemm.hip, *_atm) with this as a second argument, and GemmArgs::lrU / lrV are then
// [sets][kLowRankMax][D]; the kernels of a handle without such sets are the code, and the arguments, they always were.
struct AtmSets {
    const int* col_atm = nullptr;    // [batch] atmosphere set of a column (indexed like GemmArgs::active)
    const int* lr_ranks = nullptr;   // [sets] rank of a set's factors (0 .. kLowRankMax)
};
constexpr int kLowRankMax = 4;
// The dense launch's stream of low-rank plain rows (jn_gemm_tile.hpp, lowrank_stream): a workgroup takes a run of the plain list
// long enough for a software pipeline over its waves' batches of 4 rows -- the list dealt over kLrStreamRounds rounds of the
// launch's resident workgroups (four to a CU), in whole batches per wave, at most 64 rows a wave (its lanes hold the row ids).
#ifndef SOSRT_LR_STREAM_ROUNDS
#define SOSRT_LR_STREAM_ROUNDS 2
#endif
constexpr int kLrStreamRounds = SOSRT_LR_STREAM_ROUNDS;
inline int lr_stream_run(int n_main, int cus) {
    const long long wgs = (long long)(cus > 0 ? cus : 256) * 4 * kLrStreamRounds;
    const long long run = ((n_main + wgs - 1) / wgs + 15) / 16 * 16;
    return (int)(run < 16 ? 16 : (run > 256 ? 256 : run));
}
constexpr int kMomDoubles = 8;     // a moment record: 64 bytes, 64-byte aligned

// (publish_live_now: by the calling thread, whichever workgroup it belongs to)
__device__ inline void publish_live_now(const GemmArgs& g) {
    const int live = __hip_atomic_load(g.nactive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int* slot = g.host_pub + 4 * (g.tag & 1);
    __hip_atomic_store(slot, live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 2, g.need_small ? g.need_small[0] : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 1, g.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ inline void publish_live(const GemmArgs& g) {
    if (g.host_pub && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) publish_live_now(g);
}
// A kernel's opt-in to more than 64 KB of dynamic LDS (hipFuncSetAttribute) is made once per DEVICE: a process may hold handles on
// several GPUs (sosrt_create(device = k)), and the attribute set under one device does not reach the kernel's object on another.
struct PerDeviceOnce {
    bool seen[64] = {};
    bool first() {                                   // true the first time the current device asks
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return true;
        if (seen[d]) return false;
        seen[d] = true;
        return true;
    }
};
void launch_gemm(hipStream_t s, const GemmArgs& a, const AtmSets* at = nullptr, int cus = 0 /* CUs of the device: sizes the stream's runs */);
struct OrderLoopArgs {
    TransportArgs t;           // the column group's view (every per-column pointer offset to its first column): g, tau, Jn, I, desc, cv, Etab, erep, scan_scratch, scan_sync
    GemmArgs gm;               // the batch's view (whole-batch pointers, global column ids): folded matrices, Wmix, mix_group, idx_up / idx_down, ca / cr, C = Jn
    const double* in0;         // operand of the launch's first contraction (whole batch)
    double* gbufP;             // In of the launch's odd / even orders (whole batch) ...
    double* gbufQ;
    double* bufP;              // ... and the same from the group's first column
    double* bufQ;
    int order0;                // scattering order n of the launch's first order
    int kmax;                  // orders the launch runs at most
    int B, col0;               // the group's columns: [col0, col0 + B) of the batch
    int fixcap;
    int* sync;                 // order_loop_sync_ints(cap) zeroed ints
    int* host_done;            // pinned {status, tag}
    int tag;
    unsigned long long* log = nullptr;   // diagnostic builds (-DSOSRT_OL_STAMPS): [1 + 65000] event log, log[0] = count
    int astage = 0;            // (set by the launcher) the contraction role stages its tiles' rows of In_1 whole in LDS
};
bool order_loop_ok(const Grid& g, bool split);
int order_loop_parts(const Grid& g, bool split);
hipError_t launch_order_loop(hipStream_t s, int grid, bool split, const OrderLoopArgs& p);
// jn_gemm_f32.hip: the contraction with float operands and a float accumulator (opt-in, tolerance study)
void launch_gemm_f32(hipStream_t s, const GemmArgs& a, const float* Wa32, const float* Wmix32);
void launch_to_float(hipStream_t s, size_t n, const double* src, float* dst);
void launch_wmix(hipStream_t s, size_t n, int ngroups, const double* Wa, const double* Wr, const double* ca, const double* cr,
                 double* Wmix, const int* gset = nullptr /* [ngroups] aerosol set of a group: Wr is then [sets][n] */,
                 const int* gatm = nullptr /* [ngroups] atmosphere set of a group: Wa is then [sets][n] */);
// device fold of S phase matrices P [S][D][D] into W [S][Dp][Wld] (W[k][m] = w_k P[m][D-1-k], the host fold's bits), and the
// partial maxima {max |W|, max |W - flip W|} of its flip-asymmetry measure, out [S][nblk][2]
void launch_fold_sets(hipStream_t s, int S, int D, int Wld, size_t per, const double* w, const double* P, double* W);
void launch_fold_asymmetry(hipStream_t s, int S, int nblk, int D, int Wld, size_t per, const double* W, double* out);
// the flip-symmetric folding [k][S | A] of `nmat` contraction matrices [Dp][Wld]
void launch_symfold(hipStream_t s, int nmat, int N, int D, int Dp, int Wld, const double* W, double* SA);
// some columns have converged (at most `cols` are live, an upper bound): workgroups only for live
// columns; small_tiles: 32-row tiles and deeper staging for the last few
void launch_gemm_tail(hipStream_t s, const GemmArgs& a, int cols, bool small_tiles, bool regs = false, const AtmSets* at = nullptr);
void launch_smallmu(hipStream_t s, const Grid& g, int B, const double* tau, const double* Jn, double* In,
                    const ColDesc* desc, const int* active);
// B workgroups' worth of columns (a.live of them when the launch runs over the live list): sizes the block and the LDS and
// dispatches on the kernel's name, nothing else
void launch_transport(hipStream_t s, TransportKernel kernel, int B, const TransportArgs& a);
bool transport_fast_ok(const Plan& plan);
// erep (nullable): tables are built only for columns with erep[b] == b
void launch_attenuation(hipStream_t s, const Grid& g, int B, const double* tau, double* Etab, const int* erep);
// erep[b] = first column with the same optical-depth profile as column b (hash[B] is scratch)
// need_small / host_flag / tag (nullable): publishes k_prepare's verdict on k_smallmu to pinned host memory {flag, tag}
void launch_tau_groups(hipStream_t s, const Grid& g, int B, const double* tau, unsigned long long* hash, int* erep,
                       const int* need_small = nullptr, int* host_flag = nullptr, int tag = 0);
void launch_fluxes(hipStream_t s, const Grid& g, int B, const double* tau, const double* I, const ColDesc* desc,
                   int beam_norm, double* fdn, double* fup);
// epilogue.hip: outputs of the epilogue (each nullable): [B][L] per level, net_toa [B]
struct EpilogueOut {
    double* flux_down;
    double* flux_up;
    double* diffusivity;
    double* heating_rate;
    double* net_toa;
};
// w: np.trapz weights on the whole direction grid [D]; z_profile [L] (nullable: no heating rate)
void launch_epilogue(hipStream_t s, const Grid& g, const double* w, int B, const double* tau, const double* I,
                     const ColDesc* desc, int beam_norm, const double* z_profile, const EpilogueOut& out);
constexpr int kMaxModes = 64;      // SOSRT_MAX_MODES
// out[b][lev][dir][j] (+)= (2 - delta_m0) I^m[b][levels[lev]][dir] cos(m phi[j])   (m == 0 writes, m >= 1 adds)
void launch_azimuth_accumulate(hipStream_t s, const Grid& g, int B, int m, const double* Im, int nlev, const int* levels,
                               int nphi_out, const double* phi, double* out);
// the whole sum in one launch: out[b][lev][dir][j] = I0[b][levels[lev]][dir] + sum_{m = 1..M} 2 Im[m-1][b][levels[lev]][dir] cos(m phi[j]),
// the terms added in ascending m (the bits of the sequence of launches above)
void launch_azimuth_synthesize(hipStream_t s, const Grid& g, int B, int M, const double* I0, const double* Im, int nlev,
                               const int* levels, int nphi_out, const double* phi, double* out);
// Lorenz-Mie tables (sosrt_mie_ensembles).  nlanes = S * R spheres, lane = s * R + i; x, nmax, nstart [nlanes]
// (size parameter, terms of the series, start of the downward recurrence: from the host, mie.mie_coefficients' counts);
// ab [nlanes][n_cap][4] and qw [nlanes][kMieQ] workspaces; tn [n_cap + 1]: (n + 1) / n; part [S][mie_chunks(R)][ntab].
constexpr int kMieQ = 6;           // Q_ext, Q_sca, Q_back, g, n(r), weight in the table
constexpr int kMieChunk = 4;       // radii per workgroup of the angle kernel (fixed: a batch and its single calls sum alike)
inline int mie_chunks(int R) { return (R + kMieChunk - 1) / kMieChunk; }
void launch_mie_coefficients(hipStream_t s, int nlanes, int R, int n_cap, const double* x, const int* nmax, const int* nstart,
                             const double* m_re, const double* m_im, const double* radii, const double* r_m, const double* sig,
                             double* ab, double* qw);
void launch_mie_angles(hipStream_t s, int S, int R, int ntab, int n_cap, const double* mu, const double* ab, const int* nmax,
                       const double* tn, const double* qw, double* part);
void launch_mie_integrate(hipStream_t s, int S, int R, int ntab, const double* part, const double* radii, const double* qw,
                          double* p, double* bulk);
// view.hip: radiance at view cosines off the direction grid.  The signed view cosines (first the V downward
// lanes -mu_view, then the V upward ones) and the requested levels travel by value in the kernel arguments: nothing is staged.
constexpr int kMaxViews = 64;      // SOSRT_MAX_VIEWS
constexpr int kViewLevels = 256;   // levels per launch of the sweeps (a call with more takes several)
struct ViewMu {
    double s[2 * kMaxViews];
};
struct ViewLevels {
    int n;
    int t[kViewLevels];
};
// out [n][nphi_out] (+)= (2 - delta_m0) val[n] cos(m phi[j]), n = B nlev 2V   (m == 0 writes, m >= 1 adds; epilogue.hip)
void launch_view_azimuth_accumulate(hipStream_t s, size_t n, int m, const double* val, int nphi_out, const double* phi, double* out);
// S [nrows][2V] = diag(ca) Isrc W_atm + diag(cr) Isrc W_aer with the rows folded into Wfold [view_source_kpad(D)][view_source_cols(V)]
// (scratch); rows_aer may be null (single slab: zeros)
int view_source_cols(int V);
int view_source_kpad(int D);
void launch_view_source(hipStream_t s, int nrows, int D, int V, const double* w, const double* rows_atm, const double* rows_aer,
                        const double* Isrc, const double* ca, const double* cr, double* Wfold, double* S);
// out [B][nlev_all][2V] (offset to the first level of lv): the sweeps of S, the closed-form first order
void launch_view_transport(hipStream_t s, int B, int V, int L, int quad, int nlev_all, const double* tau, const double* S,
                           const ColDesc* desc, const ViewMu& mu, const ViewLevels& lv, double* out);
void launch_view_first_order(hipStream_t s, int B, int V, int L, int nlev_all, const double* tau, const double* p0a,
                             const double* p0r, const ColDesc* desc, const ViewMu& mu, const ViewLevels& lv, double* out);
void launch_limit_rows(hipStream_t s, const Grid& g, int R, int table, const double* rows, double* out);
void launch_asymptotic(hipStream_t s, int R, int stride, const int* len, const double* J, const double* tau,
                       const double* tau_t, const double* mu, double* out);
void launch_finalize(hipStream_t s, int B, Conv cv, int max_orders, int* n_out = nullptr, int* status_out = nullptr);
void launch_bench(hipStream_t s, int which, double* a, double* b, size_t n, int iters);

}  // namespace sosrt
