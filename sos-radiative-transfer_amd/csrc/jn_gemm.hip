// k_jn_gemm: the source function of one scattering order for every layer of every column,
//     Jn[r][:] = ca[r] (In_1[r][:] @ W_atm)  (+ cr[r] (In_1[r][:] @ W_aer) for aerosol-slab rows)
// (spec:314-323, I1_In:62-74) as an FP64-MFMA contraction.
//
// v_mfma_f64_16x16x4_f64: lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; the four
// results of lane l are D[i = 4r + (l>>4)][j = l&15], r = 0..3.
//
// Workgroup tile: 64 rows x 128 columns, 4 waves, each wave 4x2 MFMA tiles (64 accumulator
// registers).  Operands are staged through LDS in k-chunks of GEMM_KC = 16 with row strides chosen for
// the fragment READS (ds_read_b64: A rows 18 doubles, W rows 144 doubles = 32 mod 64 dwords, so the 32
// lanes of a half wave fall into 64 distinct banks).  The kernel is not free of bank conflicts, though:
// the staging STORES are 16 bytes per lane, four lanes per 18-double row, and SQ_LDS_BANK_CONFLICT counts
// 8.9e6 cycles per launch of the symmetric form, 18 % of the launch's CU-cycles, against an MFMA pipe
// busy for 47 % of the SIMD-cycles (profiles/r04_pmc_gemm_sq.txt; round 2's "conflict free" was the reads).
// The global loads of the next chunk are in registers while the current one
// is multiplied (one chunk ahead in the dense tilings, four workgroups per CU hide the rest; two chunks
// ahead in two register sets, loop unrolled by two, in the tail tiling, where a workgroup is alone on
// its CU).
//
// Rows are addressed through row lists, so that one launch covers the plain rows (against W_atm) and the
// slab rows (against the combined matrix ca W_atm + cr W_aer of their coefficient pair, one pass; two
// passes, W_atm then W_aer, only when a batch has more distinct pairs than the cache of combined matrices)
// without either writing the other's rows; the per-row coefficient is applied to the A operand on its way
// into LDS.
//
// Two forms of the product (chosen per handle from the matrices, never from the batch): the full D x D
// product, and -- when the folded matrices are flip-symmetric, as every phase function of the scattering
// angle makes them -- two N x N products on the sum and the difference of a row's two halves (SYM below):
// half the flops.
//
// The plain rows need no product at all when W_atm has a low rank (SOSRT_CONTRACT_F64, g.lr_rank >= 0: Rayleigh
// r = 2, iso r = 1; sosrt_set_phase certifies max |W_atm - U V| <= 1e-12 max |W_atm|): Jn = ca (In_1 U) V, r dot
// products and an r-term expansion per row, 16 D bytes of HBM and no MFMA (jn_gemm_tile.hpp: lowrank_rows, and for a handle
// without atmosphere sets lowrank_stream).  The launches keep their duties, and the live-column tilings their grids: a workgroup
// that would have held a tile of plain rows streams its share of that tile's rows instead, and the slab tiles -- now the long
// ones -- are numbered first.  The dense launch of such a handle is its slab tiles' workgroups, then stream workgroups with a
// run of the plain list each (launch_gemm, jn_gemm_dense).
#include "jn_gemm_tile.hpp"

namespace sosrt {

namespace {

// MFMA row tiles of a slab-row workgroup of the dense tiling: the slab rows are the last workgroups of a launch, and the last
// (partial) round of workgroups costs a whole tile's time whatever its fill -- with 16-row slab tiles (1) instead of 32-row ones (2)
// that round is twice as full and half as long.  (A row's arithmetic does not depend on its tile's height: the live-column tilings
// have always used 16-row slab tiles.)
#ifndef SOSRT_DENSE_SLAB_RT
#define SOSRT_DENSE_SLAB_RT 1
#endif
constexpr int DENSE_SLAB_RT = SOSRT_DENSE_SLAB_RT;
#ifndef SOSRT_LIVE_TILE_MAJOR
#define SOSRT_LIVE_TILE_MAJOR 1
#endif
constexpr int DENSE_SLAB_ROWS = 16 * DENSE_SLAB_RT;

// The live columns of the launch's group, in ascending order, for the transport of this order (live_list[i] = i-th live column
// relative to col0, -1 from the live count up to live_cap): one workgroup.  The live-column tilings write the list as they find
// their columns; the dense tiling has no such step, and a transport launched over ALL columns of a half-converged batch leaves
// its live columns where the batch put them -- two to a CU here, none there: 124 us for 271 live columns of 512 where the same
// kernel over the list takes 75 (profiles/r04_order_table.txt, orders 11-13).
__device__ __forceinline__ void write_live_list(const GemmArgs& g) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int before = 0;
    for (int base = 0; base < g.B; base += 256) {
        const bool f = base + tid < g.B && g.active[g.col0 + base + tid] != 0;
        const unsigned long long mk = __ballot(f);
        if (lane == 0) s_cnt[wave] = __popcll(mk);
        __syncthreads();
        int pre = before, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pre += s_cnt[w];
            tot += s_cnt[w];
        }
        const int at = pre + __popcll(mk & ((1ull << lane) - 1));
        if (f && at < g.live_cap) g.live_list[at] = base + tid;
        before += tot;
        __syncthreads();
    }
    for (int i = before + tid; i < g.live_cap; i += 256) g.live_list[i] = -1;
}

// ATM (here and below): the kernel of a batch with atmosphere phase sets in use -- its plain rows are always in the low-rank
// form, a row with the factors of its column's set (AtmSets); symmetric form only
template <bool SYM, bool ATM>
__device__ __forceinline__ void jn_gemm_dense(const GemmArgs& g, const AtmSets& at) {
    if (g.live_list && blockIdx.x == gridDim.x - 1) {    // (the launch's extra workgroup: launch_gemm)
        write_live_list(g);
        return;
    }
    publish_live(g);
    constexpr int kSA = (SYM ? 2 : 1) * 16 * (GEMM_RT > 2 ? GEMM_RT : 2) * A_LD, kSB = GEMM_KC * B_LD;
    __shared__ __attribute__((aligned(16))) double sA[kSA];
    __shared__ __attribute__((aligned(16))) double sB[kSB];
    __shared__ int s_any;
    // Workgroups are dealt round-robin over the 8 XCDs, each with its own L2.  The column tiles of one row
    // tile read the same rows of In_1: numbering them 8 apart puts them on one XCD, a few dispatches apart,
    // so that In_1 comes from HBM once instead of once per column tile.
    const int tiles_main = (g.n_main + 16 * GEMM_RT - 1) / (16 * GEMM_RT);
    const int tiles_slab = (g.n_slab + DENSE_SLAB_ROWS - 1) / DENSE_SLAB_ROWS;
    const int tiles = tiles_main + tiles_slab;
    const int nct = (g.D + GEMM_BN - 1) / GEMM_BN;
    const int id = blockIdx.x;
    if (!ATM && g.lr_rank >= 0) {
        // Low-rank plain rows, no atmosphere sets (launch_gemm sets lr_run and sizes the grid): the slab tiles' workgroups, numbered
        // as ever so that the column tiles of a slab tile share an XCD, then the stream workgroups, each with a run of lr_run entries
        // of the plain list, a quarter of it per wave -- a plain row is read by one workgroup only and has no use for the pairing.
        // No workgroup of this launch holds a TILE of plain rows: the ids that pad the slab tiles to a multiple of 8 leave.
        const int slab_ids = (tiles_slab + 7) / 8 * 8 * nct;
        if (id >= slab_ids) {
            const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x) >> 6;
            const int rw = g.lr_run >> 2, first = (id - slab_ids) * g.lr_run + wave * rw;
            lowrank_stream<true>(g, LrRun<ListRows>{ListRows{g.rows_main, g.n_main}, first, 1}, min(max(g.n_main - first, 0), rw), true,
                           sA, kSA, sB, kSB);
            return;
        }
    }
    int tile = (id / (8 * nct)) * 8 + (id & 7);
    const int bn0 = ((id >> 3) % nct) * GEMM_BN;
    if (tile >= tiles) return;
    if (ATM || g.lr_rank >= 0) {
        // low-rank plain rows: the short workgroups -- the slab tiles go first (renumbered to the end of the MFMA form's order)
        if (tile >= tiles_slab) {
            // (atmosphere sets: a workgroup streams its share of a tile of plain rows, batch by batch)
            if constexpr (ATM) lowrank_tile<false, ListRows, true>(g, ListRows{g.rows_main, g.n_main}, tile - tiles_slab, 16 * GEMM_RT, bn0, true, at);
            return;
        }
        tile += tiles_main;
    }
    if (tile < tiles_main) {
        gemm_tile<GEMM_RT, false, false, SYM>(g, sA, sB, &s_any, tile, bn0, ListRows{g.rows_main, g.n_main}, true);
    } else if (g.Wmix && g.slab_tile_group) {
        // the slab rows are listed group by group (one distinct coefficient pair per 32-row tile): one pass over the
        // group's combined matrix, the same arithmetic as the live-column tilings (a column's result does not
        // depend on which tiling, or which batch, it was computed in)
        const int st = tile - tiles_main;
        // (the host lists a group for every 32 slab rows)
        gemm_tile<DENSE_SLAB_RT, false, false, SYM>(g, sA, sB, &s_any, st, bn0, ListRows{g.rows_slab, g.n_slab}, true,
                                                    g.Wmix + (size_t)g.slab_tile_group[st * DENSE_SLAB_ROWS / 32] * g.Dp * g.Wld);
    } else if (g.slab_tile_group) {
        // two passes with several aerosol sets: the slab rows are listed set by set, and the second pass of a tile reads the
        // W_aer of its set (g.Wr: [sets][Dp][Wld])
        const int st = tile - tiles_main;
        GemmArgs gs = g;
        gs.Wr = g.Wr + (size_t)g.slab_tile_group[st * DENSE_SLAB_ROWS / 32] * g.Dp * g.Wld;
        gemm_tile<DENSE_SLAB_RT, true, false, SYM>(gs, sA, sB, &s_any, st, bn0, ListRows{g.rows_slab, g.n_slab}, true);
    } else {
        gemm_tile<DENSE_SLAB_RT, true, false, SYM>(g, sA, sB, &s_any, tile - tiles_main, bn0, ListRows{g.rows_slab, g.n_slab}, true);
    }
}
template <bool SYM>
__global__ __launch_bounds__(256, GEMM_WPS) void k_jn_gemm(GemmArgs g) { jn_gemm_dense<SYM, false>(g, AtmSets()); }
__global__ __launch_bounds__(256, GEMM_WPS) void k_jn_gemm_atm(GemmArgs g, AtmSets at) { jn_gemm_dense<true, true>(g, at); }

// The same contraction once some columns have converged.  Tiling the row lists would launch a
// workgroup for every tile of every column, and the few live tiles would queue behind thousands of
// workgroups that only find out that their columns have converged.  Here blockIdx.x = (i, tile): the
// workgroup finds the i-th live column itself (a prefix count over the live flags) and tiles that
// column's rows: 16-row tiles for the slab rows, scheduled first because their double pass over k is
// the critical path of the launch, then the tiles of the plain rows.
template <int RT, bool DEEP, bool SYM, bool ATM = false>
__device__ __forceinline__ void gemm_live_columns(const GemmArgs& g, double* sA, double* sB, const AtmSets& at = AtmSets()) {
    __shared__ int s_w[4];
    __shared__ int s_col;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ts = (g.max_slab + 16 * TAIL_RT_SLAB - 1) / (16 * TAIL_RT_SLAB);
    const int tm = (g.max_main + 16 * RT - 1) / (16 * RT);
    // same XCD-aware numbering as the dense kernel: the column tiles of a row tile 8 apart
    const int nct = (g.D + GEMM_BN - 1) / GEMM_BN;
    const int id = blockIdx.x;
    const int xq = (id / (8 * nct)) * 8 + (id & 7), bn0 = ((id >> 3) % nct) * GEMM_BN;
#if SOSRT_LIVE_TILE_MAJOR
    // Tile-major, the plain rows' tiles of every column first, the slab rows' 16-row tiles last: the last workgroups of a launch
    // decide how long its last, partly filled round of workgroups takes, and with the combined slab matrices (one pass over k) the slab
    // tiles are the short ones.  (Until round 3 a column's tiles were consecutive, slab tiles first -- from the time they made two
    // passes over k.)
    const int cap = g.live_cap > 0 ? g.live_cap : 1;
    const int tq = xq / cap, ci = xq % cap;
    if (tq >= ts + tm) return;                           // (uniform) padding of the grid
    // (low-rank plain rows: they are the short tiles, the slab tiles go first)
    const int tt = (ATM || g.lr_rank >= 0) ? tq : (tq < tm ? ts + tq : tq - tm);   // tt < ts: slab tile tt; else plain tile tt - ts
#else
    const int ci = xq / (ts + tm), tt = xq % (ts + tm);
#endif
    if (tid == 0) s_col = -1;
    int before = 0;
    for (int base = 0; base < g.B; base += 256) {
        const bool f = base + tid < g.B && g.active[g.col0 + base + tid] != 0;
        const unsigned long long mk = __ballot(f);
        if (lane == 0) s_w[wave] = __popcll(mk);
        __syncthreads();
        int pre = before, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pre += s_w[w];
            tot += s_w[w];
        }
        if (f && pre + __popcll(mk & ((2ull << lane) - 1)) == ci + 1) s_col = g.col0 + base + tid;
        before += tot;
        __syncthreads();
        if (before > ci) break;
    }
    const int b = s_col;
    // the transport of this order takes its columns from this list
    if (g.live_list && xq < (SOSRT_LIVE_TILE_MAJOR ? (g.live_cap > 0 ? g.live_cap : 1) : 1 << 30) &&
        (SOSRT_LIVE_TILE_MAJOR || tt == 0) && bn0 == 0 && tid == 0 && ci < g.live_cap)
        g.live_list[ci] = b < 0 ? -1 : b - g.col0;
    if (b < 0) return;                                   // fewer live columns than the host's (lagging) count
    const int iu = g.idx_up ? g.idx_up[b] : 0;
    const int ns = g.idx_up ? g.idx_down[b] - iu + 1 : 0;
    if (tt < ts) {
        if (tt * 16 * TAIL_RT_SLAB >= ns) return;
        if (g.Wmix)      // SLAB = false: a single pass, over the column's combined matrix
            gemm_tile<TAIL_RT_SLAB, false, DEEP, SYM>(g, sA, sB, nullptr, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true},
                                                      false, g.Wmix + (size_t)g.mix_group[b] * g.Dp * g.Wld);
        else if (g.mix_group) {                          // two passes, the second over the W_aer of the column's set
            GemmArgs gs = g;
            gs.Wr = g.Wr + (size_t)g.mix_group[b] * g.Dp * g.Wld;
            gemm_tile<TAIL_RT_SLAB, true, DEEP, SYM>(gs, sA, sB, nullptr, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true}, false);
        } else
            gemm_tile<TAIL_RT_SLAB, true, DEEP, SYM>(g, sA, sB, nullptr, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true}, false);
    } else {
        const int t2 = tt - ts;
        if (t2 * 16 * RT >= g.L - ns) return;
        // (the 64-row tiling keeps the batch-at-a-time form: its MFMA tile takes all 128 registers, and with the stream beside it in
        // one kernel the allocator spilled one of them)
        if (ATM || (RT == GEMM_RT && g.lr_rank >= 0))
            lowrank_tile<false, ColumnRows, ATM>(g, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, t2, 16 * RT, bn0, false, at);
        else if (g.lr_rank >= 0)
            lowrank_stream_tile(g, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, t2, 16 * RT, bn0, sA, (SYM ? 2 : 1) * 16 * RT * A_LD, sB, GEMM_KC * B_LD);
        else gemm_tile<RT, false, DEEP, SYM>(g, sA, sB, nullptr, t2, bn0, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, false);
    }
}

// many live columns: the tile of the dense kernel
template <bool SYM>
__global__ __launch_bounds__(256, SYM ? 4 : GEMM_WPS) void k_jn_gemm_cols(GemmArgs g) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[(SYM ? 2 : 1) * 16 * GEMM_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<GEMM_RT, false, SYM>(g, sA, sB);
}
__global__ __launch_bounds__(256, 4) void k_jn_gemm_cols_atm(GemmArgs g, AtmSets at) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[2 * 16 * GEMM_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<GEMM_RT, false, true, true>(g, sA, sB, at);
}
// few live columns: 32-row tiles (more workgroups, so more CUs take part) and deeper staging, since
// such a workgroup is alone on its CU
// (symmetric form: staged one chunk ahead like the dense tiling -- 94 registers, five workgroups per CU instead of three;
// with 55 to 200 live columns the launch is a few rounds of workgroups and the fuller CUs save a round: the tail of the
// contraction 0.63 -> 0.57 ms per step.  The full product keeps the two-chunk staging it was tuned with.)
constexpr bool kTailDeepSym = false;
constexpr int kTailWpsSym = 4;
template <bool SYM>
__global__ __launch_bounds__(256, SYM ? kTailWpsSym : 2) void k_jn_gemm_tail(GemmArgs g) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[(SYM ? 2 : 1) * 16 * TAIL_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<TAIL_RT, SYM ? kTailDeepSym : true, SYM>(g, sA, sB);
}
__global__ __launch_bounds__(256, kTailWpsSym) void k_jn_gemm_tail_atm(GemmArgs g, AtmSets at) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[2 * 16 * TAIL_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<TAIL_RT, kTailDeepSym, true, true>(g, sA, sB, at);
}
// the last few columns (at most kTailDeepCols live): a workgroup is alone on its CU and every k-chunk is a trip to L2 or HBM that
// nothing else hides, so both operands are staged two chunks ahead (the register budget no longer matters: one workgroup per CU)
constexpr int kTailDeepCols = 32;
__global__ __launch_bounds__(256, 2) void k_jn_gemm_tail_deep(GemmArgs g) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[2 * 16 * TAIL_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<TAIL_RT, true, true>(g, sA, sB);
}
__global__ __launch_bounds__(256, 2) void k_jn_gemm_tail_deep_atm(GemmArgs g, AtmSets at) {
    publish_live(g);
    __shared__ __attribute__((aligned(16))) double sA[2 * 16 * TAIL_RT * A_LD];
    __shared__ __attribute__((aligned(16))) double sB[GEMM_KC * B_LD];
    gemm_live_columns<TAIL_RT, true, true, true>(g, sA, sB, at);
}

// the last handful of columns (api.hip: plan_order, SOSRT_PLAN_GEMM_LIVE16_REGS): one tile's latency is the launch's, so the tile
// keeps its share of the folded matrix in registers and has no barrier in its k-loop (jn_gemm_tile.hpp: gemm_tile_lone), and the
// way to the tile is three memory round trips -- live flags; the column's slab rows and matrix group, requested together; operands
// -- with the report to the host on a workgroup of its own (the last one: its release at system scope and the load in front of it
// would otherwise be in front of the first tile).  Tile-major numbering as in gemm_live_columns, 16-row tiles for all rows.
template <bool ATM>
__device__ __forceinline__ void jn_gemm_lone(const GemmArgs& g, const AtmSets& at) {
    extern __shared__ __attribute__((aligned(16))) double s_lone[];
    __shared__ int s_w[4];
    __shared__ int s_col[4];                             // the tile's column, its first slab row, slab rows, matrix group
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        if (g.host_pub && tid == 0) publish_live_now(g);
        return;
    }
    const int ts = (g.max_slab + 15) / 16, tm = (g.max_main + 15) / 16;
    const int nct = (g.D + GEMM_BN - 1) / GEMM_BN;
    const int id = blockIdx.x;
    const int xq = (id / (8 * nct)) * 8 + (id & 7), bn0 = ((id >> 3) % nct) * GEMM_BN;
    const int cap = g.live_cap > 0 ? g.live_cap : 1;
    const int tq = xq / cap, ci = xq % cap;
    if (tq >= ts + tm) return;                           // (uniform) padding of the grid
    // tt < ts: slab tile tt; else plain tile tt - ts (the short slab tiles last -- low-rank plain rows: those are the short ones)
    const int tt = (ATM || g.lr_rank >= 0) ? tq : (tq < tm ? ts + tq : tq - tm);
    // The ci-th live column of the launch and, in the same round trip, what the tile needs to know of it: every thread looks at
    // one candidate column's flag and descriptors.  The requests of the first 256 candidates leave before anything else ...
    int fl = 0, iu_c = 0, id_c = -1, mg_c = 0;
    if (tid < g.B) {
        const int c = g.col0 + tid;
        fl = g.active[c];
        if (g.idx_up) {
            iu_c = g.idx_up[c]; id_c = g.idx_down[c];
            if (g.mix_group) mg_c = g.mix_group[c];
        }
    }
    // ... and behind them, for a plain tile, the first two register blocks of its matrix: W_atm whatever the column
    LoneFrag f0, f1;
    const int nkb = (g.Ks >> 2) / LONE_KB;
    if (!ATM && tt >= ts && g.lr_rank < 0) {
        const int mcol = (bn0 >> 1) + (__builtin_amdgcn_readfirstlane(tid) >> 6) * 16 + (lane & 15);
        const __amdgpu_buffer_rsrc_t rW = make_rsrc(g.Wa, g.Dp * g.Wld * 8);
        lone_load(f0, rW, 0, lane >> 4, g.Wld, g.Wld >> 1, mcol);
        if (nkb > 1) lone_load(f1, rW, 1, lane >> 4, g.Wld, g.Wld >> 1, mcol);
    }
    if (tid == 0) s_col[0] = -1;
    int before = 0;
    for (int base = 0;; base += 256) {
        const bool f = fl != 0;
        const unsigned long long mk = __ballot(f);
        if (lane == 0) s_w[wave] = __popcll(mk);
        __syncthreads();
        int pre = before, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pre += s_w[w];
            tot += s_w[w];
        }
        if (f && pre + __popcll(mk & ((2ull << lane) - 1)) == ci + 1) {
            s_col[0] = g.col0 + base + tid; s_col[1] = iu_c; s_col[2] = id_c - iu_c + 1; s_col[3] = mg_c;
        }
        before += tot;
        __syncthreads();
        if (before > ci || base + 256 >= g.B) break;
        fl = 0;                                          // the next 256 candidates (a group of more than 256 columns)
        if (base + 256 + tid < g.B) {
            const int c = g.col0 + base + 256 + tid;
            fl = g.active[c];
            if (g.idx_up) {
                iu_c = g.idx_up[c]; id_c = g.idx_down[c];
                if (g.mix_group) mg_c = g.mix_group[c];
            }
        }
    }
    const int b = s_col[0];
    // the transport of this order takes its columns from this list
    if (g.live_list && tq == 0 && bn0 == 0 && tid == 0 && ci < g.live_cap) g.live_list[ci] = b < 0 ? -1 : b - g.col0;
    if (b < 0) return;                                   // fewer live columns than the host's (lagging) count
    const int iu = g.idx_up ? s_col[1] : 0, ns = g.idx_up ? s_col[2] : 0, mg = s_col[3];
    if (tt < ts) {
        if (tt * 16 >= ns) return;
        if (g.Wmix) gemm_tile_lone<false, false>(g, s_lone, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true}, f0, f1, g.Wmix + (size_t)mg * g.Dp * g.Wld);
        else if (g.mix_group) {                          // two passes, the second over the W_aer of the column's set
            GemmArgs gs = g;
            gs.Wr = g.Wr + (size_t)mg * g.Dp * g.Wld;
            gemm_tile_lone<true, false>(gs, s_lone, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true}, f0, f1);
        } else gemm_tile_lone<true, false>(g, s_lone, tt, bn0, ColumnRows{b * g.L, iu, ns, ns, true}, f0, f1);
    } else {
        if ((tt - ts) * 16 >= g.L - ns) return;
        if (ATM) lowrank_tile<false, ColumnRows, true>(g, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, tt - ts, 16, bn0, false, at);
        else if (g.lr_rank >= 0)         // (the factors in the two halves of the tile's 16 rows of D + 2 doubles: 4 D doubles fit each)
            lowrank_stream_tile(g, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, tt - ts, 16, bn0, s_lone, 8 * (g.D + 2), s_lone + 8 * (g.D + 2), 8 * (g.D + 2));
        else gemm_tile_lone<false, true>(g, s_lone, tt - ts, bn0, ColumnRows{b * g.L, iu, ns, g.L - ns, false}, f0, f1);
    }
}
__global__ __launch_bounds__(256, 1) void k_jn_gemm_lone(GemmArgs g) { jn_gemm_lone<false>(g, AtmSets()); }
__global__ __launch_bounds__(256, 1) void k_jn_gemm_lone_atm(GemmArgs g, AtmSets at) { jn_gemm_lone<true>(g, at); }

}  // namespace

void launch_gemm_tail(hipStream_t s, const GemmArgs& a, int cols, bool small_tiles, bool regs, const AtmSets* at) {
    if (regs && a.sym) {
        const int ts = (a.max_slab + 15) / 16, tm = (a.max_main + 15) / 16;
        if (cols <= 0 || ts + tm <= 0) return;
        const int nct = (a.D + GEMM_BN - 1) / GEMM_BN;
        const int lds = 16 * (a.D + 2) * 8;
        static PerDeviceOnce big_lds;                           // (more than 64 KB of dynamic LDS from N = 256 on)
        if (big_lds.first()) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_jn_gemm_lone), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_jn_gemm_lone_atm), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        }
        // (+ 1: the workgroup that reports to the host)
        const dim3 lgrid((unsigned)((cols * (ts + tm) + 7) / 8 * 8 * nct + 1));
        if (at) hipLaunchKernelGGL(k_jn_gemm_lone_atm, lgrid, dim3(256), (size_t)lds, s, a, *at);
        else hipLaunchKernelGGL(k_jn_gemm_lone, lgrid, dim3(256), (size_t)lds, s, a);
        return;
    }
    const int rt = small_tiles ? TAIL_RT : GEMM_RT;
    const int ts = (a.max_slab + 16 * TAIL_RT_SLAB - 1) / (16 * TAIL_RT_SLAB);
    const int tm = (a.max_main + 16 * rt - 1) / (16 * rt);
    if (cols <= 0 || ts + tm <= 0) return;
    const int nct = (a.D + GEMM_BN - 1) / GEMM_BN;
    dim3 grid((unsigned)((cols * (ts + tm) + 7) / 8 * 8 * nct));
    if (at) {                                            // atmosphere sets in use (api.hip: symmetric form only)
        if (small_tiles && cols <= kTailDeepCols) hipLaunchKernelGGL(k_jn_gemm_tail_deep_atm, grid, dim3(256), 0, s, a, *at);
        else if (small_tiles) hipLaunchKernelGGL(k_jn_gemm_tail_atm, grid, dim3(256), 0, s, a, *at);
        else hipLaunchKernelGGL(k_jn_gemm_cols_atm, grid, dim3(256), (size_t)a.pad_lds, s, a, *at);
        return;
    }
    if (small_tiles) {
        if (a.sym && cols <= kTailDeepCols) hipLaunchKernelGGL(k_jn_gemm_tail_deep, grid, dim3(256), 0, s, a);
        else if (a.sym) hipLaunchKernelGGL(k_jn_gemm_tail<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_jn_gemm_tail<false>, grid, dim3(256), 0, s, a);
    } else {
        if (a.sym) hipLaunchKernelGGL(k_jn_gemm_cols<true>, grid, dim3(256), (size_t)a.pad_lds, s, a);
        else hipLaunchKernelGGL(k_jn_gemm_cols<false>, grid, dim3(256), (size_t)a.pad_lds, s, a);
    }
}

// Wmix[g] = ca[g] W_atm + cr[g] W_aer for every distinct slab coefficient pair of the batch; with several aerosol phase sets
// (gset: the set of a group, Wr: [sets][n]) a group is a distinct (set, ca, cr) and reads the W_aer of its set -- the same
// expression, so a group's matrix has the bits it has in a batch of its set alone; with atmosphere sets in use (gatm: Wa is
// [sets][n]) a group is a distinct (atmosphere set, aerosol set, ca, cr) and reads the W_atm of its set as well
__global__ void k_wmix(size_t n, int ngroups, const double* __restrict__ Wa, const double* __restrict__ Wr,
                       const double* __restrict__ ca, const double* __restrict__ cr, double* __restrict__ Wmix,
                       const int* __restrict__ gset) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (gset) {
        const double a = Wa[i];
        for (int gq = 0; gq < ngroups; ++gq) {
            const double r = Wr[(size_t)gset[gq] * n + i];
            Wmix[(size_t)gq * n + i] = ca[gq] * a + cr[gq] * r;
        }
        return;
    }
    const double a = Wa[i], r = Wr[i];
    for (int gq = 0; gq < ngroups; ++gq) Wmix[(size_t)gq * n + i] = ca[gq] * a + cr[gq] * r;
}
// atmosphere sets too (a kernel of its own: k_wmix stays the code it was)
__global__ void k_wmix_atm(size_t n, int ngroups, const double* __restrict__ Wa, const double* __restrict__ Wr,
                           const double* __restrict__ ca, const double* __restrict__ cr, double* __restrict__ Wmix,
                           const int* __restrict__ gset, const int* __restrict__ gatm) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int gq = 0; gq < ngroups; ++gq) {
        const double a = Wa[(size_t)gatm[gq] * n + i];
        const double r = Wr[(size_t)(gset ? gset[gq] : 0) * n + i];
        Wmix[(size_t)gq * n + i] = ca[gq] * a + cr[gq] * r;
    }
}
void launch_wmix(hipStream_t s, size_t n, int ngroups, const double* Wa, const double* Wr, const double* ca, const double* cr,
                 double* Wmix, const int* gset, const int* gatm) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (gatm) hipLaunchKernelGGL(k_wmix_atm, grid, dim3(256), 0, s, n, ngroups, Wa, Wr, ca, cr, Wmix, gset, gatm);
    else hipLaunchKernelGGL(k_wmix, grid, dim3(256), 0, s, n, ngroups, Wa, Wr, ca, cr, Wmix, gset);
}

// The fold of sosrt_set_phase on the device: W[q][k][m] = w_k P[q][m][D-1-k] for S matrices P [S][D][D] -> W [S][Dp][Wld]
// (the padding is zeroed by the caller).  One product per element, the host fold's (plan.cpp, Plan::fold): the same bits.
// 32 x 32 tiles through LDS, so that the transposed read and the write are both along rows.
__global__ __launch_bounds__(256) void k_fold_sets(int D, int Wld, size_t per, const double* __restrict__ w,
                                                   const double* __restrict__ P, double* __restrict__ W) {
    __shared__ double tile[32][33];
    const int q = blockIdx.z, k0 = blockIdx.y * 32, m0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const double* Pq = P + (size_t)q * D * D;
    for (int j = ty; j < 32; j += 8) {                  // tile[j][i] = P[m0 + j][D-1-(k0 + i)]
        const int m = m0 + j, k = k0 + tx;
        if (m < D && k < D) tile[j][tx] = Pq[(size_t)m * D + (D - 1 - k)];
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {                  // W[k0 + i][m0 + tx] = w[k0 + i] * tile[tx][i]
        const int k = k0 + i, m = m0 + tx;
        if (k < D && m < D) W[(size_t)q * per + (size_t)k * Wld + m] = w[k] * tile[tx][i];
    }
}
void launch_fold_sets(hipStream_t s, int S, int D, int Wld, size_t per, const double* w, const double* P, double* W) {
    const unsigned nt = (unsigned)((D + 31) / 32);
    hipLaunchKernelGGL(k_fold_sets, dim3(nt, nt, (unsigned)S), dim3(256), 0, s, D, Wld, per, w, P, W);
}

// The flip-asymmetry measure of sosrt_set_phase on folded device matrices W [S][Dp][Wld]: per matrix and per block of the grid
// out[q][blk] = { max |W[k][m]|, max |W[k][m] - W[D-1-k][D-1-m]| }, NaN in both when the block met a NaN (fmax drops NaN
// operands, hence the flag).  Maxima and one division on the host: the host loop's value for NaN-free matrices.
__global__ __launch_bounds__(256) void k_fold_asymmetry(int D, int Wld, size_t per, const double* __restrict__ W,
                                                        double* __restrict__ out) {
    __shared__ double s_w[4], s_a[4];
    __shared__ int s_nan[4];
    const int q = blockIdx.y, tid = threadIdx.x;
    const double* Wq = W + (size_t)q * per;
    double wmax = 0, amax = 0;
    int nan = 0;
    const size_t n = (size_t)D * D;
    for (size_t e = (size_t)blockIdx.x * 256 + tid; e < n; e += (size_t)gridDim.x * 256) {
        const int k = (int)(e / D), m = (int)(e % D);
        const double x = Wq[(size_t)k * Wld + m], y = Wq[(size_t)(D - 1 - k) * Wld + (D - 1 - m)];
        const double ax = fabs(x), d = fabs(x - y);
        nan |= (ax != ax) || (d != d);
        wmax = fmax(wmax, ax); amax = fmax(amax, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wmax = fmax(wmax, __shfl_xor(wmax, o, 64)); amax = fmax(amax, __shfl_xor(amax, o, 64));
        nan |= __shfl_xor(nan, o, 64);
    }
    if ((tid & 63) == 0) { s_w[tid >> 6] = wmax; s_a[tid >> 6] = amax; s_nan[tid >> 6] = nan; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i) { wmax = fmax(wmax, s_w[i]); amax = fmax(amax, s_a[i]); nan |= s_nan[i]; }
        double* o = out + ((size_t)q * gridDim.x + blockIdx.x) * 2;
        o[0] = nan ? __builtin_nan("") : wmax;
        o[1] = nan ? __builtin_nan("") : amax;
    }
}
void launch_fold_asymmetry(hipStream_t s, int S, int nblk, int D, int Wld, size_t per, const double* W, double* out) {
    hipLaunchKernelGGL(k_fold_asymmetry, dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, s, D, Wld, per, W, out);
}

void launch_gemm(hipStream_t s, const GemmArgs& a_, const AtmSets* at, int cus) {
    GemmArgs a = a_;
    const int tiles_slab = (a.n_slab + DENSE_SLAB_ROWS - 1) / DENSE_SLAB_ROWS;
    const int tiles = (a.n_main + 16 * GEMM_RT - 1) / (16 * GEMM_RT) + tiles_slab;
    if (tiles <= 0) return;
    const int nct = (a.D + GEMM_BN - 1) / GEMM_BN;
    // (+ 1 with a live list: the workgroup that writes it)
    dim3 grid((unsigned)((tiles + 7) / 8 * 8 * nct + (a.live_list ? 1 : 0)));
    if (!at && a.lr_rank >= 0) {                         // the slab tiles' workgroups, then the stream's (jn_gemm_dense)
        a.lr_run = lr_stream_run(a.n_main, cus);
        grid.x = (unsigned)((tiles_slab + 7) / 8 * 8 * nct + (a.n_main + a.lr_run - 1) / a.lr_run + (a.live_list ? 1 : 0));
    }
    if (at) hipLaunchKernelGGL(k_jn_gemm_atm, grid, dim3(256), (size_t)a.pad_lds, s, a, *at);
    else if (a.sym) hipLaunchKernelGGL(k_jn_gemm<true>, grid, dim3(256), (size_t)a.pad_lds, s, a);
    else hipLaunchKernelGGL(k_jn_gemm<false>, grid, dim3(256), (size_t)a.pad_lds, s, a);
}

// Flip-symmetric folding of a contraction matrix (gemm_tile, SYM): for k, m < N, with k' = D-1-k, m' = D-1-m,
//     S[k][m] = (W[k][m] + W[k'][m'] + W[k'][m] + W[k][m']) / 4,   A[k][m] = (W[k][m] + W[k'][m'] - W[k'][m] - W[k][m']) / 4
// (the symmetric part of W; what is dropped is W[k][m] - W[k'][m'], the rounding of the phase-matrix builders, which the
// host has checked to be negligible).  Stored [k][S: 0..Wld/2 | A: Wld/2..Wld], zero elsewhere.
__global__ void k_symfold(int nmat, int N, int D, int Dp, int Wld, const double* __restrict__ W, double* __restrict__ SA) {
    const size_t per = (size_t)Dp * Wld;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * nmat) return;
    const size_t mat = i / per, r = i % per;
    const int k = (int)(r / Wld), c = (int)(r % Wld), Nh = Wld >> 1;
    const int m = c < Nh ? c : c - Nh;
    double out = 0.0;
    if (k < N && m < N) {
        const double* w = W + mat * per;
        const double p = w[(size_t)k * Wld + m], pf = w[(size_t)(D - 1 - k) * Wld + (D - 1 - m)];
        const double q = w[(size_t)(D - 1 - k) * Wld + m], qf = w[(size_t)k * Wld + (D - 1 - m)];
        out = c < Nh ? 0.25 * ((p + pf) + (q + qf)) : 0.25 * ((p + pf) - (q + qf));
    }
    SA[i] = out;
}
void launch_symfold(hipStream_t s, int nmat, int N, int D, int Dp, int Wld, const double* W, double* SA) {
    const size_t n = (size_t)Dp * Wld * nmat;
    hipLaunchKernelGGL(k_symfold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nmat, N, D, Dp, Wld, W, SA);
}

}  // namespace sosrt
