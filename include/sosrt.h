/*
 * sosrt.h -- C ABI of libsosrt.so, the MI355X (gfx950) implementation of the
 * Successive-Orders-of-Scattering hot path of
 * Guillaume-SOULIER/SOS-Radiative-Transfer (reference snapshot 2025-09-05).
 *
 * The reference has no FFI layer: its boundary for this path is a set of plain
 * Python functions on caller-owned float64 NumPy arrays.  Each entry point
 * below names the reference interface it replaces (file:line, relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SOSRT_E_* code on error;
 *     sosrt_last_error() returns a message for the calling thread.
 *   - all floating-point data is IEEE double, row-major, index order
 *     [column][order][layer t][direction m], m fastest; directions
 *     are ordered mu = -1..0 (m = 0..N-1, downward) then 0..+1 (m = N..2N-1).
 *   - "host" entry points take host pointers and copy in/out; "_dev" entry
 *     points take device pointers (hipMalloc'd, resident) and only enqueue
 *     work on the handle's stream.
 *   - a handle is bound to one device and one stream and is not thread-safe;
 *     distinct handles may be used concurrently.
 *   - the caller owns every buffer passed in.
 */
#ifndef SOSRT_H
#define SOSRT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sosrt_handle sosrt_t;

#define SOSRT_OK              0
#define SOSRT_E_INVALID      -1   /* bad argument / shape (Python layer raises ValueError)   */
#define SOSRT_E_HIP          -2   /* HIP runtime error                                        */
#define SOSRT_E_STATE        -3   /* call order (grid / phase / columns not set)              */
#define SOSRT_E_NOMEM        -4

/* per-column status written by transport / solve */
#define SOSRT_COL_OK           0
#define SOSRT_COL_INDEXERROR   1  /* upward mu->0+ search ran off the grid: the reference raises IndexError (spec:404, I1_In:103) */
#define SOSRT_COL_MAXORDERS    2  /* not converged within max_orders                                                          */
#define SOSRT_COL_INTERNAL     3  /* the transport kernel gave up waiting on itself (never expected; the column's field is unusable) */

/* geometry of a column */
#define SOSRT_GEOM_THREE_ZONE  0  /* above / inside / below the aerosol slab: SOS_Aer_main_specular.py:104-458 */
#define SOSRT_GEOM_SINGLE_SLAB 1  /* one homogeneous slab, black surface:      SOS_Aer_I1_In.py:13-130           */

/* surface model for orders n >= 2 */
#define SOSRT_SURFACE_NONE       0  /* single slab (I1_In:86-98)                                       */
#define SOSRT_SURFACE_SPECULAR   1  /* spec:397/399                                                    */
#define SOSRT_SURFACE_LAMBERTIAN 2  /* lam:399/401, coded sign (SURVEY hazard H2): the reflected radiance comes
                                       out negative, because the code integrates over a descending mu array      */
#define SOSRT_SURFACE_LAMBERTIAN_README 3  /* the same term with the sign of README.md:215 (positive); not what the
                                              reference's file computes -- non-default, parity unpinned            */

const char* sosrt_last_error(void);
/* 100 * major + minor of the ABI this library was built from.  101 (round 4): sosrt_set_stream(h, NULL) names the legacy default
 * stream (100 read NULL as "the handle's own stream"); the per-handle launch plan (sosrt_plan_launch) and the order loop that
 * runs several orders per launch (sosrt_set_order_loop) were added (sosrt_plan_launch may answer SOSRT_PLAN_GEMM_LIVE16_REGS since the
 * second half of that round).  102: the azimuth-resolved solve -- Fourier modes of the phase functions
 * (sosrt_phase_modes, sosrt_phase_p0_modes[_dev]), fixed order counts per column (sosrt_set_order_targets) and the
 * synthesis in azimuth (sosrt_azimuth_accumulate_dev); nothing that existed before changes.  103: the low-rank form of the
 * plain rows (sosrt_phase_rank, SOSRT_CONTRACT_F64_DENSE); results move within SOSRT_LOWRANK_TOL.  104: Mie tables built on the
 * device (sosrt_mie_ensembles[_dev], sosrt_mie_efficiencies, sosrt_mie_timing, sosrt_phase_table_dev); nothing that existed
 * before changes.  105: several aerosol phase matrices on one handle, chosen per column or per aerosol zone
 * (sosrt_set_phase_sets[_dev], sosrt_phase_matrix_dev, sosrt_set_aerosol_sets, sosrt_phase_sets_info; sosrt_plan_fold answers
 * for every set); nothing that
 * existed before changes.  A binding checks sosrt_version() >= the SOSRT_VERSION it was written against. */
#define SOSRT_VERSION 105
int sosrt_version(void);

/* ---- handle ------------------------------------------------------------------------------- */
/* L = nb_layers, N = nb_angles per hemisphere (spec:33,57).  Buffers are sized for max_batch
 * columns; max_orders bounds the order loop of spec:309.  device < 0 makes a host-only handle
 * (plan queries only, no GPU is touched).  4 <= N <= 1024; 2 <= L, and three values per layer of a column must fit the
 * 64 KiB of LDS the first-order kernel asks for (L <= 2686 at N = 128; the reference ships L = 800): SOSRT_E_INVALID
 * otherwise, with the largest L in sosrt_last_error(). */
int sosrt_create(int device, int L, int N, int max_batch, int max_orders, sosrt_t** out);
int sosrt_destroy(sosrt_t* h);
/* Streams.  A new handle enqueues on a stream of its own, created as a BLOCKING stream (hipStreamDefault): it orders against
 * the legacy default stream, so a caller that fills its buffers on the default stream (handle NULL -- torch's default stream
 * is that one) and then calls a `_dev` entry point gets the order it wrote, without an explicit synchronise.
 * sosrt_set_stream runs the handle on the caller's hipStream_t instead; NULL names the legacy default stream itself, as it
 * does everywhere in HIP (round 2 read NULL as "the handle's own stream", and that stream was non-blocking: a torch caller
 * passing torch.cuda.current_stream().cuda_stream == 0 got work that raced its own fills -- gpurun_out/split_full.txt).
 * sosrt_use_own_stream goes back to the handle's stream. */
int sosrt_set_stream(sosrt_t* h, void* hip_stream);
int sosrt_use_own_stream(sosrt_t* h);
int sosrt_synchronize(sosrt_t* h);
/* I_saved_out of the solves that follow holds `slots` orders per column ([B][slots][L][2N], 1 <= slots <=
 * max_orders; orders beyond are computed but not stored).  Default: max_orders.  The reference's list
 * I_saved (spec:304-305,458) has exactly n entries: solve once without it to learn n, then once with slots = max n. */
int sosrt_set_saved_orders(sosrt_t* h, int slots);
/* The solves that follow run at most `max_orders` orders (1 <= max_orders <= the max_orders of sosrt_create, which is the default):
 * a column still iterating then has status SOSRT_COL_MAXORDERS.  (The reference's loop, spec:309, has no bound.)  Lets one handle
 * serve callers with different budgets -- the Python layer's handle cache does. */
int sosrt_set_order_budget(sosrt_t* h, int max_orders);

/* ---- per-sweep setup ------------------------------------------------------------------------ */
/* direction grid mu[2N] (spec:59-61).  Builds the trapezoid weights of np.trapz(.., mu) used by
 * Jn (I1_In:73), the small-mu lane list (gva:5-7) and the extrapolation tables that replace
 * improved_limit_mu_down (In_limit:113-141). */
int sosrt_set_grid(sosrt_t* h, const double* mu);
/* phase matrices P(mu, mu') [2N x 2N] (outputs of phase_func, phase:12); P_aer may be NULL for the
 * single-slab geometry.  Folded on the host into W[k][m] = w_k P[m][2N-1-k] (I1_In:73, spec:321). */
int sosrt_set_phase(sosrt_t* h, const double* P_atm, const double* P_aer);

/* ---- several aerosol phase matrices in one batch ----------------------------------------------------------------------
 * sosrt_set_phase_sets: as sosrt_set_phase with S aerosol matrices P_aer [S][2N][2N] (host), 1 <= S <= SOSRT_MAX_PHASE_SETS.
 * S = 1 is sosrt_set_phase, bit for bit.  The symmetric form of the contraction is taken only if W_atm and EVERY set pass
 * SOSRT_SYMMETRY_TOL (sosrt_phase_asymmetry reports the maximum over them); the low-rank factor is of W_atm alone.
 * sosrt_plan_fold(h, 1 + s, ..) returns the fold of set s.
 *
 * sosrt_set_aerosol_sets: which set the aerosol of a column reads.  Called after sosrt_set_columns with nzmax = 1
 * (zone_set [B]: one set per column) or after sosrt_set_columns_zones with its nzmax (zone_set [B][nzmax]: one set per
 * aerosol zone; entries of clear zones are ignored).  Every sosrt_set_columns* call puts all columns back on set 0, so a
 * caller that never calls this sees no change.  A set outside 0..S-1, or a later sosrt_set_phase* with fewer sets than the
 * current columns use: SOSRT_E_INVALID with a message, nothing changed.
 *
 * How it is computed.  The slab rows of the contraction are multiplied by combined matrices ca W_atm + cr W_aer, one per
 * distinct coefficient pair of the batch ("group"); with sets a group is a distinct (set, ca, cr), and a batch with several
 * aerosols runs the same single pass over its slab rows, at the same flop count, with the bits each column has in a batch
 * of its own set alone.  While every column is on set 0 the cache holds 32 groups and a batch with more takes two passes
 * (W_atm, then W_aer), as before.  With another set in use the cache may hold up to 128 groups within 256 MiB of combined
 * matrices (never fewer than 32: 128 groups up to N = 256, 32 at N = 501); a batch with more groups takes the two passes
 * too: its slab rows are then listed set by set, and the second pass of a tile (dense tiling) or of a column (live-column
 * tilings) reads the W_aer of its set.  Two passes sum a slab row in another order than the single pass (same 1e-10 parity,
 * not the same bits).  The float contraction has no two-pass form (SOSRT_E_INVALID beyond the cache, as before).
 *
 * P0_aer of sosrt_first_order / sosrt_solve[_dev] stays [B][2N] when sets are per column (nzmax = 1): the caller passes
 * each column the P0 of its own set, as it always did.  After sosrt_set_aerosol_sets with nzmax > 1, P0_aer is
 * [B][nzmax][2N] and aerosol zone z of column b reads row (b, z) (the values in rows of clear zones are ignored), until the next
 * sosrt_set_columns* call.
 *
 * Not combined with sets: SOSRT_FIRST_ORDER_README (it reads the one W_aer element by element) -- sosrt_set_first_order and
 * sosrt_set_phase_sets with S > 1 refuse each other with SOSRT_E_INVALID.
 *
 * sosrt_phase_sets_info: out[4] = { sets of the last sosrt_set_phase*, groups of the current columns (0: none, or two passes),
 * 1 if the slab rows of the current columns take the single pass, groups the cache would hold with sets in use }. */
#define SOSRT_MAX_PHASE_SETS 64
int sosrt_set_phase_sets(sosrt_t* h, const double* P_atm, int S, const double* P_aer /*[S][2N][2N]*/);
/* The same with the aerosol matrices in DEVICE memory (d_P_aer [S][2N][2N], e.g. written by sosrt_phase_matrix_dev): fold
 * and asymmetry measure run as kernels in the handle's stream order, so the matrices go from the azimuth builders to the
 * contraction without visiting the host; a few partial maxima come back to decide the symmetric form (the call waits for
 * them).  The folds have the bits of the host fold (sosrt_plan_fold fetches one when asked); for NaN-free matrices the
 * asymmetry is the host loop's number, and any NaN switches the symmetric form off.  P_atm stays a host pointer: its low-rank
 * factorisation is host code.  S = 1 is allowed.  d_P_aer may be freed once the call returns. */
int sosrt_set_phase_sets_dev(sosrt_t* h, const double* P_atm /*host*/, int S, const double* d_P_aer /*device*/);
int sosrt_set_aerosol_sets(sosrt_t* h, int B, int nzmax, const int* zone_set /*[B][nzmax]*/);
int sosrt_phase_sets_info(sosrt_t* h, int* out /*[4]*/);

/* Several ATMOSPHERE phase matrices in one batch: what the Fourier modes of one scene need when they are
 * solved as the columns (m, b) of one batch -- mode m reads (-1)^m P_atm^m.  Detected by symbol; SOSRT_VERSION is unchanged.
 * sosrt_set_atm_phase_sets: S_atm matrices P_atm_sets [S_atm][2N][2N] (host), 1 <= S_atm <= SOSRT_MAX_PHASE_SETS, called AFTER
 * sosrt_set_phase* (which defines the aerosol matrices and atmosphere set 0, and puts S_atm back to 1).  Set 0 of the stack
 * replaces the handle's W_atm, exactly as sosrt_set_phase would have stored that matrix.  Every set is folded and must pass
 * the two certificates of sosrt_set_phase's W_atm: a low-rank factorisation of rank <= 4 within SOSRT_LOWRANK_TOL
 * (sosrt_phase_rank; iso 1, Rayleigh's modes 2, 1, 1, 0, ...; a zero matrix has rank 0) and flip symmetry within
 * SOSRT_SYMMETRY_TOL.  A set that fails either, or holds a NaN or an infinity, gives SOSRT_E_INVALID and the handle is left
 * as it was.  The choice of the symmetric contraction made by sosrt_set_phase* stands.
 * sosrt_set_atmosphere_sets: col_set [B], the atmosphere set of every current column (one per column, not per zone).  Every
 * sosrt_set_columns* call puts all columns back on set 0, so a caller that never calls this sees no change.  The plain rows
 * of a column take the low-rank factors of its set, its slab rows the combined matrix ca W_atm[set] + cr W_aer[aerosol set]:
 * a combined-matrix group is a distinct (atmosphere set, aerosol set, ca, cr), within the cache of sosrt_phase_sets_info.
 * A column on set s has the bits of the same column on a handle whose sosrt_set_phase got that set's matrix.
 * Refused with SOSRT_E_INVALID (and nothing changes) while S_atm > 1 or a column is off atmosphere set 0:
 *   - a batch with more groups than the cache holds (its two-pass form reads the one W_atm);
 *   - SOSRT_CONTRACT_F64_DENSE, _FULL and _F32, in either order of the calls (their plain rows are MFMA tiles over row lists
 *     that straddle columns), and matrices sosrt_set_phase* found not flip-symmetric;
 *   - SOSRT_FIRST_ORDER_README, in either order;
 *   - sosrt_set_phase* while a column is off set 0 (reset the columns first).
 * The order-loop launch is not planned while a column is off set 0.
 * sosrt_atm_sets_info: out[2] = { S_atm, 1 if any current column is off atmosphere set 0 }. */
int sosrt_set_atm_phase_sets(sosrt_t* h, int S_atm, const double* P_atm_sets /*host [S_atm][2N][2N]*/);
int sosrt_set_atmosphere_sets(sosrt_t* h, int B, const int* col_set /*[B]*/);
int sosrt_atm_sets_info(sosrt_t* h, int* out /*[2]*/);

/* First order of the solve.  CODED (default): spec:104-292 -- what both mains of the reference compute, with the specularly
 * reflected beam (SOS_Aer_main_lambertian.py's first-order blocks are the same formulas; its lines 274-276 crash).
 * README: the Lambertian first order of the reference's README.md:126-171 -- direct beam + the beam reflected isotropically by
 * the ground (int_0^1 mu'/(mu'-mu) ... dmu' by the trapezoid rule on the upward directions, the removable singularity at
 * mu' = mu taken analytically) + isotropic reflection of the downward first order.  PARITY UNPINNED: no runnable reference
 * code exists for it.  Meant for SOSRT_SURFACE_LAMBERTIAN_README; three-zone geometry only. */
#define SOSRT_FIRST_ORDER_CODED 0
#define SOSRT_FIRST_ORDER_README 1
int sosrt_set_first_order(sosrt_t* h, int mode);

/* arithmetic of the source-function contraction (BASELINE configs[4]: "fp64 -> fp32 mixed with tolerance study").
 * SOSRT_CONTRACT_F64 (default): v_mfma_f64_16x16x4_f64 -- the only mode that meets the 1e-10 parity bar.
 * SOSRT_CONTRACT_F32: operands rounded to float, v_mfma_f32_16x16x4_f32 with a float accumulator; transport, running
 * total and convergence test stay fp64.  About 3e-7 of the field maximum away from the fp64 result (measured on the
 * device: profiles/r02_mixed_precision_gpu.txt) -- an opt-in for callers with that tolerance, never the default.
 * Needs at most 32 distinct slab coefficient pairs in the batch.
 *
 * Within SOSRT_CONTRACT_F64 the library uses the flip symmetry of the folded matrices when they have it: every phase
 * function of the scattering angle on a grid with mu[2N-1-k] = -mu[k] gives W[2N-1-k][2N-1-m] = W[k][m], and then
 *   Jn[m] +- Jn[2N-1-m] = sum_{k<N} (In_1[k] +- In_1[2N-1-k]) (W[k][m] +- W[2N-1-k][m])
 * -- two N x N products instead of one 2N x 2N, half the flops, same v_mfma_f64 arithmetic.  sosrt_set_phase measures
 * max |W[k][m] - W[2N-1-k][2N-1-m]| / max |W| (sosrt_phase_asymmetry); at or below SOSRT_SYMMETRY_TOL (the rounding of
 * the phase-matrix builders: 1e-14 for the reference's) the symmetric form is used on the symmetric part of W, so Jn moves
 * by at most that fraction of max |W| sum |In_1| -- four orders of magnitude inside the 1e-10 parity bar; above it (any
 * matrix without the symmetry) the full product runs.  SOSRT_CONTRACT_F64_FULL forces the full product.
 *
 * Within SOSRT_CONTRACT_F64 the plain rows (every row outside a column's aerosol slab: Jn = ca In_1 W_atm) also use a low rank of
 * W_atm when it has one: sosrt_set_phase factors W_atm = U V (U: 2N x r, V: r x 2N, r <= 4) by cross approximation and accepts r
 * when max |W_atm - U V| <= SOSRT_LOWRANK_TOL max |W_atm| -- the Rayleigh matrix has r = 2 (the azimuth average of 3/4 (1 +
 * cos^2) is 3/8 (3 - mu^2 - mu'^2 + 3 mu^2 mu'^2)), iso r = 1, a zero matrix r = 0.  A plain row is then r dot products and an
 * r-term expansion, Jn = ca (In_1 U) V, and moves by at most SOSRT_LOWRANK_TOL max |W_atm| sum |In_1| (the argument of the
 * symmetric form).  The slab rows keep the MFMA product.  SOSRT_CONTRACT_F64_DENSE is SOSRT_CONTRACT_F64 without the low-rank
 * form (the MFMA product, symmetric when the matrices allow it, on every row: for A/B runs and tests).  SOSRT_CONTRACT_F32 is
 * always the dense product. */
#define SOSRT_CONTRACT_F64 0
#define SOSRT_CONTRACT_F32 1
#define SOSRT_CONTRACT_F64_FULL 2
#define SOSRT_CONTRACT_F64_DENSE 3
#define SOSRT_SYMMETRY_TOL 1e-12
#define SOSRT_LOWRANK_TOL 1e-12
int sosrt_set_contraction(sosrt_t* h, int mode);

/* The order loop of spec:309-458 runs an order as two launches (source function, transport) and the host learns the live count
 * between them.  Once few columns of a batch (or column group) are left -- their transport workgroups at most half the CUs --
 * the REMAINING orders run in ONE launch whose workgroups keep their roles (csrc/order_loop.hip): the chunk-parallel transport
 * of each live column and, on all other workgroups, the tiles of the live columns' source functions, tied by per-column
 * counters in device memory; the host only waits for the launch's report.  Same arithmetic, same bits.  mode 0 (default): never --
 * measured on MI355X the launch is bit-identical but SLOWER than the two launches per order it replaces (the dependency chain
 * sweep -> source-function tile -> sweep is the same; DESIGN section 5 item 9, profiles/r04_order_loop_ab_v0.txt); mode 1: where
 * the launch plan says so (sosrt_plan_launch), kept for the measurements and as the scaffold of a finer-grained pipeline; mode 2
 * (tests): as 1 with a grid of twice the device's CUs, which can never be resident -- every launch is refused and handed back.
 * A launch is only ever planned for columns of up to three zones with an even direction count N <= 256 (N <= 128 under a
 * Lambertian surface) and at most 64 chunks of 8 layers per sweep, L <= 512; every other shape keeps its two launches per order.
 * The launch checks its own residency first and hands the orders back
 * to the two-launch loop when another process's kernels keep its grid from being resident (sosrt_order_loop_stats: launches of
 * the last solve, how many of them were refused that way, and the (column, order) pairs that ran inside them). */
int sosrt_set_order_loop(sosrt_t* h, int mode);
int sosrt_order_loop_stats(sosrt_t* h, int* launches, int* refused, long long* column_orders /* nullable: (column, order) pairs run inside them; synchronises */);
/* asymmetry of the folded matrices of the last sosrt_set_phase (see above); *uses_symmetry: what the next solve will do */
int sosrt_phase_asymmetry(sosrt_t* h, double* asymmetry, int* uses_symmetry);
/* low rank of the folded W_atm of the last sosrt_set_phase (see above): *rank = r, or -1 when no r <= 4 meets the bar (a NaN, or a
 * matrix that is not low-rank); *residual = max |W_atm - U V| / max |W_atm| of the factors (or of the last step tried); *uses:
 * whether the next solve computes its plain rows in the low-rank form */
int sosrt_phase_rank(sosrt_t* h, int* rank, double* residual, int* uses);

/* per-column scalars (the locals of spec:23-53).  Arrays have B entries.
 *   THREE_ZONE : idx_up, idx_down (spec:40), mu0, grd_alb, alb_atm, alb_aer, dtau_atm, dtau_aer
 *                (spec:50-53), tauStar_tot (spec:36).
 *   SINGLE_SLAB: idx_* ignored (may be NULL); alb_atm = alb, tauStar_tot = tauStar of
 *                I1_NumInt / In_NumInt (I1_In:13,77); grd_alb, alb_aer, dtau_* ignored (may be NULL). */
int sosrt_set_columns(sosrt_t* h, int B, int geometry, int surface,
                      const int* idx_up, const int* idx_down,
                      const double* mu0, const double* grd_alb,
                      const double* alb_atm, const double* alb_aer,
                      const double* dtau_atm, const double* dtau_aer,
                      const double* tauStar_tot);

/* The same with a caller's ZONE TABLE instead of one slab: zones top to bottom, zone z of column b starts at
 * row zone_r0[b][z] (zone_r0[b][0] = 0, ascending) and ends before the next one; zone_mix[b][z] = 1 marks an aerosol zone
 * with single-scattering albedo zone_alb_aer[b][z] and optical-depth step zone_dtau_aer[b][z] (the dtau_aer of spec:52,
 * i.e. the slab's aerosol optical depth / its number of rows), 0 a clear zone (its two aerosol entries are ignored).
 * Aerosol zones are separated and bounded by clear ones; at most SOSRT_MAX_ZONES zones (four slabs).  Arrays are
 * [B][nzmax] row-major; nz[b] <= nzmax zones are read for column b.  Every formula of the path is evaluated per zone
 * exactly as the reference writes it for its three (spec:113-449); the extrapolation bucket (spec:342,361,380) of a clear
 * zone below a slab follows that slab's last row.  (clear, slab, clear) columns give bit-for-bit the results of
 * sosrt_set_columns.  The optical-depth grid tau of the solve must be consistent with the table (taup:21-27 per slab). */
#define SOSRT_MAX_ZONES 8
int sosrt_set_columns_zones(sosrt_t* h, int B, int surface, int nzmax, const int* nz, const int* zone_r0, const int* zone_mix,
                            const double* mu0, const double* grd_alb, const double* alb_atm, const double* dtau_atm,
                            const double* zone_alb_aer, const double* zone_dtau_aer, const double* tauStar_tot);

/* ---- step level (host pointers): parity surface of SOS_Aer_I1_In.py ------------------------- */
/* I1_NumInt (I1_In:13) / three-zone first order (spec:104-292).
 * tau [B][L], P0_atm / P0_aer [B][2N] (P0_aer may be NULL for SINGLE_SLAB), I1 out [B][L][2N].
 * P0_aer is [B][nzmax][2N] after sosrt_set_aerosol_sets with nzmax > 1 (one row per zone of the caller's table). */
int sosrt_first_order(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer,
                      double* I1_out);
/* Jn_NumInt (I1_In:62) / spec:314-323.  In_1 [B][L][2N] -> Jn [B][L][2N] */
int sosrt_source(sosrt_t* h, int B, const double* In_1, double* Jn_out);
/* In_NumInt (I1_In:77) / spec:326-449 (+ lam:399/401).  Jn [B][L][2N] -> In [B][L][2N];
 * status_out [B] receives SOSRT_COL_* (may be NULL). */
int sosrt_transport(sosrt_t* h, int B, const double* tau, const double* Jn, double* In_out, int* status_out);

/* ---- column level: the order loop of spec:301-458 ------------------------------------------- */
/* Iterates I1 -> [Jn -> In] until max(In/I at TOA-up, In/I at surface-down) < tol (spec:309) per
 * column.  Outputs: I_out [B][L][2N]; I_saved_out [B][slots][L][2N] or NULL (spec:304-305,458; slots =
 * max_orders unless sosrt_set_saved_orders was called);
 * n_orders_out [B] (the final n of spec:307-310); status_out [B] or NULL; I1_in (nullable,
 * [B][L][2N]) replaces the computed first order (used to pin the Lambertian n>=2 path).
 * I_out may be NULL: the field then stays on the device for sosrt_epilogue.
 * P0_aer is [B][nzmax][2N] after sosrt_set_aerosol_sets with nzmax > 1 (see there); the same holds for sosrt_solve_dev. */
int sosrt_solve(sosrt_t* h, int B, const double* tau, const double* P0_atm, const double* P0_aer,
                double tol, const double* I1_in,
                double* I_out, double* I_saved_out, int* n_orders_out, int* status_out);
/* same with device pointers; asynchronous on the handle's stream except for the convergence
 * polls.  n_orders_out / status_out are device int arrays (nullable). */
int sosrt_solve_dev(sosrt_t* h, int B, const double* d_tau, const double* d_P0_atm, const double* d_P0_aer,
                    double tol, const double* d_I1_in,
                    double* d_I_out, double* d_I_saved_out, int* d_n_orders_out, int* d_status_out);
/* number of order iterations (max over the batch) and sum over columns of the last solve */
int sosrt_last_solve_stats(sosrt_t* h, int* max_orders_run, long long* sum_orders);

/* ---- fused epilogue (graphe:157-158, crit:377-382): fluxes from a radiance field ------------ */
/* flux_down/up [B][L]; beam_norm 0: F0/(4 pi) (crit:380), 1: F0 (graphe:157). host pointers. */
int sosrt_fluxes(sosrt_t* h, int B, const double* tau, const double* I, int beam_norm,
                 double* flux_down, double* flux_up);

/* ---- epilogue on a RESIDENT field: what the reference's callers consume (a few kB per column instead of the
 * 0.4-1.6 MB field).  flux_down / flux_up as sosrt_fluxes (graphe:157-158, crit:380-381); diffusivity
 * -trapz(I mu, mu) / trapz(I, mu) per level (graphe:10); heating_rate per level (graphe:74-91, F0/(4 pi) beam
 * terms, last level copied, the two levels at the slab boundaries overwritten as in 'erase_pics'; needs
 * z_profile[L], the altitude grid np.linspace(z0, 0, L) of spec:39); net_toa [B] = -flux_down[0] - flux_up[0]
 * with the F0/(4 pi) beam terms (crit:382).  The net flux of graphe:41 is flux_down + flux_up with beam_norm 1.
 * Every output is nullable and skipped when NULL.
 * _dev: all pointers are device pointers (d_z_profile [L]); enqueued on the handle's stream.
 * sosrt_epilogue: works on the field and the optical depths the last sosrt_solve left in the handle (sosrt_solve
 * accepts I_out == NULL for that), host z_profile and host outputs. */
int sosrt_epilogue_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, int beam_norm,
                       const double* d_z_profile, double* d_flux_down, double* d_flux_up, double* d_diffusivity,
                       double* d_heating_rate, double* d_net_toa);
int sosrt_epilogue(sosrt_t* h, int B, int beam_norm, const double* z_profile, double* flux_down, double* flux_up,
                   double* diffusivity, double* heating_rate, double* net_toa);

/* ---- inputs of the path built on the device: azimuth-averaged phase functions (phase:68-292) --------------- */
#define SOSRT_PHASE_ISO       0   /* phase:68  isotropic                                                      */
#define SOSRT_PHASE_RAYLEIGH  1   /* phase:79  rayleigh                                                       */
#define SOSRT_PHASE_HG        2   /* phase:141 henyey_greenstein, asymmetry g                                 */
#define SOSRT_PHASE_TABLE     3   /* phase:238 fwc: a tabulated p(cos Theta), linear interpolation phase:198  */
/* table of SOSRT_PHASE_TABLE (host arrays, tab_mu ascending; fwc:3,173 is the reference's table) */
int sosrt_phase_table(sosrt_t* h, const double* tab_mu, const double* tab_p, int ntab);
/* The same from device arrays, in stream order (no trip through the host): d_tab_mu NULL means the uniform abscissa
 * linspace(-1, 1, ntab), what sosrt_mie_ensembles tabulates on.  Ascending order of a caller's d_tab_mu is not checked. */
int sosrt_phase_table_dev(sosrt_t* h, const double* d_tab_mu, const double* d_tab_p, int ntab);

/* ---- Lorenz-Mie tables on the device ------------------------------------------------------------
 * The series of Bohren & Huffman (1983) ch. 4 with the term counts of the package's host module: x = 2 pi r / wl,
 * n_max = round(x + 4 x^(1/3) + 2) terms, logarithmic derivative D_n(mx) downward from max(n_max, |mx|) + 16.  m = m_re + i m_im
 * with m_im > 0 ABSORBING (time factor exp(-i w t)); a caller under the other convention conjugates first.
 *
 * sosrt_mie_ensembles: S log-normal ensembles, phase:398-489.  Radii linspace(r_min, r_max, nb_radius) (micrometres, as wl
 * and r_m), n(r) = exp(-(ln r - ln r_m)^2 / (2 ln^2 sig)) / r, each sphere's intensity (|S1|^2 + |S2|^2) / (2 pi x^2 Q_ext)
 * weighted by n(r) Q_sca(r), trapezoid over r: p_out [S][ntab] on mu = linspace(-1, 1, ntab), un-normalised (every consumer
 * normalises).  nb_radius = 1 is ONE SPHERE of radius r_min without weights (phase:299; r_m, sig, r_max are not read).
 * bulk_out [S][3] (may be NULL), same trapezoid: {single-scattering albedo int n r^2 Q_sca / int n r^2 Q_ext, asymmetry
 * parameter int n r^2 Q_sca g / int n r^2 Q_sca, mean extinction cross-section pi int n r^2 Q_ext / int n in the square of
 * the unit of r}; one sphere: {Q_sca / Q_ext, g, pi r^2 Q_ext}.  Sums run in a fixed order: the same call gives the same
 * bits, and a batch the bits of its single calls.
 * wl, m_re, m_im, r_m, sig [S] are HOST arrays in both forms (the workspaces are sized from them); _dev: d_p_out and
 * d_bulk_out are device pointers and the work is enqueued on the handle's stream.
 * Caps: x <= SOSRT_MIE_MAX_X and |m x| <= SOSRT_MIE_MAX_MX for every sphere, and a workspace (32 n_max bytes per sphere plus
 * 8 ntab bytes per four radii) of at most SOSRT_MIE_MAX_WORKSPACE bytes per call; beyond them, and for sig <= 1, ntab < 2,
 * nb_radius < 1: SOSRT_E_INVALID, a message, nothing written. */
#define SOSRT_MIE_MAX_X 20000.0
#define SOSRT_MIE_MAX_MX 200000.0
#define SOSRT_MIE_MAX_WORKSPACE (2ull << 30)
int sosrt_mie_ensembles(sosrt_t* h, int S, const double* wl, const double* m_re, const double* m_im, const double* r_m,
                        const double* sig, int nb_radius, double r_min, double r_max, int ntab, double* p_out, double* bulk_out);
int sosrt_mie_ensembles_dev(sosrt_t* h, int S, const double* wl, const double* m_re, const double* m_im, const double* r_m,
                            const double* sig, int nb_radius, double r_min, double r_max, int ntab, double* d_p_out,
                            double* d_bulk_out);
/* The coefficient kernel alone: out [K][4] = {Q_ext, Q_sca, Q_back, g} of K spheres (m_re, m_im, x [K]; host arrays) */
int sosrt_mie_efficiencies(sosrt_t* h, int K, const double* m_re, const double* m_im, const double* x, double* out);
/* milliseconds the three kernels of the last sosrt_mie_ensembles[_dev] took (coefficients, angles, integration; HIP events
 * around each; waits for them) */
int sosrt_mie_timing(sosrt_t* h, double* ms /*[3]*/);

/* P0(mu, mu0[b]) for B columns (phase:86-103): 25-point azimuth trapezoid, normalised to trapz(P0, mu) = 2.
 * _dev: d_mu0 [B] and d_P0_out [B][2N] are device pointers (a mu0 sweep builds its P0 where the solve reads it). */
int sosrt_phase_p0_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0, double* d_P0_out);
int sosrt_phase_p0(sosrt_t* h, int B, int kind, double g, const double* mu0, double* P0_out);
/* P(mu, mu') [2N][2N] row-major with the column normalisation trapz(P[:, n], mu) = 4 (phase:107-131); host output */
int sosrt_phase_matrix(sosrt_t* h, int kind, double g, double* P_out);
/* the same matrix left in device memory (d_P_out [2N][2N]), enqueued on the handle's stream: what sosrt_set_phase_sets_dev reads */
int sosrt_phase_matrix_dev(sosrt_t* h, int kind, double g, double* d_P_out);

/* ---- azimuth-resolved radiance: Fourier modes in azimuth ------------------------------------------
 * The builders above average over the azimuth.  With the reference's scattering cosine c(a, b, phi) = -(mu_a mu_b + s_a s_b
 * cos phi), s = sqrt(1 - mu^2), and phi_q = linspace(0, pi, nphi), mode m of a pair of directions is the trapezoid rule
 *     R^m(a, b) = trapz_q [p(c(a, b, phi_q)) + (-1)^m p(c(a, b, phi_q + pi))] cos(m phi_q)
 * and the modes are normalised by the m = 0 ring of the same nphi:
 *     P0^m[b][a] = R^m(a, mu0_b) / (4 pi) * 2 / Z0_b,  Z0_b = trapz_mu(R^0(., mu0_b) / (4 pi))
 *     P^m[a][n]  = R^m(a, n) / (2 pi) * 4 / Z_n,       Z_n  = trapz_mu(R^0(., n) / (2 pi)).
 * Mode m of the radiance obeys the order loop of the azimuth average with ((-1)^m P^m, P0^m) in place of (P, P0): the
 * contraction pairs P[a][flip b] with I[b] (the reference's fold), and with c above that pair is the physical scattering
 * cosine at phi + pi, whose mode m is (-1)^m times the one at phi; P0 has no fold.  Then
 *     I(t, mu, phi) = sum_{m=0}^{M} (2 - delta_m0) I^m(t, mu) cos(m phi).
 * Azimuth convention: phi is the ring's angle; phi = 0 with an upward mu = mu0 is exact back-scatter (toward the sun).
 * Mode 0 is always the output of sosrt_phase_matrix / sosrt_phase_p0 (the reference's 25-point ring), bit for bit;
 * modes m >= 1 use nphi points, 1 <= m <= min(SOSRT_MAX_MODES, nphi - 2) (higher modes alias on nphi points).
 * Isotropic scattering has no mode m >= 1, Rayleigh none above 2 (p is quadratic in cos phi): exact zeros.  Every mode keeps the flip symmetry P^m(-mu, -mu') = P^m(mu, mu'), so
 * sosrt_set_phase takes the symmetric contraction for them by itself. */
#define SOSRT_MAX_MODES 64
/* modes m_first .. m_first + m_count - 1 of P: P_out [m_count][2N][2N], host output */
int sosrt_phase_modes(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, double* P_out);
/* sosrt_phase_modes with the matrices LEFT ON THE DEVICE: d_P_out [m_count][2N][2N], enqueued on the handle's stream (which
 * is synchronised first when a mode m >= 1 is asked for).  sign_odd != 0: mode m is written as (-1)^m P^m, what the solve of
 * mode m takes -- negation is exact, so these are the bits of the host's -1.0 * P.  The output goes straight into
 * sosrt_set_phase_sets_dev. */
int sosrt_phase_modes_dev(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, double* d_P_out);
/* the same modes of P0 for B columns: P0_out [m_count][B][2N] (the [B][2N] block of one mode is what sosrt_solve_dev reads).
 * _dev: d_mu0 [B], d_P0_out device pointers, enqueued on the handle's stream (synchronises it first when a mode m >= 1 is asked
 * for: the weights of the modes go to the device). */
int sosrt_phase_p0_modes_dev(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* d_mu0,
                             double* d_P0_out);
int sosrt_phase_p0_modes(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi, const double* mu0,
                         double* P0_out);
/* Fixed order counts.  A mode m >= 1 has no usable In/I test (its I^m crosses zero and vanishes at mu = +-1, and whole modes
 * vanish).  While targets are set (d_targets: device int [B] of the solves that follow, the caller's buffer, read by every
 * solve until cleared; NULL = off, the default) column b runs exactly max(target[b], 1) orders: the ratio is written but not
 * tested, reaching the target is SOSRT_COL_OK, and only a target above the order budget gives SOSRT_COL_MAXORDERS.  The
 * order-loop launch (sosrt_set_order_loop) is not planned while targets are set.  The azimuth-resolved driver runs mode m
 * for the n[b] orders the mode-0 solve of the same column ran. */
int sosrt_set_order_targets(sosrt_t* h, const int* d_targets);
/* synthesis: out[b][lev][dir][j] (+)= (2 - delta_m0) * I^m[b][levels[lev]][dir] * cos(m * phi[j]); m == 0 writes out, m >= 1
 * adds to it.  d_Im [B][L][2N], d_levels [nlev] (0 <= level < L; a level outside gives NaN rows), d_phi [nphi_out] (radians),
 * d_out [B][nlev][2N][nphi_out]; device pointers, enqueued on the handle's stream. */
int sosrt_azimuth_accumulate_dev(sosrt_t* h, int B, int m, const double* d_Im, int nlev, const int* d_levels, int nphi_out,
                                 const double* d_phi, double* d_out);
/* the whole sum in ONE launch: d_I0 [B][L][2N] is mode 0, d_Im [M][B][L][2N] the modes 1..M (0 <= M <= SOSRT_MAX_MODES; may be
 * NULL for M = 0) -- the layout of a batch whose column index is (m, b).  The terms are added in ascending m, so d_out has the
 * bits of sosrt_azimuth_accumulate_dev called for m = 0, 1, .., M, and is written once instead of rewritten per mode. */
int sosrt_azimuth_synthesize_dev(sosrt_t* h, int B, int M, const double* d_I0, const double* d_Im, int nlev, const int* d_levels,
                                 int nphi_out, const double* d_phi, double* d_out);

/* ---- view radiance: the solved field's source integrated off the grid -----------------------------------
 * The solve returns radiance on its own direction grid.  A sensor looks at a view zenith angle that is not a node, and next to
 * mu = 0+ the grid's upward lanes are an interpolation (the blend of spec:402-409), not a transport.  This stage integrates the
 * source function of a resident field along the line of sight at the view cosine itself.  It runs after a solve, reads the
 * columns of the last sosrt_set_columns* (zone table, mu0, grd_alb, albedos, steps), is enqueued on the handle's stream, and
 * writes nothing but its outputs and scratch of its own: the handle and the field are as they were.  Detected by symbol;
 * SOSRT_VERSION is unchanged.
 *
 * View cosines mu_view[V] (host), each finite and in [0.01, 1], 1 <= V <= SOSRT_MAX_VIEWS.  Signed lanes s[j], j < 2V:
 * s[j] = -mu_view[j] (downward) for j < V, s[V + j] = +mu_view[j] (upward); every output is ordered by j.
 *
 * sosrt_phase_rows_dev: rows of the stored phase matrix at exit cosines mu_signed [V2] (host, each in [-1, 1], V2 <= 2
 * SOSRT_MAX_VIEWS) with the stored matrix's own normalisers, d_rows_out[j][n] = 4 ring(s_j, mu_n) / trapz_a ring(mu_a, mu_n)
 * (ring: the 25-node azimuth rule of sosrt_phase_matrix); at a node the row of sosrt_phase_matrix.  sosrt_phase_p0_rows_dev:
 * the same of P0, d_out[b][j] = 2 ring(s_j, mu0_b) / trapz_a ring(mu_a, mu0_b).  Isotropic: 2 and 1.
 *
 * sosrt_view_radiance_dev: d_scat_out[b][lev][j] is the transport of the source
 *     S[b][t][j] = ca(b,t) sum_k w_k rows_atm[j][2N-1-k] I_src[b][t][k] + cr(b,t) sum_k w_k rows_aer[j][2N-1-k] I_src[b][t][k]
 * ((ca, cr): the row coefficients of the contraction, spec:321,323) at the rows `levels` (host, each in [0, L)), with
 * E = exp(-dtau / mu), dtau the step to the row the sweep comes from:
 *   SOSRT_VIEW_QUAD_GRID    the grid's arithmetic per lane, without its mu -> 0 treatments: trapezoid rule,
 *                           D[t] = E D[t-1] + (dtau / 2)(S[t-1] E + S[t]) / mu continuous across zones, U[t] = E U[t+1] + (dtau / 2)
 *                           (S[t] + S[t+1] E) / mu inside a zone, and the last row of every zone but the bottom one attenuated
 *                           and not integrated.  With I_src = I - I_last of a solve it reproduces I - I1 at a node.
 *                           It inherits the trapezoid rule's overshoot where dtau / mu >~ 1.
 *   SOSRT_VIEW_QUAD_LINEAR  exact attenuation of a piecewise-linear source, U[t] = E U[t+1] + w0 S[t] + w1 S[t+1] with
 *                           a = (1 - E) / x, x = dtau / mu, w0 = 1 - a, w1 = a - E (a series below x = 0.25), no zone restarts
 *                           and no gaps: the quadrature for limb-ward views.
 * Surface: rho times the downward value of the mirror lane (specular), 0 (SOSRT_SURFACE_NONE).
 * d_first_out[b][lev][j]: the closed-form first order (spec:104-292; I1_In:13-58 for the single slab) at the lanes s_j, from
 * d_p0rows_atm / d_p0rows_aer [B][2V]; it does not depend on the quadrature.  Either output may be NULL; the inputs of a
 * NULL output are not read.  The radiance at the view lanes is d_first_out + d_scat_out with I_src the sum of all orders but
 * the last (I_src = I adds the next term of the series, below tol of I at the rows the stopping rule tests).
 * Refused with SOSRT_E_INVALID, nothing written: Lambertian surfaces; SOSRT_FIRST_ORDER_README with d_first_out; columns off
 * aerosol set 0 or atmosphere set 0; V outside 1..SOSRT_MAX_VIEWS; a mu_view that is not finite or outside [0.01, 1]; a level
 * outside [0, L); B above the current columns; an unknown quadrature; d_first_out without both p0rows.
 * sosrt_view_timing: milliseconds of the last call's source contraction, sweeps and first order (HIP events; waits for them). */
#define SOSRT_MAX_VIEWS 64
#define SOSRT_VIEW_QUAD_GRID   0
#define SOSRT_VIEW_QUAD_LINEAR 1
int sosrt_phase_rows_dev(sosrt_t* h, int kind, double g, int V2, const double* mu_signed /*host [V2]*/, double* d_rows_out /*[V2][2N]*/);
int sosrt_phase_p0_rows_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0 /*[B]*/, int V2,
                            const double* mu_signed /*host [V2]*/, double* d_out /*[B][V2]*/);
int sosrt_view_radiance_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                            const double* d_I_src /*[B][L][2N]*/, const double* d_rows_atm, const double* d_rows_aer /*[2V][2N]*/,
                            const double* d_p0rows_atm, const double* d_p0rows_aer /*[B][2V]; needed only with d_first_out*/,
                            int quadrature, int nlev, const int* levels /*host, rows in [0, L)*/,
                            double* d_scat_out /*[B][nlev][2V], nullable*/, double* d_first_out /*[B][nlev][2V], nullable*/);
int sosrt_view_timing(sosrt_t* h, double* ms /*[3]*/);

/* ---- azimuth-resolved view radiance: the view stage per Fourier mode ------------------------------------
 * A sensor looks at a view zenith AND a relative azimuth.  Mode m of the radiance obeys the order loop with ((-1)^m P^m, P0^m),
 * and the view stage is linear in its rows and in P0: mode m at a view cosine is sosrt_view_radiance_dev run on the resident
 * I^m with the rows of mode m, and the radiance at (s_j, phi) is the synthesis sum_m (2 - delta_m0) I^m(s_j) cos(m phi) over the
 * view lanes.  Conventions as above: signed lanes s = (-mu_view, +mu_view), V2 = 2V <= 2 SOSRT_MAX_VIEWS,
 * c(a, b, phi) = -(mu_a mu_b + s_a s_b cos phi), phi_q = linspace(0, pi, nphi); phi = 0 with an upward mu = mu0 is back-scatter.
 * The specular surface holds mode by mode, at the same phi.  Detected by symbol; SOSRT_VERSION is unchanged.
 *
 * sosrt_phase_rows_modes_dev: d_rows_out[m - m_first][j][n] = R^m(s_j, mu_n) / (2 pi) * 4 / Z_n with the nphi-node normaliser
 * Z_n of sosrt_phase_modes (the same reduction over the 2N grid exits), so at a node s_j = mu_a the row is row a of
 * sosrt_phase_modes_dev, bit for bit.  sign_odd != 0 writes (-1)^m rows^m: what the view source of mode m takes, because it
 * pairs rows[j][2N-1-k] with I[k], the fold of the grid.  sosrt_phase_p0_rows_modes_dev: d_out[m - m_first][b][j] =
 * R^m(s_j, mu0_b) / (4 pi) * 2 / Z0_b with the normaliser of sosrt_phase_p0_modes.  Modes 1 <= m_first, m_first + m_count - 1
 * <= min(SOSRT_MAX_MODES, nphi - 2); mode 0 stays sosrt_phase_rows_dev / sosrt_phase_p0_rows_dev.  Isotropic: exact zeros;
 * Rayleigh m >= 3: exact zeros.  Both synchronise the handle's stream first (the weights of the modes go to the device).
 *
 * sosrt_phase_p0_rows_azimuth_dev: d_out[i][b][j] = p(c(s_j, mu0_b, phi_i)) / Z0_b, Z0_b the 25-node normaliser of the stored
 * P0 (what sosrt_phase_p0_rows_dev divides by): the sum the modes of P0 converge to, without the truncation at M.  The
 * [B][V2] block of one azimuth is the d_p0rows_* of sosrt_view_radiance_dev (d_scat_out = NULL): the first order at that
 * azimuth; the mirror lane of the reflected-beam term is at the same phi, because c(-a, -b, phi) = c(a, b, phi).  Isotropic: 1.
 *
 * sosrt_view_azimuth_accumulate_dev: d_out[b][lev][j][i] (+)= (2 - delta_m0) d_val[b][lev][j] cos(m phi_i); m == 0 writes,
 * m >= 1 adds, the term of sosrt_azimuth_accumulate_dev, so calls in ascending m give the bits of that rule.
 *
 * Refused with SOSRT_E_INVALID, nothing written: V2 outside 1..2 SOSRT_MAX_VIEWS; a lane that is not finite or outside
 * [-1, 1]; a mode range outside the limits; nphi_out < 1; B above the current columns.  All enqueued on the handle's stream. */
int sosrt_phase_rows_modes_dev(sosrt_t* h, int kind, double g, int m_first, int m_count, int nphi, int sign_odd, int V2,
                               const double* mu_signed /*host [V2]*/, double* d_rows_out /*[m_count][V2][2N]*/);
int sosrt_phase_p0_rows_modes_dev(sosrt_t* h, int B, int kind, double g, int m_first, int m_count, int nphi,
                                  const double* d_mu0 /*[B]*/, int V2, const double* mu_signed /*host [V2]*/,
                                  double* d_out /*[m_count][B][V2]*/);
int sosrt_phase_p0_rows_azimuth_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0 /*[B]*/, int V2,
                                    const double* mu_signed /*host [V2]*/, int nphi_out, const double* d_phi /*[nphi_out]*/,
                                    double* d_out /*[nphi_out][B][V2]*/);
int sosrt_view_azimuth_accumulate_dev(sosrt_t* h, int B, int m, int nlev, int V2, const double* d_val /*[B][nlev][V2]*/,
                                      int nphi_out, const double* d_phi /*[nphi_out]*/, double* d_out /*[B][nlev][V2][nphi_out]*/);

/* ---- delta-M scaling of a forward-peaked phase function, with a TMS first order -----------------------
 * The builders sample a phase function at the 2N nodes of the grid through a 25-node azimuth ring; a function whose forward
 * peak is narrower than the grid (the cloud table fwc: p(1) / mean = 5e4) is not held by that quadrature.  Delta-M (Wiscombe
 * 1977) replaces it by the Legendre series truncated at order Lambda with the fraction f = chi_Lambda of the scattering moved
 * into the direct beam: the truncated table is smooth, the optical depth and albedo of the aerosol are scaled by the caller
 * (tau' = tau (1 - w f), w' = (1 - f) w / (1 - w f)), and the solve is an ordinary solve.  Detected by symbol; SOSRT_VERSION
 * is unchanged.
 *
 * sosrt_phase_moments[_dev]: chi[s][l] = int p~ P_l dx / int p~ dx, l = 0 .. lmax, of S tables tab_p [S][ntab] on one abscissa
 * tab_mu [ntab] (ascending; NULL: the uniform abscissa of sosrt_phase_table_dev), p~ the table's piecewise-linear interpolant
 * -- the function the builders read -- so chi[s][0] = 1; norm[s] (may be NULL) = 1/2 int p~ dx.  The rule is the definition:
 * 4-node Gauss-Legendre on every table interval, P_l by the upward recurrence P_{l+1} = a_l x P_l - b_l P_{l-1}, a_l =
 * (2l + 1) / (l + 1), b_l = l / (l + 1); exact to rounding for l <= 6.  Sums run in a fixed order that ntab and lmax set (no
 * floating-point atomics): the same call gives the same bits, and table s of a batch the bits of its single call.
 *
 * sosrt_phase_delta_m[_dev]: f[s] = chi[s][order] and tab_out[s][i] = sum_{l < order} (2l + 1) (chi[s][l] - f) / (1 - f)
 * P_l(x_i), l ascending, on the same abscissa: the table of the truncated function, normalised like the moments (its mean
 * over [-1, 1] is 1).  A slightly negative f (a converged series) is accepted.  f_out may be NULL.
 *
 * Caps: 2 <= ntab <= SOSRT_DELTAM_MAX_NTAB, 1 <= lmax <= SOSRT_DELTAM_MAX_LMAX, 1 <= order <= lmax, 1 <= S <= 65535; beyond
 * them, for |f| >= 1 - 1e-6 and for a moment that is not finite: SOSRT_E_INVALID, a message, nothing written.  The host forms
 * also refuse a tab_mu that is not strictly ascending.  _dev: every pointer is a device pointer and the work is enqueued on
 * the handle's stream; sosrt_phase_delta_m_dev copies the S (lmax + 1) moments to the host for its refusals and waits for them.
 *
 * sosrt_phase_p0_normaliser_dev: d_Z_out[b] = Z0_b, the 25-node normaliser sosrt_phase_p0_rows_azimuth_dev divides by, and
 * nothing else: point values of one function times Z0 / Z0' carry the normaliser of another -- the TMS first order takes the
 * exact table's values with the truncated table's normaliser.  (Isotropic: 1, the value the rule gives.) */
#define SOSRT_DELTAM_MAX_NTAB 65536
#define SOSRT_DELTAM_MAX_LMAX 128
int sosrt_phase_moments(sosrt_t* h, int S, const double* tab_mu /*[ntab] or NULL*/, const double* tab_p /*[S][ntab]*/, int ntab,
                        int lmax, double* chi_out /*[S][lmax + 1]*/, double* norm_out /*[S] or NULL*/);
int sosrt_phase_moments_dev(sosrt_t* h, int S, const double* d_tab_mu /*[ntab] or NULL*/, const double* d_tab_p /*[S][ntab]*/,
                            int ntab, int lmax, double* d_chi_out /*[S][lmax + 1]*/, double* d_norm_out /*[S] or NULL*/);
int sosrt_phase_delta_m(sosrt_t* h, int S, const double* chi /*[S][lmax + 1]*/, int lmax, int order,
                        const double* tab_mu /*[ntab] or NULL*/, int ntab, double* tab_out /*[S][ntab]*/, double* f_out /*[S] or NULL*/);
int sosrt_phase_delta_m_dev(sosrt_t* h, int S, const double* d_chi /*[S][lmax + 1]*/, int lmax, int order,
                            const double* d_tab_mu /*[ntab] or NULL*/, int ntab, double* d_tab_out /*[S][ntab]*/,
                            double* d_f_out /*[S] or NULL*/);
int sosrt_phase_p0_normaliser_dev(sosrt_t* h, int B, int kind, double g, const double* d_mu0 /*[B]*/, double* d_Z_out /*[B]*/);

/* ---- pseudo-spherical direct beam: the slant path of the beam, first order and flux terms on it ---------
 * Every solve attenuates the direct solar beam as exp(-tau / mu0), the plane-parallel secant law; at low sun that is the largest
 * physical error of the path (at mu0 = 0.21 the converged field of the EVA column moves by 6.7 % of its maximum).  In the
 * pseudo-spherical approximation the beam is attenuated along its slant path through spherical shells and everything scattered is
 * transported plane-parallel as before: the first order changes, the order loop does not -- the solve is
 * sosrt_solve_dev(.., d_I1_in = d_I1, ..) with the first order of this stage.  Detected by symbol; SOSRT_VERSION is unchanged.
 * All three are enqueued on the handle's stream, read the columns of the last sosrt_set_columns / sosrt_set_columns_zones
 * (mu0, grd_alb, albedos, steps, tauStar_tot, zone table) and write nothing but their outputs: the handle's columns, resident
 * field, order targets and phase state are as they were.  1 <= B <= the current columns (the first B of them).
 *
 * sosrt_beam_slant_dev: levels t = 0..L-1 at altitudes d_z [L] (km, finite, strictly descending, shared by the batch -- the
 * np.linspace(z0, 0, L) of spec:39), r_t = earth_radius_km + z_t, p^2 = r_t^2 (1 - mu0^2):
 *     sigma_0 = 0,  sigma_t = sum_{k=1..t} (tau_k - tau_{k-1}) c_{t,k},
 *     c_{t,k} = (r_{k-1} + r_k) / (sqrt(r_{k-1}^2 - p^2) + sqrt(r_k^2 - p^2))
 * (the path through shell k over its thickness; 1 at mu0 = 1, -> 1 / mu0 as the radius grows, so sigma -> tau / mu0).
 * d_mu0 [B] or NULL for the columns' own mu0; a caller's must be finite and in (0, 1].  d_sigma_out [B][L].  An O(L^2) sum per
 * column.  The call reads d_z (and a caller's d_mu0) back to check them: it waits for the stream's earlier work.
 *
 * sosrt_first_order_beam_dev: the first order layer by layer on a beam path d_sigma [B][L] THAT IS AN INPUT (sigma = tau / mu0
 * gives the coded first order, SOSRT_FIRST_ORDER_CODED, to rounding: how the kernel is pinned).  With F0 = pi / mu0, T =
 * tauStar_tot, R = F0 rho exp(-sigma_{L-1} - (T - tau_{L-1}) / mu0), q[m] of spec:149 per zone, a = |mu_m|, Delta the optical
 * thickness of a layer, E = exp(-Delta / a), s = (slant thickness of the layer) / Delta, phi(y) = (1 - exp(-y)) / y:
 *     downward  D_0 = 0,  D_t = D_{t-1} E + q_t F0 exp(-sigma_t) (Delta / a) phi((1 / a - s) Delta)
 *                               + [t is not the first row of a zone below the top one] q_t[mirror] R exp(-(T - tau_t) / mu0) (Delta / a) phi((1 / a + 1 / mu0) Delta)
 *     surface   U_{L-1} = rho D_{L-1}[mirror]
 *     upward    U_t = U_{t+1} E + q_t F0 exp(-sigma_t) (Delta / a) phi((1 / a + s) Delta)
 *                               + [t is not the last row of a zone above the bottom one] q_t[mirror] R exp(-(T - tau_t) / mu0) (Delta / a) phi((1 / a - 1 / mu0) Delta)
 *     mu = 0    q_t F0 exp(-sigma_t) + q_t[mirror] R exp(-(T - tau_t) / mu0)
 * (layer (t-1, t) of the downward sweep takes the q of row t, layer (t, t+1) of the upward sweep the q of row t; the two
 * exclusions are the reference's own level choices; the reflected beam travels upward plane-parallel at mu0).  phi is
 * exact at y = 0, so the |mu -+ mu0| < 1e-4 limit branches of spec:111,204 have no counterpart: on such a lane the result is up to
 * 1e-4 of the maximum away from the coded first order.  d_P0_atm [B][2N]; d_P0_aer [B][2N], or [B][nzmax][2N] after
 * sosrt_set_aerosol_sets with nzmax > 1; d_I1_out [B][L][2N].  A layer is assumed thinner than 700 mu0 (exp(Delta / mu0) finite).
 *
 * sosrt_epilogue_beam_dev: sosrt_epilogue_dev with the beam terms of the fluxes on the path d_sigma [B][L]: downward
 * -fb exp(-sigma_t), upward +fb rho exp(-sigma_{L-1}) exp(-(tau_{L-1} - tau_t) / mu0) (fb: F0 / (4 pi) or F0 by beam_norm); with
 * sigma = tau / mu0 it is sosrt_epilogue_dev to rounding.  Outputs nullable as there.
 *
 * Refused with SOSRT_E_INVALID, a message and nothing written: the single-slab geometry; SOSRT_FIRST_ORDER_README; B outside
 * 1..the current columns; a null pointer (the nullable outputs of the epilogue aside); z not finite or not strictly descending;
 * earth_radius_km not finite or <= 0; L > 2048.  Open: refraction, a spherical path of the reflected beam or of the scattered
 * light, the README first order on a slant path. */
int sosrt_beam_slant_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_z /*[L]*/, double earth_radius_km,
                         const double* d_mu0 /*[B], nullable: the columns' own*/, double* d_sigma_out /*[B][L]*/);
int sosrt_first_order_beam_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_sigma /*[B][L]*/,
                               const double* d_P0_atm, const double* d_P0_aer, double* d_I1_out /*[B][L][2N]*/);
int sosrt_epilogue_beam_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, int beam_norm, const double* d_z_profile,
                            double* d_flux_down, double* d_flux_up, double* d_diffusivity, double* d_heating_rate,
                            double* d_net_toa, const double* d_sigma /*[B][L]*/);

/* ---- pseudo-spherical direct beam at view lanes -----------------------------------------------------------
 * sosrt_view_first_order_beam_dev: the first order of sosrt_first_order_beam_dev at view cosines off the direction grid -- its
 * recurrences with a = mu_view[v] in place of |mu_m|, on the signed lanes of sosrt_view_radiance_dev, (-mu_view, +mu_view): lane j
 * and its mirror j +- V.  q of a zone from the p0 rows at the lane, (w_atm p0_atm[j] f_atm + w_aer p0_aer[j] f_aer) / (4 pi); the
 * two level exclusions and the reflected beam R as there; U_{L-1} = rho D_{L-1}[mirror]; no mu = 0 lane (mu_view >= 0.01); phi is
 * exact at mu_view = mu0.  With sigma = tau / mu0 it is the d_first_out of sosrt_view_radiance_dev to rounding, but for lanes within
 * 1e-4 of mu0, where that one takes its limit form (up to 1e-4 of the maximum apart).  Detected by symbol; SOSRT_VERSION is unchanged.
 * nset sets of p0 rows (the azimuths of an exact first order, or 1) share one evaluation of the geometry: a lane's value is linear
 * in (p0_atm[j], p0_aer[j], p0_atm[mirror], p0_aer[mirror]) and the kernel carries the four coefficients.  d_p0rows_* [nset][B][2V];
 * d_first_out [nset][B][nlev][2V].  Enqueued on the handle's stream; reads the columns of the last sosrt_set_columns* and writes
 * nothing but its output.  Refused with SOSRT_E_INVALID, a message and nothing written: what sosrt_first_order_beam_dev refuses;
 * V, mu_view, nlev, levels outside the limits of sosrt_view_radiance_dev; a Lambertian surface; columns off aerosol set 0, a
 * per-zone P0 layout or atmosphere phase sets; nset < 1; a null pointer. */
int sosrt_view_first_order_beam_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                                    const double* d_sigma /*[B][L]*/, int nset, const double* d_p0rows_atm /*[nset][B][2V]*/,
                                    const double* d_p0rows_aer /*[nset][B][2V]*/, int nlev, const int* levels /*host*/,
                                    double* d_first_out /*[nset][B][nlev][2V]*/);

/* ---- thermal emission: Planck sources in the layers and at the ground ------------------------------------
 * Every other solve is driven by the solar beam.  This stage computes the radiation the layers and the ground EMIT, the field
 * I_0 of a thermal problem; the order loop scatters and transports it as it is -- the full field is
 * sosrt_solve_dev(.., d_I1_in = d_I0, ..), I = sum_{n>=0} I_n, and mu0 does not enter.  Detected by symbol; SOSRT_VERSION is
 * unchanged.  All three are enqueued on the handle's stream, read the columns of the last sosrt_set_columns /
 * sosrt_set_columns_zones (grd_alb, albedos, steps, zone table; the handle's surface) and write nothing but their outputs: the
 * handle's columns, resident field, order targets, phase state and first-order mode are as they were.  1 <= B <= the current
 * columns (the first B of them).
 *
 * d_planck [B][L]: the Planck radiance b_t at level t, in any unit (the field comes out in it); d_planck_surface [B]: the
 * ground's, b_s; d_emissivity [B]: the ground's emissivity e_s, NULL: 1 - grd_alb.  Emission coefficient of a row's zone:
 * eps = 1 - alb_atm in a clear zone, 1 - (alb_atm f_atm + alb_aer f_aer) in an aerosol zone (f of spec:149).  The layer between
 * rows t-1 and t takes the eps of row t in BOTH sweeps.  The source is linear in tau between two levels and attenuated exactly:
 * a = |mu|, x = Delta / a, E = exp(-x), A = (1 - E) / x, w0 = 1 - A (the row the sweep arrives at), w1 = A - E (the row it
 * leaves), both 0 at x = 0 and summed as a series below x = 0.25 -- the rule of SOSRT_VIEW_QUAD_LINEAR.
 *     downward  D_0 = 0,  D_t = D_{t-1} E + eps_t (w0 b_t + w1 b_{t-1})
 *     ground    U_{L-1} = boundary(D_{L-1}) + e_s b_s
 *     upward    U_t = U_{t+1} E + eps_{t+1} (w0 b_t + w1 b_{t+1})
 *     mu = 0    eps_t b_t
 * boundary: what the order loop applies for the handle's surface (specular: rho times the mirror lane; the two Lambertian
 * grounds: their scalar of the downward surface row; SOSRT_SURFACE_NONE: 0).
 *
 * sosrt_emission_view_dev: the same sweeps at a = mu_view[v], the requested levels only; out lanes as sosrt_view_radiance_dev
 * ([B][nlev][2V]: first the V downward lanes, then the V upward ones).  Specular and SOSRT_SURFACE_NONE only.
 * sosrt_epilogue_emission_dev: sosrt_epilogue_dev without the two beam terms.  Outputs nullable as there.
 *
 * Refused with SOSRT_E_INVALID, a message and nothing written: the single-slab geometry; B outside 1..the current columns; a
 * null pointer (d_emissivity and the nullable outputs of the epilogue aside); L > 2048; V, mu_view or levels outside
 * the limits of sosrt_view_radiance_dev; a Lambertian surface in the view call; the heating rate without z_profile.  No device
 * array is read back to be checked. */
int sosrt_emission_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_planck /*[B][L]*/,
                       const double* d_planck_surface /*[B]*/, const double* d_emissivity /*[B], NULL: 1 - grd_alb*/,
                       double* d_I0_out /*[B][L][2N]: the d_I1_in of sosrt_solve_dev*/);
int sosrt_emission_view_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V], each in [0.01, 1]*/,
                            const double* d_tau, const double* d_planck, const double* d_planck_surface,
                            const double* d_emissivity, int nlev, const int* levels /*host*/, double* d_out /*[B][nlev][2V]*/);
int sosrt_epilogue_emission_dev(sosrt_t* h, int B, const double* d_tau, const double* d_I, const double* d_z_profile,
                                double* d_flux_down, double* d_flux_up, double* d_diffusivity, double* d_heating_rate,
                                double* d_net_toa);   /* outputs nullable as in sosrt_epilogue_dev */

/* ---- gas absorption profiles: per-level weights on the source function ------------------------------------
 * A pure absorber added to a layer multiplies the source of that level by w_t = Delta tau_scattering / (Delta tau_scattering +
 * Delta tau_gas), for both constituents alike, while tau carries the gas.  The ABI takes two weights per row, one on each row
 * coefficient of the contraction: while set, the coefficients of every solve and of sosrt_source are (alb_atm f_atm / 4)
 * w_atm[b][t] and (alb_aer f_aer / 4) w_aer[b][t] -- any per-level albedo of the atmosphere and any per-level aerosol fraction
 * of a slab, relative to the zone's nominal values.  Detected by symbol; SOSRT_VERSION is unchanged.
 *
 * sosrt_set_row_weights_dev: copies the weights of the first B columns (device arrays [B][L]) into buffers of the handle, in
 * stream order; the other columns of the batch keep weight one.  One NULL stands for ones, both NULL clear the weights.  They
 * belong to the columns of the last sosrt_set_columns / sosrt_set_columns_zones: either call clears them.  While set, slab rows
 * run the two-pass form of the contraction (cleared: the grouping is restored), the order-loop launch stays off, and the entries
 * that evaluate one constant per zone -- sosrt_first_order, sosrt_solve[_dev] without a caller's first order,
 * sosrt_first_order_beam_dev, sosrt_view_first_order_beam_dev, sosrt_view_radiance_dev, sosrt_emission_dev,
 * sosrt_emission_view_dev -- return SOSRT_E_STATE with a message and write nothing, as do sosrt_set_aerosol_sets and
 * sosrt_set_atmosphere_sets (set the sets first, then the weights).  The BRDF ground's stages (sosrt_ground_*_dev,
 * sosrt_view_ground*_dev, sosrt_bounce_accumulate_dev) read no albedo and no fraction of the columns -- they reflect a surface row and
 * attenuate along tau -- and stay open.  With no weights set nothing changes: not a launch, not a bit.
 * At view lanes the weighted forms are entries of their own (below): sosrt_view_radiance_profile_dev,
 * sosrt_view_first_order_profile_dev and sosrt_emission_view_profile_dev.
 * The weights are not read back: finite and >= 0 is the caller's contract.  Refused with a message, nothing written: the
 * single-slab geometry, B outside 1..the current columns, no columns set, columns on atmosphere sets.
 *
 * sosrt_first_order_profile_dev: the recurrences of sosrt_first_order_beam_dev (level choices, the two exclusions, R, phi and the
 * mu = 0 lane as there; d_sigma = tau / mu0 is the plane beam, sosrt_beam_slant_dev on the total tau the sphere) with the handle's
 * weights in q, row by row:  q_t[m] = (alb_atm f_atm w_atm,t P0_atm[m] + alb_aer f_aer w_aer,t P0_aer[m]) / 4 pi.
 * sosrt_emission_profile_dev: sosrt_emission_dev with eps_t = 1 - (alb_atm f_atm w_atm,t + alb_aer f_aer w_aer,t) per row in
 * place of the zone's; the same sweeps, the same boundary.
 * Both refuse what their models refuse (L > 1024 here: two more rows of L doubles in LDS), and a handle with no weights set
 * (SOSRT_E_STATE). */
int sosrt_set_row_weights_dev(sosrt_t* h, int B, const double* d_w_atm /*[B][L] or NULL*/, const double* d_w_aer /*[B][L] or NULL*/);
int sosrt_first_order_profile_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_sigma /*[B][L]*/,
                                  const double* d_P0_atm /*[B][2N]*/, const double* d_P0_aer /*[B][2N] or [B][nzmax][2N]*/,
                                  double* d_I1_out /*[B][L][2N]: the d_I1_in of sosrt_solve_dev*/);
int sosrt_emission_profile_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_planck /*[B][L]*/,
                               const double* d_planck_surface /*[B]*/, const double* d_emissivity /*[B], NULL: 1 - grd_alb*/,
                               double* d_I0_out /*[B][L][2N]*/);

/* ---- gas absorption at view angles: per-level weights in the view stage ------------------------------------
 * The radiance at view cosines off the grid of a column whose rows carry the weights of sosrt_set_row_weights_dev.  Three entries
 * beside the guarded ones, which keep their guards; detected by symbol, SOSRT_VERSION is unchanged.  All three need weights to
 * be set (SOSRT_E_STATE with a message otherwise) and refuse, before the first launch and with nothing written, what their
 * unweighted models refuse -- the single slab, B outside 1..the current columns, V, mu_view or levels outside the view stage's
 * limits, a Lambertian surface, null pointers; the two that take phase rows also several aerosol phase sets or atmosphere sets
 * -- and L > 1024.  Enqueued on the handle's stream; nothing but the outputs and the view stage's own scratch is written.
 *
 * sosrt_view_radiance_profile_dev: the scattered term of sosrt_view_radiance_dev (the same code, the same kernels) with the
 * handle's weights on the stage's row coefficients: S_t = w_atm,t ca_t (rows_atm . I_src,t) + w_aer,t cr_t (rows_aer . I_src,t).
 * It has no first-order arguments: under weights the first term is one of the two entries below.  With I_src = I - I_last of a
 * weighted solve and SOSRT_VIEW_QUAD_GRID it gives, at a node's cosine, the grid's own I - I1.
 *
 * sosrt_view_first_order_profile_dev: the argument list, output layout and recurrences of sosrt_view_first_order_beam_dev (the two
 * exclusions, R, phi, the four coefficient chains; d_sigma = tau / mu0 is the plane beam, sosrt_beam_slant_dev on the total tau
 * the sphere) with A and Rz of a row:  A_t = alb_atm w_atm,t f_atm / 4 pi,  Rz_t = alb_aer w_aer,t f_aer / 4 pi.
 *
 * sosrt_emission_view_profile_dev: sosrt_emission_view_dev with eps_t = 1 - (alb_atm f_atm w_atm,t + alb_aer f_aer w_aer,t) per
 * row, the expression of sosrt_emission_profile_dev; specular surface or SOSRT_SURFACE_NONE.
 * With unit weights the three have the bits of their unweighted models. */
int sosrt_view_radiance_profile_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                                    const double* d_I_src /*[B][L][2N]*/, const double* d_rows_atm /*[2V][2N]*/,
                                    const double* d_rows_aer /*[2V][2N]*/, int quadrature, int nlev, const int* levels /*host*/,
                                    double* d_scat_out /*[B][nlev][2V]*/);
int sosrt_view_first_order_profile_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                                       const double* d_sigma /*[B][L]*/, int nset, const double* d_p0rows_atm /*[nset][B][2V]*/,
                                       const double* d_p0rows_aer /*[nset][B][2V]*/, int nlev, const int* levels /*host*/,
                                       double* d_first_out /*[nset][B][nlev][2V]*/);
int sosrt_emission_view_profile_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                                    const double* d_planck /*[B][L]*/, const double* d_planck_surface /*[B]*/,
                                    const double* d_emissivity /*[B], NULL: 1 - grd_alb*/, int nlev, const int* levels /*host*/,
                                    double* d_out /*[B][nlev][2V]*/);

/* ---- band integration: spectral points in one batch --------------------------------------------------------
 * A batch of K spectral points x C physical columns is solved as K C library columns laid out point-major, b = k C + c.  Two
 * stages beside the solve, detected by symbol (SOSRT_VERSION is unchanged).  Both are enqueued on the handle's stream; the Planck
 * stage reads the handle's L; nothing else of the handle's solve state is read or written (like every stage, a call ends the
 * run of adjacent launches that the handle's profiling slots keep track of), and no device array is read back.
 *
 * sosrt_planck_bands_dev: the Planck radiance of K bands [nu_lo, nu_hi] (wavenumbers, cm^-1) at the L levels and at the ground
 * of C columns, from temperatures in kelvin.  x = c2 nu / T, c2 = 100 h c / k (CODATA 2018);
 *     B = 2 k^4 T^4 / (h^3 c^2) [G(x_lo) - G(x_hi)]  W m^-2 sr^-1,   G(x) = int_x^inf t^3 / (e^t - 1) dt,
 * split at x = 1: below it G = pi^4 / 15 - S(x), S(x) = sum c_k x^{k+3}, c_k = B_k / ((k + 3) k!) over the ten non-zero
 * Bernoulli terms k = 0, 1, 2, 4, .., 16; at and above it G = sum_{n=1}^{30} e^{-n x} (x^3/n + 3 x^2/n^2 + 6 x/n^3 + 6/n^4).
 * The difference takes the form that does not cancel: S(x_hi) - S(x_lo) with both edges below 1, the two sums with both at or
 * above it, (pi^4/15 - S(x_lo)) - G(x_hi) otherwise.  nu_lo = 0 is allowed; pi B(0, inf) = sigma T^4.  A band of width dnu
 * loses digits by cancellation (up to 6e-13 relative at 1 cm^-1, 6e-11 at 0.01 cm^-1): a monochromatic source is the caller's.
 * T <= 0 is not refused (the temperatures are not read back): such an entry comes out NaN.  Under normalise = 1 a (k, c) with
 * no positive value -- every radiance underflows to 0, a band far in the Wien tail of a cold column (x above about 745), or every
 * temperature is <= 0 -- gets scale = 0 and NaN outputs (0 / 0): the caller tests the scale it reads back.
 * normalise = 1: per (k, c) scale = max(max_t b_t, b_s); the outputs are b / scale, their maximum exactly 1.0, and d_scale_out
 * receives scale -- the order loop's mu -> 0 search has an absolute threshold and wants a source of order 1.
 * normalise = 0: the outputs as computed, scale = 1; d_scale_out may then be NULL.
 * Refused with SOSRT_E_INVALID, a message and nothing written: C or K < 1; a null pointer (the scale under normalise = 0
 * aside); an edge that is not finite or is negative; nu_hi <= nu_lo; normalise other than 0 or 1.
 *
 * sosrt_band_reduce_dev: out[c][m] = acc_K, acc_0 = accumulate ? out[c][m] : 0, and for k = 0 .. K-1 in this order
 * acc_{k+1} = fma(w[k][c] s[k][c], x[k][c][m], acc_k) with the product w s rounded once; a NULL d_weight or d_scale stands for
 * ones.  The result depends neither on the launch geometry nor on how K is split over calls with accumulate = 1.  M is what
 * the caller sums: L for a flux or heating-rate profile, 1 for net_toa, nlev 2V for view radiances.
 * Refused: C, K or M < 1; null d_x or d_out. */
int sosrt_planck_bands_dev(sosrt_t* h, int C, int K, const double* d_T /*[C][L] kelvin at the levels*/,
                           const double* d_T_surface /*[C]*/, const double* nu_lo /*host [K], cm^-1*/,
                           const double* nu_hi /*host [K]*/, int normalise, double* d_planck_out /*[K][C][L]*/,
                           double* d_planck_surface_out /*[K][C]*/, double* d_scale_out /*[K][C]*/);
int sosrt_band_reduce_dev(sosrt_t* h, int C, int K, int M, const double* d_weight /*[K][C] or NULL: 1*/,
                          const double* d_scale /*[K][C] or NULL: 1*/, const double* d_x /*[K][C][M]*/,
                          double* d_out /*[C][M]*/, int accumulate);

/* ---- brightness temperature of a band-summed radiance ------------------------------------------------------
 * The inverse of the Planck stage.  T_out[c][m] is the temperature T at which
 *     f_c(T) = sum_k w[k][c] B_k(T)
 * equals radiance[c][m]; B_k is the band radiance of sosrt_planck_bands_dev over [nu_lo[k], nu_hi[k]] (the same S / G split, the
 * same constants, the same non-cancelling difference), w the weights of sosrt_band_reduce_dev without the scales (the scale is a
 * property of the normalised source, not of the channel); a NULL d_weight stands for ones.  g-points of one band: K equal pairs of
 * edges, weights that sum to 1.  Sub-bands of a response function: distinct edges, the response as weights.  f_c is strictly
 * increasing in T for weights >= 0 that are not all zero.
 * Iteration, per element: Newton on ln f in the variable u = 1 / T (close to linear in the Wien regime), from T = 250 K:
 *     u' = u + ln(f / R) f / (T^2 f'),  T' = 1 / u',
 *     f' = sum_k w_k dB_k/dT,  dB/dT = 4 B / T + (2 k^4 / h^3 c^2) T^3 [x_lo^4 / (e^x_lo - 1) - x_hi^4 / (e^x_hi - 1)]
 * (expm1; the first bracket term is 0 at x_lo = 0), safeguarded by a bracket [1 K, 1e5 K] that every evaluation tightens (f < R
 * raises the lower end to T, f > R lowers the upper end to T): an iterate that is not finite or falls outside the closed bracket
 * is replaced by the bracket's geometric mean.  The first accepted Newton step with |T' - T| <= 1e-9 T' is applied and ends the
 * iteration (quadratic convergence leaves the result at rounding); at most 40 iterations, and an element that has not stopped by
 * then is NaN.  NaN also where the radiance is not finite or <= 0, where it lies outside (f(1 K), f(1e5 K)), and where the
 * column's weights are all zero or one is negative.  Nothing is read back to be checked.  Within 1e-12 relative of the NumPy form
 * for bands of 10 cm^-1 and more (narrower bands lose digits as the Planck stage does).
 * One lane per element; the band edges travel by value, so K <= 64: the sum over the bands sits inside the iteration and cannot
 * be split over launches.  A stage beside the solve, detected by symbol (SOSRT_VERSION is unchanged), enqueued on the handle's
 * stream; nothing of the handle's solve state is read or written.
 * Refused with SOSRT_E_INVALID, a message and nothing written: C, K or M < 1; K > 64; a null nu_lo, nu_hi, d_radiance or d_T_out;
 * an edge that is not finite or is negative; nu_hi <= nu_lo. */
int sosrt_brightness_temperature_dev(sosrt_t* h, int C, int K, int M, const double* nu_lo /*host [K], cm^-1*/,
                                     const double* nu_hi /*host [K]*/, const double* d_weight /*[K][C] or NULL: 1*/,
                                     const double* d_radiance /*[C][M], W m^-2 sr^-1*/, double* d_T_out /*[C][M], kelvin*/);

/* ---- BRDF ground: a series in ground reflections around the order loop -------------------------------------
 * The field over a ground that reflects by a bidirectional reflectance factor rho(mu_out, mu_in, phi) is the sum over the number
 * of ground reflections: the solve over a black ground (specular surface, grd_alb = 0), then per reflection ("bounce") the
 * downward surface row of the previous term reflected through an operator, its unscattered upward field, and a black-ground
 * solve started from that field (sosrt_solve_dev, d_I1_in).  Five stages beside the solve, detected by symbol (SOSRT_VERSION is
 * unchanged); all are enqueued on the handle's stream and write their outputs only -- the handle's columns, resident field,
 * order targets and phase state stay as they were (like every stage, a call ends the run of adjacent launches that the
 * handle's profiling slots keep track of).  These build the azimuth mean (mode m = 0) of the BRDF; its modes m >= 1 follow below.
 *
 * Lanes: i = 0 .. N-2 is the upward direction N+1+i, j = 0 .. N-2 the downward direction j; the two mu = 0 nodes (N-1, N) take
 * no part.  rho_bar(a, b) = (1 / pi) int_0^pi rho(a, b, phi) dphi by the trapezoid rule on nphi nodes of [0, pi].
 *
 * sosrt_brdf_operator_dev: the operator with the quadrature of the reflected flux folded in,
 *     R(i, j) = 2 w_j |mu_j| rho_bar(mu_i, |mu_j|),   w the trapezoid weights of the nodes mu[0 .. N-2],
 * stored with the lanes i of one j contiguous: d_R_out[j (N-1) + i].  sosrt_brdf_beam_dev: r0[b][i] = rho_bar(mu_i, mu0[b]), the
 * reflection of the direct beam.  Kinds: SOSRT_BRDF_LAMBERTIAN (no parameters; rho = 1 -- the albedo is the per-column scale of
 * sosrt_ground_source_dev, and R is the in-loop Lambertian boundary of SOSRT_SURFACE_LAMBERTIAN_README up to the order of
 * summation) and SOSRT_BRDF_RPV (params = { rho0, k, Theta }, Rahman-Pinty-Verstraete:
 *     rho = rho0 (a b (a + b))^(k-1) (1 - Theta^2) / (1 + 2 Theta cos g + Theta^2)^(3/2) (1 + (1 - rho0) / (1 + G)),
 *     cos g = a b + sqrt(1-a^2) sqrt(1-b^2) cos phi,  G^2 = tan^2 a + tan^2 b - 2 tan a tan b cos phi, tan x = sqrt(1-x^2)/x,
 * G^2 evaluated as max(0, (tan a - tan b)^2 + 4 tan a tan b sin^2(phi/2)), which does not cancel at the hot spot a = b, phi = 0;
 * rho_bar is symmetric in (a, b)).  A caller with a BRDF of their own fills R and r0 themselves.
 *
 * sosrt_ground_source_dev: S[b][i] = scale[b] (sum_j R(i, j) I[b][L-1][j] + r0[b][i] exp(-tau[b][L-1] / mu0[b])), mu0 the
 * columns'; d_r0 NULL: no beam term (every bounce after the first); d_scale NULL: 1.  The sum runs over j ascending in fused
 * multiply-adds, one lane per i: a column's bits do not depend on B.
 *
 * sosrt_ground_first_order_dev: the unscattered field of the ground source,
 *     G[b][t][N+1+i] = S[b][i] exp(-(tau[b][L-1] - tau[b][t]) / mu_i),   G[b][t][N] = 0,   G[b][t][0 .. N-1] = 0,
 * then on every row the mu -> 0+ blend of the order loop's upward sweep (spec:402-409): k = N+1, while |(G[k] - G[k+1]) -
 * (G[k+1] - G[k+2])| > 1e-4: k += 1; k += 1; lanes N+1 .. k-1 become (1 - w) G[N] + w G[k], w = mu[m] / mu[k].  A search that
 * would read past lane 2N-1 (the reference raises IndexError there) leaves its row unblended and gives the column
 * SOSRT_COL_INDEXERROR in d_status (nullable; SOSRT_COL_OK otherwise).
 *
 * sosrt_bounce_accumulate_dev: I_total += Ik (one addition per element), and ratio[b] = the larger of max |Ik| / max |I_total|
 * over the upward lanes of row 0 and over the downward lanes of row L-1 (of the updated total; a row whose total is all zero
 * counts 0).
 *
 * Refused with SOSRT_E_INVALID, a message and nothing written: the single-slab geometry; B outside 1 .. the current columns; a
 * null pointer (d_r0, d_scale, d_status and the params of a kind without any aside); nphi < 3 or > SOSRT_BRDF_MAX_NPHI; an
 * unknown kind or a wrong nparams; RPV parameters outside rho0 > 0, k > 0, |Theta| < 1; N < 4.
 *
 * The kernel-driven Ross-Li model, rho = f_iso + f_vol K_vol + f_geo K_geo, is linear in its weights, and its
 * two kernels depend on the geometry only: they are two more kinds, each with params = { mu_floor } in [0, 1), and the isotropic
 * term is SOSRT_BRDF_LAMBERTIAN.  Every builder here and below takes them, with the guarantees it gives for RPV.  Both are
 * evaluated at a' = max(a, mu_floor), b' = max(b, mu_floor) (they carry sec theta and are not meant for grazing angles; 0: as
 * written); s = sqrt(max(0, 1 - c^2)), t = s / c per direction; cos xi = clip(a' b' + s_a s_b cos phi, -1, 1), xi = acos(cos xi):
 *     SOSRT_BRDF_ROSS_THICK    K_vol = ((pi/2 - xi) cos xi + sin xi) / (a' + b') - pi/4
 *     SOSRT_BRDF_LI_SPARSE_R   K_geo = O - sec + (1 + cos xi) / (2 a' b'),   sec = 1/a' + 1/b'   (h/b = 2, b/r = 1),
 *         O = (t - sin t cos t) sec / pi,   cos t = clip(2 sqrt(D^2 + (t_a t_b sin phi)^2) / sec, -1, 1),
 *         D^2 = (t_a - t_b)^2 + 2 t_a t_b (1 - cos phi)   (RPV's non-cancelling form),   sin^2 phi = (1 - cos phi)(1 + cos phi).
 * Neither is clamped: they cross zero, and K_geo is negative over most of the hemisphere.
 *
 * sosrt_ground_source_terms_dev: the ground source of K operator terms with per-column weights,
 *     S[b][i] = sum_k weight[b][k] c_k,   c_k = sum_j R_k(i, j) I[b][L-1][j] + r0_k[b][i] exp(-tau[b][L-1] / mu0[b])   (d_r0 NULL: none),
 * c_k the chain of sosrt_ground_source_dev without its scale, then acc = +0 and acc = fma(weight[b][k], c_k, acc) for k ascending.
 * So with K = 1 S has the bits of sosrt_ground_source_dev with scale = weight (up to the sign of a zero), a term of weight 0
 * leaves the bits alone, all weights 0 give +0, and a column's bits do not depend on B.  1 <= K <= SOSRT_BRDF_MAX_TERMS.  One
 * workgroup per column, the surface row staged once for the K operators.  Refused as sosrt_ground_source_dev refuses, and for K
 * outside its range or a null d_weight.
 *
 * SOSRT_BRDF_COX_MUNK: the sun glint of a rough water surface, the isotropic Gaussian slope distribution of
 * Cox and Munk with the unpolarised Fresnel reflectance of a real index and, optionally, the bidirectional Smith shadowing.
 * params = { sigma2, refractive_index, shadow }, exactly three: sigma2 finite and > 0 (the slope variance; Cox and Munk's wind
 * law is 0.003 + 0.00512 U), refractive_index finite and > 1, shadow exactly 0 or 1.  With s = sqrt(max(0, 1 - c^2)):
 *     rho = F(cos chi) exp(-t2 / sigma2) (1 + t2)^2 / (4 sigma2 a b) S,
 *     h2 = (s_a - s_b)^2 + 2 s_a s_b (1 + cos phi),   t2 = h2 / (a + b)^2,   cos^2 chi = (h2 + (a + b)^2) / 4,
 *     F(c) = (r_s^2 + r_p^2) / 2,   g = sqrt(n^2 - 1 + c^2),   r_s = (c - g) / (c + g),   r_p = (n^2 c - g) / (n^2 c + g),
 *     S = 1 / (1 + Lambda(a) + Lambda(b)) (shadow = 1; else 1),
 *     Lambda(c) = (sqrt(sigma2 / pi) exp(-cot^2 / sigma2) / cot - erfc(cot / sqrt(sigma2))) / 2,   cot = c / s,   Lambda(1) = 0.
 * phi = pi is the specular direction (phi = 0 with a = b is back-scatter, as for every kind).  h2 and cos^2 chi are sums of
 * non-negative terms; rho is symmetric in (a, b) and not clamped (toward grazing angles its hemispherical integral exceeds 1).
 * Every builder here and below takes the kind, with the guarantees it gives for RPV; a ground f_iso + f_glint rho is two operator
 * terms with SOSRT_BRDF_LAMBERTIAN.  Refused like the other kinds: nparams != 3, null params, a parameter outside its range. */
#define SOSRT_BRDF_LAMBERTIAN  0
#define SOSRT_BRDF_RPV         1
#define SOSRT_BRDF_ROSS_THICK  2
#define SOSRT_BRDF_LI_SPARSE_R 3
#define SOSRT_BRDF_COX_MUNK    4
#define SOSRT_BRDF_MAX_NPHI    65537
#define SOSRT_BRDF_MAX_TERMS   4
int sosrt_brdf_operator_dev(sosrt_t* h, int kind, const double* params /*host*/, int nparams, int nphi, double* d_R_out /*[N-1][N-1], [j][i]*/);
int sosrt_brdf_beam_dev(sosrt_t* h, int B, int kind, const double* params /*host*/, int nparams, int nphi, const double* d_mu0 /*[B]*/,
                        double* d_r0_out /*[B][N-1]*/);
int sosrt_ground_source_dev(sosrt_t* h, int B, const double* d_I /*[B][L][2N]*/, const double* d_tau /*[B][L]*/,
                            const double* d_R /*[N-1][N-1], [j][i]*/, const double* d_r0 /*[B][N-1] or NULL*/,
                            const double* d_scale /*[B] or NULL*/, double* d_S_out /*[B][N-1]*/);
int sosrt_ground_source_terms_dev(sosrt_t* h, int B, int K, const double* d_I /*[B][L][2N]*/, const double* d_tau /*[B][L]*/,
                                  const double* d_R /*[K][N-1][N-1], each [j][i]*/, const double* d_r0 /*[K][B][N-1] or NULL*/,
                                  const double* d_weight /*[B][K]*/, double* d_S_out /*[B][N-1]*/);
int sosrt_ground_first_order_dev(sosrt_t* h, int B, const double* d_tau /*[B][L]*/, const double* d_S /*[B][N-1]*/,
                                 double* d_G_out /*[B][L][2N]*/, int* d_status /*[B] or NULL*/);
int sosrt_bounce_accumulate_dev(sosrt_t* h, int B, const double* d_Ik /*[B][L][2N]*/, double* d_I_total /*[B][L][2N]*/,
                                double* d_ratio_out /*[B]*/);

/* ---- BRDF ground, azimuth-resolved: the reflection modes m >= 1 --------------------------------------------
 * The Fourier modes in azimuth of the BRDF, for the azimuth-resolved radiance over a BRDF ground.  With the ring angle phi of the
 * azimuth modes above (phi = 0 at an upward mu = mu0 is back-scatter, which is RPV's hot spot phi = 0),
 *     rho^m(a, b) = (1 / pi) int_0^pi rho(a, b, phi) cos(m phi) dphi
 * by the trapezoid rule on the nphi nodes phi_q = pi q / (nphi - 1) of rho_bar = rho^0.  cos(m phi_q) is taken of the integer m q
 * reduced modulo 2 (nphi - 1): node nphi - 1 gives (-1)^m and m = 0 gives 1 exactly, so MODE 0 HAS THE BITS OF
 * sosrt_brdf_operator_dev / sosrt_brdf_beam_dev at the same nphi.  rho at a (pair, node) is evaluated once per launch for up to 8
 * modes; more modes are further launches.
 *     sosrt_brdf_operator_modes_dev   R^m(i, j) = 2 w_j |mu_j| rho^m(mu_i, |mu_j|), d_R_out[m - m_first][j (N-1) + i]
 *     sosrt_brdf_beam_modes_dev       r0^m[b][i] = rho^m(mu_i, mu0[b]),             d_r0_out[m - m_first][b][i]
 * The ground source of mode m of the radiance is
 *     S^m = scale ((-1)^m R^m I^m[L-1] + [bounce 1] r0^m exp(-tau* / mu0)):
 * the down-welling lane and the reflected lane stand at the BRDF's relative azimuth phi_i - phi_j + pi, the pi of the fold of the
 * phase matrices, so the operator carries (-1)^m and the beam row, like P0, none.  sign_odd != 0 writes mode m as (-1)^m R^m
 * (negation is exact): what sosrt_ground_source_dev takes for mode m.  Everything after S^m is the series above unchanged, with
 * ((-1)^m P^m, order targets) on the handle.  The modes of a Lambertian ground vanish for m >= 1 (to rounding: <= 1e-15).
 * Modes: m_first >= 0, m_count >= 1, m_first + m_count - 1 <= min(SOSRT_MAX_MODES, nphi - 2).  Refused as the two entry points
 * above refuse, and for a range of modes outside that, with SOSRT_E_INVALID, a message and nothing written.  Enqueued on the
 * handle's stream; they write their outputs only. */
int sosrt_brdf_operator_modes_dev(sosrt_t* h, int kind, const double* params /*host*/, int nparams, int nphi, int m_first, int m_count,
                                  int sign_odd, double* d_R_out /*[m_count][N-1][N-1], [m][j][i]*/);
int sosrt_brdf_beam_modes_dev(sosrt_t* h, int B, int kind, const double* params /*host*/, int nparams, int nphi, int m_first,
                              int m_count, const double* d_mu0 /*[B]*/, double* d_r0_out /*[m_count][B][N-1]*/);

/* ---- BRDF ground seen from a view lane: the ground's term of the view stage --------------------------------
 * Over a BRDF ground the field is the sum over ground reflections I = sum_k I(k), and the radiance at a view cosine off the grid
 * is the sum of (1) the closed-form first order over the black ground, (2) sosrt_view_radiance_dev on the SUMMED field with the
 * black-ground columns (the stage is linear in d_I_src) and (3) the ground's own unscattered radiance at the view lanes:
 *     upward lane V + v:   sum_k S_k[b][v] exp(-(tau[b][L-1] - tau[b][t]) / mu_view[v]),      downward lanes: +0,
 *     S_k[b][v] = scale[b] (sum_j Rv[v][j] I(k-1)[b][L-1][j] + [k = 1] r0v[b][v] exp(-tau[b][L-1] / mu0[b])),
 *     Rv[v][j] = 2 w_j |mu_j| rho_bar(mu_view[v], |mu_j|),   r0v[b][v] = rho_bar(mu_view[v], mu0[b]).
 * No view lane is blended.  Per azimuth mode m the same with (-1)^m Rv^m, rho^m and the mode's fields; the beam's single
 * reflection may instead be taken exactly at an azimuth, rho(mu_view, mu0, phi) (phi = 0: the hot spot).  Four stages, detected by
 * symbol (SOSRT_VERSION is unchanged), enqueued on the handle's stream, without scratch; they write their outputs only.
 *     sosrt_brdf_view_rows_modes_dev    d_out[m - m_first][j V + v] = 2 w_j |mu_j| rho^m(mu_view[v], |mu_j|)   ((-1)^m with sign_odd)
 *     sosrt_brdf_view_beam_modes_dev    d_out[m - m_first][b][v] = rho^m(mu_view[v], mu0[b])
 *     sosrt_brdf_view_beam_azimuth_dev  d_out[q][b][v] = rho(mu_view[v], mu0[b], d_phi[q]), no quadrature
 * At a view cosine equal to the node mu[N+1+i] the first two have THE BITS OF sosrt_brdf_operator_modes_dev's column i and of
 * sosrt_brdf_beam_modes_dev (mode 0: of the azimuth-mean entry points).
 * sosrt_view_ground_dev: one workgroup per column, one lane per v, the sum over j ascending in fused multiply-adds -- the chain of
 * sosrt_ground_source_dev, so a column's bits do not depend on B and at a node d_S_out equals that entry point's S[i].  d_I and
 * d_Rv both NULL: the beam-only call; d_r0v NULL: the diffuse-only call; d_scale NULL: 1.  accumulate != 0 adds the upward lanes
 * to d_out and leaves the downward ones; otherwise both are written (downward: +0).  d_S_out (nullable) receives S.
 * Refused with SOSRT_E_INVALID, a message and nothing written: what the builders above refuse (single slab, B outside 1 .. the
 * current columns, kind, nparams, RPV parameters, nphi, the range of modes, N < 4, null pointers); V outside 1..SOSRT_MAX_VIEWS; a
 * mu_view that is not finite or outside [0.01, 1]; a level outside [0, L); nphi_out < 1; d_I without d_Rv or d_Rv without d_I;
 * no source at all (d_I, d_Rv and d_r0v NULL).
 * sosrt_view_ground_terms_dev: sosrt_view_ground_dev over K operator terms with per-column weights, S as in
 * sosrt_ground_source_terms_dev with Rv [K][N-1][V] and r0v [K][B][V] -- the same arithmetic and the same four consequences.  It
 * refuses what sosrt_view_ground_dev refuses, K outside 1..SOSRT_BRDF_MAX_TERMS and a null d_weight. */
int sosrt_brdf_view_rows_modes_dev(sosrt_t* h, int kind, const double* params /*host*/, int nparams, int nphi, int m_first,
                                   int m_count, int sign_odd, int V, const double* mu_view /*host [V]*/,
                                   double* d_out /*[m_count][N-1][V]*/);
int sosrt_brdf_view_beam_modes_dev(sosrt_t* h, int B, int kind, const double* params /*host*/, int nparams, int nphi, int m_first,
                                   int m_count, const double* d_mu0 /*[B]*/, int V, const double* mu_view /*host [V]*/,
                                   double* d_out /*[m_count][B][V]*/);
int sosrt_brdf_view_beam_azimuth_dev(sosrt_t* h, int B, int kind, const double* params /*host*/, int nparams,
                                     const double* d_mu0 /*[B]*/, int V, const double* mu_view /*host [V]*/, int nphi_out,
                                     const double* d_phi /*[nphi_out]*/, double* d_out /*[nphi_out][B][V]*/);
int sosrt_view_ground_dev(sosrt_t* h, int B, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                          const double* d_I /*[B][L][2N] or NULL*/, const double* d_Rv /*[N-1][V] or NULL*/,
                          const double* d_r0v /*[B][V] or NULL*/, const double* d_scale /*[B] or NULL*/, int nlev,
                          const int* levels /*host [nlev]*/, int accumulate, double* d_S_out /*[B][V] or NULL*/,
                          double* d_out /*[B][nlev][2V]*/);
int sosrt_view_ground_terms_dev(sosrt_t* h, int B, int K, int V, const double* mu_view /*host [V]*/, const double* d_tau /*[B][L]*/,
                                const double* d_I /*[B][L][2N] or NULL*/, const double* d_Rv /*[K][N-1][V] or NULL*/,
                                const double* d_r0v /*[K][B][V] or NULL*/, const double* d_weight /*[B][K]*/, int nlev,
                                const int* levels /*host [nlev]*/, int accumulate, double* d_S_out /*[B][V] or NULL*/,
                                double* d_out /*[B][nlev][2V]*/);

/* ---- multi-GPU: one process per GPU, columns sharded, ONE collective at the end ------------------
 * Nothing in SOS_Aer_main_specular.py:104-458 couples columns, so the order loop never communicates; these entry
 * points only assemble the results of the ranks on `root` over RCCL (xGMI inside a node).  RCCL is bound at run time
 * (dlopen): the library has no link-time dependency on it.
 *   sosrt_comm_unique_id  rank 0 fills id_out[128] (ncclGetUniqueId); the caller hands it to the other ranks by any
 *                         means (file, MPI, torch.distributed store, environment).
 *   sosrt_comm_init       every rank, same id: ncclCommInitRank on the handle's device.
 *   sosrt_gather          every rank: counts[world] doubles per rank (ragged shards allowed, counts[r] may be 0),
 *                         d_send = this rank's counts[rank] doubles (device), d_recv on root = the ranks' blocks one
 *                         after the other (device, sum of counts; ignored elsewhere).  Enqueued on the handle's stream
 *                         as ncclSend / ncclRecv pairs in one group -- a gather over the point-to-point links, each
 *                         sender on its own link to the root.
 *   sosrt_comm_destroy    ncclCommDestroy. */
int sosrt_comm_unique_id(void* id_out);
int sosrt_comm_init(sosrt_t* h, int rank, int world, const void* unique_id);
int sosrt_gather(sosrt_t* h, int root, const long long* counts, const double* d_send, double* d_recv);
int sosrt_comm_destroy(sosrt_t* h);

/* ---- helper level (In_limit:70,113) on device, host pointers -------------------------------- */
/* rows [R][N] of downward radiances; returns the idx rewritten values per row: out [R][idx] with
 * out[r][i] = improved_limit_mu_down(rows[r], mu[:N], N, idx, i). */
int sosrt_limit_mu_down(sosrt_t* h, int R, int idx, const double* rows, double* out);
/* out[r] = improved_asymptotic_downward_radiance(J[r][:len[r]], tau[r][:len[r]], tau_t[r], mu[r]);
 * J, tau are [R][stride]. */
int sosrt_asymptotic_down(sosrt_t* h, int R, int stride, const int* len, const double* J, const double* tau,
                          const double* tau_t, const double* mu, double* out);

/* ---- plan introspection (host only, no GPU needed) ------------------------------------------ */
int sosrt_plan_weights(sosrt_t* h, double* w_out /*2N*/);
/* (which: until ABI 104 any non-zero value meant W_aer; from 105 on a value outside 0 .. sets is SOSRT_E_INVALID) */
int sosrt_plan_fold(sosrt_t* h, int which /*0 atm, 1 aer, 1 + s: aerosol set s of sosrt_set_phase_sets*/, double* W_out /*2N x 2N, W[k][m]*/);
/* a4b table for a given rewritten-angle count idx: s0 (first source lane), ns (sources),
 * C_out [idx][ns] (ns <= 5). */
int sosrt_plan_fix_table(sosrt_t* h, int idx, int* s0, int* ns, double* C_out);
int sosrt_plan_fix_count(double tau_ref, int N);  /* I1_In:124-127 */
/* The kernels an order of the order loop launches, as sosrt_solve_dev decides it (one function of the handle's shape and knobs;
 * needs sosrt_set_grid only): a batch of `batch` columns with up to `zones` zones each (3: the reference's clear / slab / clear)
 * over `surface`, of whose first column group `live` columns are still live, on a device of `cus` CUs (0: the handle's).
 * out[9] = { column groups of the batch, SOSRT_PLAN_GEMM_*, capacity of the live-column contraction (0: dense tiling),
 *            SOSRT_PLAN_TRANSPORT_*, workgroups per column of the chunk-parallel transport, 1 if the general kernel follows as
 *            a repair pass, 1 if this and all later orders go into one order-loop launch, its transport workgroups per
 *            column, its grid }. */
#define SOSRT_PLAN_GEMM_DENSE        0   /* 64-row tiles over the batch's row lists (tiles of converged columns leave at once) */
#define SOSRT_PLAN_GEMM_LIVE64       1   /* tiles laid over the live columns, 64 rows                                           */
#define SOSRT_PLAN_GEMM_LIVE32       2   /* ... 32 rows (at most 200 live columns)                                              */
#define SOSRT_PLAN_GEMM_LIVE32_DEEP  3   /* ... both operands staged two chunks ahead (at most 32 live columns)                */
#define SOSRT_PLAN_GEMM_LIVE16_REGS  4   /* ... 16 rows, a lane's matrix fragments in registers, no barrier in the k-loop (the   */
                                         /*     last few live columns of the symmetric form: a tile's latency is the launch's)    */
/* (the library's own name for these is TransportKernel, csrc/kernels.hpp; 2 is its repair pass, reported in out[5], never here) */
#define SOSRT_PLAN_TRANSPORT_GENERAL 0   /* kernels.hip k_transport                                                             */
#define SOSRT_PLAN_TRANSPORT_FAST    1   /* transport_fast.hip (odd N, N > 256)                                                 */
#define SOSRT_PLAN_TRANSPORT_RING    3   /* transport_ring.hip                                                                  */
#define SOSRT_PLAN_TRANSPORT_SCAN    4   /* transport_scan.hip (chunk-parallel)                                                 */
int sosrt_plan_launch(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int* out /*[9]*/);
/* The same plan's decision on the ring kernel's moment mode (both launches of the order: the contraction writes a 64-byte
 * moment record per plain row instead of the row of Jn, the ring kernel expands it -- the same bits): *on = 1 or 0.  Unlike
 * sosrt_plan_launch it plans with the phase matrices the handle HAS (none: no low-rank form, so 0).  flags: what a host-only
 * handle cannot be told otherwise.  SOSRT_RING_MOMENTS=0 at sosrt_create turns the mode off for the handle. */
#define SOSRT_PLAN_SAVED_ORDERS 1   /* the caller wants every order's field                */
#define SOSRT_PLAN_ATM_SETS     2   /* some column reads an atmosphere phase set            */
#define SOSRT_PLAN_NEED_SMALLMU 4   /* some |mu| < 0.01 lane keeps its k_smallmu value      */
int sosrt_plan_ring_moments(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int flags, int* on);
/* What the last solve did, where the query above says what a plan would allow: the (column group, order) pairs that the contraction
 * and the ring kernel ran in moment mode, and all the pairs that the two-launch loop ran (either pointer nullable).  The mode also
 * stays off while some |mu| < 0.01 lane keeps its k_smallmu value, which only the solve knows (SOSRT_PLAN_NEED_SMALLMU). */
int sosrt_ring_moments_stats(sosrt_t* h, int* moment_orders, int* orders);
/* The moment mode of the chunk-parallel kernel (transport_scan.hip), a second and separate decision of the same plan: in an order
 * that kernel transports in its one-workgroup or split form (not the WIDE instantiation), under the conditions of the ring
 * kernel's mode, the contraction writes the same records and the chunk-parallel kernel expands them -- the same bits.  *on = 1 or
 * 0; never 1 where sosrt_plan_ring_moments answers 1.  Arguments and flags as above.  Knobs, read once at sosrt_create:
 * SOSRT_SCAN_MOMENTS=0 turns the mode off for the handle; SOSRT_SCAN_MOMENTS_MIN=n keeps it to the orders whose column group has
 * at least n planned live columns (default 128, measured on the headline sweep: DESIGN section 3a; below it the transport's
 * launch sits on its latency floor, where the expansion costs more than the contraction's smaller writes save). */
int sosrt_plan_scan_moments(sosrt_t* h, int batch, int live, int surface, int zones, int cus, int flags, int* on);
/* What the last solve did: the (column group, order) pairs that the contraction and the chunk-parallel kernel ran in moment mode,
 * and all the pairs that the two-launch loop ran (the same count sosrt_ring_moments_stats reports; either pointer nullable). */
int sosrt_scan_moments_stats(sosrt_t* h, int* moment_orders, int* orders);

/* ---- profiling: HIP-event timing of the dominant kernels on the handle's stream ------------- */
#define SOSRT_K_GEMM      0
#define SOSRT_K_TRANSPORT 1
#define SOSRT_K_FIRST     2
#define SOSRT_K_SMALLMU   3
#define SOSRT_K_ORDER_LOOP 4  /* the order-loop launches (several orders of a few columns each) */
#define SOSRT_K_COUNT     5
int sosrt_profile_enable(sosrt_t* h, int on);
int sosrt_profile_reset(sosrt_t* h);
/* total milliseconds and launch count since the last reset (synchronises the stream) */
int sosrt_profile_get(sosrt_t* h, int kernel, double* total_ms, long long* launches, double* work /*flops or bytes*/);

/* ---- diagnostics: device buffer [B][2][8] of clock64() stamps written by the fast transport kernel
 * (start, prologue done, downward done, surface done, upward done, end); NULL switches it off.  The buffer belongs to this
 * handle: only its transport launches write it, and it is forgotten with the handle. */
int sosrt_debug_stamps(sosrt_t* h, unsigned long long* d_stamps);

/* ---- machine peaks measured on this device (roofline denominators) --------------------------- */
/* which 0: back-to-back v_mfma_f64_16x16x4_f64, TFLOP/s; 1: streaming copy of 1 GiB, GB/s (read+write);
 * 2: v_fma_f64, TFLOP/s. */
int sosrt_microbench(sosrt_t* h, int which, double* result);

#ifdef __cplusplus
}
#endif
#endif /* SOSRT_H */
