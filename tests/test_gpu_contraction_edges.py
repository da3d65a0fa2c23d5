"""The source-function contraction on the device at every rank, tiling and edge shape (csrc/jn_gemm_tile.hpp: lowrank_rows /
lowrank_tile and the MFMA tiles; csrc/jn_gemm_f32.hip): Legendre-series atmospheres of 0 .. 5 terms, with and without the flip
symmetry, against a long-double sum -- per element, inside bounds derived from the summations (tests/legendre_phase.py: bounds)
-- and whole solves of ranks 1, 3, 4 against the oracle, against the dense contraction and, bit for bit, across the tilings."""
import functools

import numpy as np
import pytest

import legendre_phase as LP
import sos_oracle as O
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from sosrt.solver import Solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu

MODES = ("f64", "f64_dense", "f64_full", "f32")
# case -> (terms of the atmosphere's series, no_flip, the rank sosrt_phase_rank must answer)
CASES = {"zero": (0, False, 0), "r1": (1, False, 1), "r2": (2, False, 2), "r3": (3, False, 3), "r4": (4, False, 4),
         "five_terms": (5, False, -1), "r3_no_flip": (3, True, 3)}
# (L, N, B, geometry): ("slab", first row, last row) | ("single",) every row plain | ("zones", table per column).  N = 4, 6, 37:
# D < 128, lanes with nothing to do; 63, 100, 501: D % 128 != 0 and D % 16 != 0; one-row slabs and plain-row counts that are no
# multiple of 4 or 16: partial LR_ROWS groups.  The zone tables have SOSRT_MAX_ZONES zones: three one- or two-row slabs (an aerosol
# zone needs a clear one on either side, so eight zones hold no fourth) and two clear zones at the bottom.
SHAPES = {
    "L9_N4": (9, 4, 1, ("slab", 3, 3)),
    "L9_N6": (9, 6, 1, ("slab", 2, 5)),
    "L21_N37_B2": (21, 37, 2, ("slab", 7, 7)),
    "L19_N63": (19, 63, 1, ("slab", 1, 16)),
    "L37_N100_B3": (37, 100, 3, ("slab", 10, 20)),
    "L24_N256": (24, 256, 1, ("slab", 5, 9)),
    "L12_N501": (12, 501, 1, ("slab", 4, 6)),
    "single_L21_N37_B2": (21, 37, 2, ("single",)),
    "zones_L40_N64_B2": (40, 64, 2, ("zones", [[0, 3, 4, 9, 11, 17, 18, 30], [0, 5, 7, 12, 13, 20, 22, 35]])),
}
ZONE_MIX = [0, 1, 0, 1, 0, 1, 0, 0]          # SOSRT_MAX_ZONES = 8 entries


@functools.lru_cache(maxsize=None)
def _hg(N):
    """The aerosol matrix: not low-rank, so slab rows keep the MFMA product."""
    return inputs.phase_function("hg", N, inputs.direction_grid(N), 0.5, 0.7)[1]


@functools.lru_cache(maxsize=None)
def _atmosphere(N, case):
    r, no_flip, _ = CASES[case]
    return LP.legendre_phase(N, inputs.direction_grid(N), LP.terms(r), no_flip=no_flip)[0]


def _column_scalars(B):
    b = np.arange(B)
    return dict(mu0=0.45 + 0.2 * b, rho=0.1 * b, alb_atm=1.0 - 0.1 * b, alb_aer=0.95 - 0.1 * b, dtau_atm=0.002 * (1 + b),
                dtau_aer=0.03 / (1 + b))


def _set_columns(s, L, B, geom):
    """Columns with different mu0 and albedos each.  Returns (ca, cr [B, L], slab [B, L]) as k_prepare computes them
    (csrc/kernels.hip: ca = (alb_atm / 4) fa, cr = (alb_aer / 4) fr in a slab, alb_atm / 4 elsewhere)."""
    c = _column_scalars(B)
    ca = np.repeat((c["alb_atm"] / 4)[:, None], L, axis=1)
    cr = np.zeros((B, L))
    slab = np.zeros((B, L), bool)
    if geom[0] == "single":
        s.set_columns_single_slab(c["mu0"], c["alb_atm"], np.full(B, 0.3))
        return ca, cr, slab
    fa = c["dtau_atm"] / (c["dtau_atm"] + c["dtau_aer"])
    fr = c["dtau_aer"] / (c["dtau_atm"] + c["dtau_aer"])
    if geom[0] == "slab":
        iu, idn = geom[1], geom[2]
        s.set_columns(np.full(B, iu), np.full(B, idn), c["mu0"], c["rho"], c["alb_atm"], c["alb_aer"], c["dtau_atm"], c["dtau_aer"],
                      np.full(B, 0.5))
        slab[:, iu:idn + 1] = True
    else:
        zr0 = np.array(geom[1], dtype=np.int32)
        nz = zr0.shape[1]
        zwr = np.repeat(c["alb_aer"][:, None], nz, axis=1)
        zdt = np.repeat(c["dtau_aer"][:, None], nz, axis=1)
        s.set_columns_zones(zr0, np.tile(ZONE_MIX, (B, 1)), c["mu0"], c["rho"], c["alb_atm"], c["dtau_atm"], zwr, zdt, np.full(B, 0.5))
        for b in range(B):
            for z in range(nz):
                if ZONE_MIX[z]:
                    slab[b, zr0[b, z]:zr0[b, z + 1]] = True
    for b in range(B):
        ca[b, slab[b]] = (c["alb_atm"][b] / 4) * fa[b]
        cr[b, slab[b]] = (c["alb_aer"][b] / 4) * fr[b]
    return ca, cr, slab


def _edge_input(rng, B, L, D, slab):
    """Random signs, magnitudes over six decades; in every column three plain rows are a row of zeros, a single 1.0 at k = D - 1
    and a single 1.0 at k = 0 (with three plain rows in all, the zeros go to a slab row and one plain row stays random), the first
    slab row a single 1.0 at k = D - 1 and (slabs of two rows or more) the last slab row a single 1.0 at k = 0.  Returns
    (X [B, L, D], [(b, row, k)] of the single-1.0 rows)."""
    X = rng.choice([-1.0, 1.0], (B, L, D)) * 10.0 ** rng.uniform(-6, 0, (B, L, D))
    ones = []
    for b in range(B):
        plain = np.flatnonzero(~slab[b])
        rows = np.flatnonzero(slab[b])
        X[b, plain[0] if plain.size > 3 else rows[rows.size // 2]] = 0.0
        X[b, plain[1:3]] = 0.0
        X[b, plain[1], D - 1] = 1.0
        X[b, plain[2], 0] = 1.0
        ones += [(b, int(plain[1]), D - 1), (b, int(plain[2]), 0)]
        if rows.size:
            X[b, rows[0]] = 0.0
            X[b, rows[0], D - 1] = 1.0
            ones.append((b, int(rows[0]), D - 1))
        if rows.size > 1:
            X[b, rows[-1]] = 0.0
            X[b, rows[-1], 0] = 1.0
            ones.append((b, int(rows[-1]), 0))
    return X, ones


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", list(CASES))
def test_source_at_every_rank_against_the_long_double_sum(case, shape):
    """Solver.source in the four contraction modes, per element within the derived bound of its mode (legendre_phase.bounds); the
    largest error / bound of every mode is printed before it is asserted.  Also: the rank and the forms the handle reports in
    every mode, no NaN, the first f64 result bit for bit after the other modes, the single-1.0 rows against rows 0 and D - 1 of
    c W, exact zeros for the plain rows of a zero matrix, and f64 == f64_dense bit for bit when the factors were refused."""
    L, N, B, geom = SHAPES[shape]
    terms, no_flip, want_rank = CASES[case]
    D = 2 * N
    mu = inputs.direction_grid(N)
    Pa, Pr = _atmosphere(N, case), _hg(N)
    s = Solver(L, N, max_batch=B)
    try:
        s.set_grid(mu)
        s.set_phase(Pa, None if geom[0] == "single" else Pr)
        rank, res, uses = s.phase_rank()
        asym, sym = s.phase_asymmetry()
        assert rank == want_rank and uses == (rank >= 0), (rank, res, uses)
        assert sym == (not no_flip), asym
        ca, cr, slab = _set_columns(s, L, B, geom)
        X, ones = _edge_input(np.random.default_rng(1000 * L + N), B, L, D, slab)
        J = {}
        for mode in MODES:
            s.set_contraction(mode)
            assert s.phase_rank()[2] == (mode == "f64" and rank >= 0)
            assert s.phase_asymmetry()[1] == (sym and mode in ("f64", "f64_dense"))
            J[mode] = s.source(X)
            assert not np.isnan(J[mode]).any(), mode
        s.set_contraction("f64")
        assert np.array_equal(s.source(X), J["f64"]), "f64 after the other modes"
        Wa = s.plan_fold(0)
    finally:
        s.close()
    UV = LP.factor(Wa) if rank >= 0 else None
    assert UV is None or UV[0].shape[1] == rank
    worst = dict.fromkeys(MODES, 0.0)
    Wa_ld, Wr_ld = LP.fold_ld(Pa, mu), LP.fold_ld(Pr, mu)
    for b in range(B):
        J_ld, bound = LP.bounds(X[b], mu, Pa, Pr if slab[b].any() else None, ca[b], cr[b], Wa, sym, UV)
        for mode in MODES:
            worst[mode] = max(worst[mode], LP.worst_ratio(J[mode][b], J_ld, bound[mode]))
        # a single 1.0 at k reproduces row k of c W (column 0 / D - 1 of the reference's c P[:, ::-1] w): a transposed or shifted
        # factor, or a dropped first or last element, fails here outright
        for (bb, t, k) in ones:
            if bb != b:
                continue
            want = ca[b, t] * Wa_ld[k] + (cr[b, t] * Wr_ld[k] if slab[b, t] else 0)
            for mode in MODES:
                assert np.all(np.abs(J[mode][b, t] - want) <= bound[mode][t]), (mode, b, t, k)
        if case == "zero":
            for mode in ("f64", "f64_dense", "f64_full"):
                assert not J[mode][b][~slab[b]].any(), mode            # exactly 0.0
    print("RATIO %-10s %-18s " % (case, shape) + " ".join("%s=%.4f" % (m, worst[m]) for m in MODES))
    for mode in MODES:
        assert worst[mode] <= 1.0, "%s: error / bound = %.3f" % (mode, worst[mode])
    if case == "five_terms":
        assert np.array_equal(J["f64"], J["f64_dense"])                  # nothing low-rank ran


# ---- whole solves: ranks 1, 3, 4 (and 0) through every tiling ----------------------------------------------------------------------
SOLVES = {"L72_N64_B40": (72, 64, 40), "L200_N128_B24": (200, 128, 24)}
KNOBS = ("SOSRT_GEMM_REGS", "SOSRT_GEMM_SMALL", "SOSRT_DENSE_LIVE_LIST", "SOSRT_GROUPS", "SOSRT_SPLIT_MIN", "SOSRT_ORDER_LOOP")


def _fresh(monkeypatch=None, **env):
    from sosrt import main as M
    if monkeypatch is not None:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    for s_ in list(M._solvers.values()):
        s_.close()
    M._solvers.clear()


@functools.lru_cache(maxsize=None)
def _batch(L, N, B, r):
    """Columns that converge at different orders: (mu0, tau_aer, rho [B], keywords of SOS_Aer_batch with the phase arrays)."""
    rng = np.random.default_rng(100 * L + N + r)
    mu = inputs.direction_grid(N)
    mu0 = rng.uniform(0.2, 1.0, B)
    taer = rng.choice([0.02, 0.12, 0.6], B)
    rho = rng.uniform(0.0, 0.8, B)
    Pa = LP.legendre_phase(N, mu, LP.terms(r))[0]
    P0a = np.stack([LP.legendre_phase(N, mu, LP.terms(r), mu0=m)[1] for m in mu0])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in mu0])
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa, P_aer=_hg(N))
    return mu0, taer, rho, P0a, P0r, kw


_default = {}


def _default_run(monkeypatch, L, N, B, r):
    """The batch with no knob set, on a fresh handle; computed once and shared (nothing writes to it)."""
    key = (L, N, B, r)
    if key not in _default:
        mu0, taer, rho, P0a, P0r, kw = _batch(L, N, B, r)
        _fresh(monkeypatch)
        _default[key] = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P0_aer=P0r, **kw)
        _fresh()
    return _default[key]


def _oracle(L, N, r, mu0, taer, rho, P0a, P0r, kw):
    c = O.make_column(mu0, 120, 25, 17, L, 0.124, taer, rho, 1.0, 0.95, N, P0a, kw["P_atm"], P0r, kw["P_aer"])
    return O.solve_column(c, literal=False)


@pytest.mark.parametrize("r", [1, 3, 4])
@pytest.mark.parametrize("shape", list(SOLVES))
def test_whole_columns_of_rank_1_3_4_against_the_oracle_and_the_dense_contraction(shape, r, monkeypatch):
    """A Legendre atmosphere of r terms over the HG aerosol: three columns (the slowest, the fastest, one more) against the oracle
    at RTOL with equal order counts; the whole batch against f64_dense on the same handle, equal order counts and 1e-12."""
    from sosrt import main as M
    L, N, B = SOLVES[shape]
    mu0, taer, rho, P0a, P0r, kw = _batch(L, N, B, r)
    lr = _default_run(monkeypatch, L, N, B, r)
    assert (lr.status == 0).all() and lr.n.max() > lr.n.min()
    _fresh(monkeypatch)
    again = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P0_aer=P0r, **kw)
    (s,) = M._solvers.values()
    assert s.phase_rank()[0] == r and s.phase_rank()[2]
    assert np.array_equal(again.I, lr.I) and np.array_equal(again.n, lr.n)
    s.set_contraction("f64_dense")
    assert not s.phase_rank()[2]
    dense = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P0_aer=P0r, **kw)
    assert len(M._solvers) == 1
    _fresh()
    assert (dense.status == 0).all() and np.array_equal(lr.n, dense.n)
    assert_close(lr.I, dense.I, 1e-12, "low-rank against dense")
    for b in sorted({int(np.argmax(lr.n)), int(np.argmin(lr.n)), B // 2}):
        ref = _oracle(L, N, r, mu0[b], taer[b], rho[b], P0a[b], P0r[b], kw)
        assert int(lr.n[b]) == ref.n, (b, lr.n[b], ref.n)
        assert_close(lr.I[b], ref.I, RTOL, "rank %d, column %d" % (r, b))


@pytest.mark.parametrize("knob", ["gemm_regs_0", "gemm_small_0", "dense_live_list_0", "two_groups", "order_loop_1",
                                  "alone_and_sub_batch"])
@pytest.mark.parametrize("r", [1, 3, 4])
@pytest.mark.parametrize("shape", list(SOLVES))
def test_whole_columns_of_rank_1_3_4_keep_their_bits_across_the_tilings(shape, r, knob, monkeypatch):
    """Every tiling computes its plain rows in lowrank_rows, so a row's bits do not depend on the tiling, the batch or the launch:
    the default run against the staged live-column tilings (SOSRT_GEMM_REGS=0), the dense tiling until the live-column ones
    (SOSRT_GEMM_SMALL=0), the transport over all columns (SOSRT_DENSE_LIVE_LIST=0), two column groups, the order loop (off unless asked for; its
    launches ran and were not refused), and a column alone and in a sub-batch of 7 -- fields and order counts bit for bit."""
    from sosrt import main as M
    L, N, B = SOLVES[shape]
    mu0, taer, rho, P0a, P0r, kw = _batch(L, N, B, r)
    ref = _default_run(monkeypatch, L, N, B, r)
    env = {"gemm_regs_0": {"SOSRT_GEMM_REGS": "0"}, "gemm_small_0": {"SOSRT_GEMM_SMALL": "0"},
           "dense_live_list_0": {"SOSRT_DENSE_LIVE_LIST": "0"}, "two_groups": {"SOSRT_GROUPS": "2", "SOSRT_SPLIT_MIN": "2"},
           "order_loop_1": {"SOSRT_ORDER_LOOP": "1"}, "alone_and_sub_batch": {}}[knob]
    _fresh(monkeypatch, **env)
    try:
        if knob == "alone_and_sub_batch":
            lo = B // 3
            sub = SOS_Aer_batch(mu0[lo:lo + 7], taer[lo:lo + 7], rho[lo:lo + 7], P0_atm=P0a[lo:lo + 7], P0_aer=P0r[lo:lo + 7], **kw)
            assert np.array_equal(sub.n, ref.n[lo:lo + 7]) and np.array_equal(sub.I, ref.I[lo:lo + 7])
            for c in sorted({int(np.argmax(ref.n)), int(np.argmin(ref.n)), B - 1}):
                one = SOS_Aer_batch(mu0[c:c + 1], taer[c:c + 1], rho[c:c + 1], P0_atm=P0a[c:c + 1], P0_aer=P0r[c:c + 1], **kw)
                assert one.n[0] == ref.n[c], c
                assert np.array_equal(one.I[0], ref.I[c]), c
            return
        out = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P0_aer=P0r, **kw)
        (s,) = M._solvers.values()
        assert s.phase_rank()[0] == r and s.phase_rank()[2]
        plans = {live: s.plan_launch(B, live) for live in (B, 2)}
        if knob == "gemm_regs_0":
            assert plans[2]["gemm"] == _lib.PLAN_GEMM_LIVE32_DEEP, plans
        else:
            assert plans[2]["gemm"] == _lib.PLAN_GEMM_LIVE16_REGS, plans
        if knob == "gemm_small_0":
            assert plans[B]["gemm"] == _lib.PLAN_GEMM_DENSE, plans
        assert plans[B]["groups"] == (2 if knob == "two_groups" else 1), plans
        launches = s.order_loop_stats()
        if knob == "order_loop_1":
            assert launches[0] >= 1 and launches[1] == 0, launches      # it ran, and was never refused
        else:
            assert launches[0] == 0, launches
        assert np.array_equal(out.n, ref.n), (out.n, ref.n)
        assert np.array_equal(out.status, ref.status)
        assert np.array_equal(out.I, ref.I)                              # bit for bit
    finally:
        _fresh()


def test_whole_columns_over_a_zero_atmosphere_against_the_oracle(monkeypatch):
    """r = 0: the plain rows are written as zeros, only the aerosol slab scatters."""
    from sosrt import main as M
    L, N, B = 72, 64, 4
    mu = inputs.direction_grid(N)
    mu0 = np.array([0.3, 0.5, 0.7, 0.9]); taer = np.array([0.6, 0.12, 0.6, 0.02]); rho = np.array([0.0, 0.3, 0.6, 0.8])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in mu0])
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=np.zeros((2 * N, 2 * N)), P_aer=_hg(N))
    _fresh(monkeypatch)
    try:
        r = SOS_Aer_batch(mu0, taer, rho, P0_atm=np.zeros((B, 2 * N)), P0_aer=P0r, **kw)
        (s,) = M._solvers.values()
        assert s.phase_rank() == (0, 0.0, True)
    finally:
        _fresh()
    assert (r.status == 0).all()
    for b in range(B):
        ref = _oracle(L, N, 0, mu0[b], taer[b], rho[b], np.zeros(2 * N), P0r[b], kw)
        assert int(r.n[b]) == ref.n
        assert_close(r.I[b], ref.I, RTOL, "zero atmosphere, column %d" % b)
