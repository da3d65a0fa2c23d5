"""The chunk-parallel kernel's moment mode against rows of Jn, bit for bit (csrc/transport_scan_body.hpp, MOM; the records are
those of the ring kernel's mode: csrc/jn_gemm_tile.hpp, lowrank_rows with GemmArgs::mom; csrc/transport_util.hpp: lr_expand, the
one expansion every side calls).  Every case solves the same columns to tolerance on two handles of one process -- one created
with SOSRT_SCAN_MOMENTS=0, one without, both with SOSRT_TRANSPORT=scan and SOSRT_SCAN_MOMENTS_MIN=1 so that a batch of three
columns takes the chunk-parallel kernel in moment mode -- and requires the field, the order counts and the status words to be
equal bit for bit.  Every case also requires that the mode RAN: sosrt_scan_moments_stats counts the orders of the last solve whose
contraction wrote records and whose chunk-parallel launch expanded them -- every order of the two-launch loop on the second
handle, none on the first.

Optical depths and slab positions are those of tests/test_gpu_ring_moments.py: the columns start at depth 0.07, so that no
|mu| < 0.01 lane keeps its k_smallmu value (the mode stays off while one does); a slab lies strictly inside its column.  The slabs
put a zone boundary at the top rows, inside a chunk of eight rows, across a chunk boundary, around exactly one chunk, at the last
rows and around one row: the record of "the row before the chunk" is then read on both sides of a boundary, in both sweeps.

Forms: N <= 128 has the one-workgroup form (SOSRT_SCAN_SPLIT=0, and every Lambertian launch), N > 64 the split form of
ceil(N / 64) workgroups per column (specular surface or none)."""
import functools
import os

import numpy as np
import pytest
import torch

import legendre_phase as LP
import sos_oracle as O
from sosrt import _lib, inputs
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

# (L, N, split): one lane group; a ragged last chunk; whole chunks; a ragged last part; four parts -- N = 128 in both forms
FORMS = [(16, 64, False), (37, 128, False), (37, 128, True), (40, 128, False), (40, 128, True), (24, 192, True), (24, 256, True)]
RANKS = (0, 1, 2, 3, 4)
TATM = 0.124
TOP = 0.07                                                 # depth at row 0: above the first extrapolation bucket (0.0625)
# three columns, the second of which converges several orders before the others (the transport's grid comes from the live list)
MU0 = np.array([0.35, 0.9, 0.6]); TAER = np.array([0.6, 0.02, 0.6]); RHO = np.array([0.5, 0.05, 0.7])
KNOBS = ("SOSRT_SCAN_MOMENTS", "SOSRT_SCAN_MOMENTS_MIN", "SOSRT_RING_MOMENTS", "SOSRT_TRANSPORT", "SOSRT_SCAN_SPLIT", "SOSRT_GROUPS",
         "SOSRT_CONTRACT")


def _form_id(f):
    return "L%d_N%d_%s" % (f[0], f[1], "split" if f[2] else "one")


def _slabs(L):
    return {"top": (1, 3), "inside_a_chunk": (9, 11), "across_a_boundary": (6, 9), "one_chunk": (8, min(15, L - 2)),
            "bottom": (L - 4, L - 2), "one_row": (5, 5)}


@functools.lru_cache(maxsize=None)
def _phase(N, r):
    """(P_atm of r Legendre terms, P_aer (HG, not low-rank), P0_atm [3, 2N], P0_aer [3, 2N])"""
    mu = inputs.direction_grid(N)
    Pa = LP.legendre_phase(N, mu, LP.terms(r))[0]
    Pr = inputs.phase_function("hg", N, mu, 0.5, 0.7)[1]
    P0a = np.stack([LP.legendre_phase(N, mu, LP.terms(r), mu0=m)[1] for m in MU0])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in MU0])
    return Pa, Pr, P0a, P0r


def _tau(L, iu, idn, taer):
    k = np.arange(L)
    step = taer / (idn + 1 - iu)
    return TOP + k * TATM / (L - 1) + np.where(k < iu, 0.0, np.where(k <= idn, (k + 1 - iu) * step, taer))


def _solvers(L, N, B, envs, max_orders=200):
    """One handle per environment of `envs` (knobs are read when a handle is created)"""
    keep = {k: os.environ.get(k) for k in KNOBS}
    out = []
    try:
        for env in envs:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            s = Solver(L, N, max_batch=B, max_orders=max_orders)
            s.set_grid(inputs.direction_grid(N))
            out.append(s)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def _pair(L, N, B, split=True, **env):
    """(handle with rows of Jn, handle in moment mode), both transporting with the chunk-parallel kernel"""
    base = dict(SOSRT_TRANSPORT="scan", SOSRT_SCAN_MOMENTS_MIN="1", SOSRT_SCAN_SPLIT="1" if split else "0", **env)
    return _solvers(L, N, B, [dict(base, SOSRT_SCAN_MOMENTS="0"), base])


def _mode_ran(rows, mom, what):
    """The last solve of `mom` ran every order after the first in the chunk-parallel kernel's moment mode, that of `rows` none;
    neither ran an order in the ring kernel's."""
    m, r = mom.scan_moments_stats(), rows.scan_moments_stats()
    assert 0 < m[0] == m[1] and r[0] == 0 and r[1] == m[1], (what, m, r)
    assert mom.ring_moments_stats() == (0, m[1]) and rows.ring_moments_stats() == (0, m[1]), what


def _mode_off(rows, other, what):
    m, r = other.scan_moments_stats(), rows.scan_moments_stats()
    assert m[0] == 0 and r[0] == 0 and m[1] == r[1] > 0, (what, m, r)


def _same_bits(a, b, what):
    assert torch.equal(torch.from_numpy(a.n), torch.from_numpy(b.n)), (what, a.n, b.n)
    assert torch.equal(torch.from_numpy(a.status), torch.from_numpy(b.status)), what
    same = torch.equal(torch.from_numpy(a.I), torch.from_numpy(b.I))
    if not same:
        d = np.argwhere(a.I != b.I)
        print(what, "differing elements:", len(d), "first (column, row, direction):", d[0], a.I[tuple(d[0])], b.I[tuple(d[0])])
    assert same, what


def _parts(N, split, surface):
    return (N + 63) // 64 if split and surface != "lambertian" else 1


@pytest.mark.parametrize("slab", list(_slabs(16)))
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_three_zone_columns_at_every_rank_and_surface(form, slab):
    L, N, split = form
    iu, idn = _slabs(L)[slab]
    rows, mom = _pair(L, N, 3, split)
    try:
        tau = np.stack([_tau(L, iu, idn, t) for t in TAER])
        spread = 0
        for r in RANKS:
            Pa, Pr, P0a, P0r = _phase(N, r)
            for s in (rows, mom):
                s.set_phase(Pa, Pr)
            assert mom.phase_rank()[0] == r and mom.phase_rank()[2]
            # (a Lambertian launch has the one-workgroup form only: N <= 128)
            for surface in (("specular",) if split else ("specular", "lambertian")):
                res = []
                for s in (rows, mom):
                    s.set_columns(np.full(3, iu), np.full(3, idn), MU0, RHO, 1.0, 0.95, TATM / L, TAER / (idn + 1 - iu), TOP + TATM + TAER,
                                  surface=surface)
                    res.append(s.solve(tau, P0a, P0r))
                plan = mom.plan_launch(3, 3, surface=surface)
                assert plan["transport"] == _lib.PLAN_TRANSPORT_SCAN and plan["parts"] == _parts(N, split, surface), plan
                assert mom.plan_scan_moments(3, 3, surface=surface) and not rows.plan_scan_moments(3, 3, surface=surface)
                what = "L=%d N=%d split=%d slab %d-%d rank %d %s" % (L, N, split, iu, idn, r, surface)
                _mode_ran(rows, mom, what)
                # (a thick one-row slab stops a column with the reference's IndexError: the status words must agree as well)
                assert (res[0].status == _lib.COL_OK).any() and res[0].n.min() >= 2
                spread = max(spread, int(res[0].n.max() - res[0].n.min()))
                _same_bits(res[0], res[1], what)
        assert spread >= 2                                  # a column left the live list orders before the others
    finally:
        rows.close(); mom.close()


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_columns_without_a_surface_at_every_rank(form):
    """The single-slab geometry: every row plain, no surface."""
    L, N, split = form
    rows, mom = _pair(L, N, 3, split)
    try:
        tau = np.stack([np.arange(L) * t / (L - 1) for t in (0.3, 0.08, 0.8)])     # (tauStar is the reference depth: above 0.0625)
        for r in RANKS:
            Pa, _, P0a, _ = _phase(N, r)
            res = []
            for s in (rows, mom):
                s.set_phase(Pa, None)
                s.set_columns_single_slab(MU0, np.array([0.95, 0.5, 1.0]), tau[:, -1])
                res.append(s.solve(tau, P0a, None))
            what = "single slab L=%d N=%d split=%d rank %d" % (L, N, split, r)
            plan = mom.plan_launch(3, 3, surface="none", zones=1)
            assert plan["transport"] == _lib.PLAN_TRANSPORT_SCAN and plan["parts"] == _parts(N, split, "none"), plan
            _mode_ran(rows, mom, what)
            assert (res[0].status == _lib.COL_OK).all()
            _same_bits(res[0], res[1], what)
    finally:
        rows.close(); mom.close()


@pytest.mark.parametrize("split", [False, True], ids=["one", "split"])
def test_rows_whose_search_leaves_the_first_wave(split):
    """The long-blend input of tests/test_gpu_ring_moments.py (flip-symmetric, so the Rayleigh matrix keeps its symmetric low-rank
    form): the mu -> 0+ search leaves the first lane group in most orders -- rows finished one by one, and the row-by-row redo of
    the upward sweep, whose plain rows then come from the records as well (in the split form, for the other workgroup's half too)."""
    N, L = 128, 40
    mu = inputs.direction_grid(N)
    j = np.arange(N)
    c = np.ones(2 * N)
    c[N:] = np.where(j < 70, 1 + 0.3 * (-1.0) ** j, 1.0)
    c[:N] = c[N:][::-1]
    cols = [(0.6, 0.3, 0.3), (0.6, 0.9, 0.6), (0.35, 0.5, 0.45)]
    P_atm = O.phase_rayleigh(N, mu, 0.5)[1] * c[:, None]
    P_aer = O.phase_hg(N, mu, 0.5, 0.7)[1] * c[:, None]
    m0, ta, rh = (np.array(x) for x in zip(*cols))
    P0a = np.stack([O.phase_rayleigh(N, mu, m)[0] for m in m0])
    P0r = np.stack([O.phase_hg(N, mu, m, 0.7)[0] for m in m0])
    iu, idn = inputs.slab_indices(120, 40, 12, L)
    tau = np.stack([inputs.tau_profile(TATM, t, 120, 40, 12, L) for t in ta])
    rows, mom = _pair(L, N, 3, split)
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(P_atm, P_aer)
            s.set_columns(np.full(3, iu), np.full(3, idn), m0, rh, 1.0, 0.95, TATM / L, ta / (idn + 1 - iu), TATM + ta)
            res.append(s.solve(tau, P0a, P0r))
        assert mom.phase_rank()[2] and mom.phase_asymmetry()[1]
        assert mom.plan_launch(3, 3)["parts"] == (2 if split else 1)
        _mode_ran(rows, mom, "long blends")                 # (reference depths: 0.079 above the slab, more inside it)
    finally:
        rows.close(); mom.close()
    assert (res[0].status == _lib.COL_OK).all()
    _same_bits(res[0], res[1], "long blends")
    col = O.make_column(cols[0][0], 120, 40, 12, L, TATM, cols[0][1], cols[0][2], 1.0, 0.95, N, P0a[0], P_atm, P0r[0], P_aer)
    ref = O.solve_column(col, literal=False)
    assert res[1].n[0] == ref.n
    long_blends = sum(int(np.argmax(np.abs(np.diff(In[L // 2, N:], 2)) > 1e-12)) + 1 > 64 for In in ref.I_saved)
    assert long_blends >= 3


def test_the_default_plan_runs_every_order_in_one_of_the_two_modes():
    """260 columns at L = 16, N = 64 in one column group with the default transport policy: the ring kernel with records while
    more than 200 columns are live, the chunk-parallel kernel with records after that.  Against both knobs off; and with
    SOSRT_SCAN_MOMENTS_MIN=128 the chunk-parallel kernel goes back to rows of Jn below 128 live columns, with the same bits."""
    L, N, B = 16, 64, 260
    rng = np.random.default_rng(260)
    mu = inputs.direction_grid(N)
    mu0 = rng.uniform(0.2, 1.0, B); taer = rng.choice([0.02, 0.12, 0.6], B); rho = rng.uniform(0.0, 0.8, B)
    Pa = LP.legendre_phase(N, mu, LP.terms(2))[0]
    Pr = inputs.phase_function("hg", N, mu, 0.5, 0.7)[1]
    P0a = np.stack([LP.legendre_phase(N, mu, LP.terms(2), mu0=m)[1] for m in mu0])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in mu0])
    iu, idn = 6, 9
    tau = np.stack([_tau(L, iu, idn, t) for t in taer])
    names = ("default", "rows", "min128")
    envs = [dict(SOSRT_GROUPS="1", SOSRT_SCAN_MOMENTS_MIN="1"), dict(SOSRT_GROUPS="1", SOSRT_RING_MOMENTS="0", SOSRT_SCAN_MOMENTS="0"),
            dict(SOSRT_GROUPS="1", SOSRT_SCAN_MOMENTS_MIN="128")]
    solvers = _solvers(L, N, B, envs)
    res = {}
    try:
        for name, s in zip(names, solvers):
            s.set_phase(Pa, Pr)
            s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.95, TATM / L, taer / (idn + 1 - iu), TOP + TATM + taer)
            res[name] = s.solve(tau, P0a, P0r)
            ring, scan = s.ring_moments_stats(), s.scan_moments_stats()
            assert s.plan_launch(B, B)["groups"] == 1 and ring[1] == scan[1] > 0
            assert [s.plan_ring_moments(B, live) for live in (260, 201, 200)] == ([True, True, False] if name != "rows" else [False] * 3)
            if name == "default":
                # (N = 64 has no |mu| < 0.01 lane) both regimes ran, and between them every order after the first
                assert 0 < ring[0] and 0 < scan[0] and ring[0] + scan[0] == ring[1], (ring, scan)
                assert [s.plan_scan_moments(B, live) for live in (260, 201, 200, 127, 1)] == [False, False, True, True, True]
            elif name == "rows":
                assert ring[0] == 0 and scan[0] == 0
            else:
                assert 0 < ring[0] and 0 < scan[0] and ring[0] + scan[0] < ring[1], (ring, scan)
                assert [s.plan_scan_moments(B, live) for live in (201, 200, 128, 127, 1)] == [False, True, True, False, False]
    finally:
        for s in solvers:
            s.close()
    n = res["default"].n
    assert (res["default"].status == _lib.COL_OK).all()
    # every regime ran: every column was live for some orders, fewer than 128 were for the last ones
    assert n.min() >= 3 and np.sum(n == n.max()) < 128
    _same_bits(res["rows"], res["default"], "default plan against rows of Jn")
    _same_bits(res["rows"], res["min128"], "records down to 128 live columns against rows of Jn")


def _three_zone_inputs(L, N, r=2):
    iu, idn = 6, 9
    Pa, Pr, P0a, P0r = _phase(N, r)
    tau = np.stack([_tau(L, iu, idn, t) for t in TAER])
    cols = (np.full(3, iu), np.full(3, idn), MU0, RHO, 1.0, 0.95, TATM / L, TAER / (idn + 1 - iu), TOP + TATM + TAER)
    return Pa, Pr, P0a, P0r, tau, cols


def test_saved_orders_keep_rows_of_Jn():
    L, N = 16, 64
    Pa, Pr, P0a, P0r, tau, cols = _three_zone_inputs(L, N)
    rows, mom = _pair(L, N, 3, False)
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(Pa, Pr); s.set_columns(*cols)
            # (two solves: one for the order counts, which runs in moment mode on `mom`, then the one that saves)
            res.append(s.solve(tau, P0a, P0r, save_orders=True))
        assert mom.plan_scan_moments(3, 3) and not mom.plan_scan_moments(3, 3, saved_orders=True)
        _mode_off(rows, mom, "saved orders")
        _same_bits(res[0], res[1], "saved orders")
        assert torch.equal(torch.from_numpy(np.asarray(res[0].I_saved)), torch.from_numpy(np.asarray(res[1].I_saved)))
        # ... and the mode is back for the next solve of the same handle, with the same field
        plain = mom.solve(tau, P0a, P0r)
        assert 0 < mom.scan_moments_stats()[0] == mom.scan_moments_stats()[1]
        _same_bits(res[0], plain, "after saved orders")
    finally:
        rows.close(); mom.close()


def test_the_full_contraction_keeps_rows_of_Jn():
    L, N = 16, 64
    Pa, Pr, P0a, P0r, tau, cols = _three_zone_inputs(L, N)
    rows, mom = _pair(L, N, 3, False, SOSRT_CONTRACT="full")
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(Pa, Pr); s.set_columns(*cols)
            res.append(s.solve(tau, P0a, P0r))
        assert mom.phase_rank()[0] == 2 and not mom.phase_rank()[2] and not mom.plan_scan_moments(3, 3)
        _mode_off(rows, mom, "full contraction")
        _same_bits(res[0], res[1], "full contraction")
    finally:
        rows.close(); mom.close()


def test_atmosphere_sets_keep_rows_of_Jn():
    L, N = 16, 64
    Pa, Pr, P0a, P0r, tau, cols = _three_zone_inputs(L, N)
    Pa3 = _phase(N, 3)[0]
    rows, mom = _pair(L, N, 3, False)
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(Pa, Pr); s.set_atm_phase_sets(np.stack([Pa, Pa3])); s.set_columns(*cols); s.set_atmosphere_sets([0, 1, 0])
            res.append(s.solve(tau, P0a, P0r))
        assert not mom.plan_scan_moments(3, 3)
        _mode_off(rows, mom, "atmosphere sets")
        assert (res[0].status == _lib.COL_OK).all()
        _same_bits(res[0], res[1], "atmosphere sets")
    finally:
        rows.close(); mom.close()


def test_a_five_zone_column_keeps_rows_of_Jn():
    """The batch of tests/transport_launch_cases.py: zones_run -- a five-zone column between two three-zone ones."""
    L, N = 48, 64
    mu = inputs.direction_grid(N)
    P0a, Pa = inputs.phase_function("rayleigh", N, mu, 0.6)
    P0r, Pr = inputs.phase_function("hg", N, mu, 0.6, 0.7)
    tau1, r1, mix1, dta1 = inputs.tau_profile_slabs(0.124, [(25, 17, 0.3)], 120, L)
    c2 = O.make_column_slabs(0.6, 120, [(60, 50, 0.2, 0.90), (25, 17, 0.4, 0.97)], L, 0.124, 0.3, 1.0, N, P0a, Pa, P0r, Pr)
    nzmax = len(c2.zones)
    assert nzmax == 5 and len(r1) == 3

    def pad(x, fill=0):
        return list(x) + [fill] * (nzmax - len(x))

    wr1 = pad([0.95 if m else 0.0 for m in mix1])
    zr0 = np.array([pad(r1), [z.r0 for z in c2.zones], pad(r1)], dtype=np.int32)
    zmix = np.array([pad(mix1), [z.kind == "mix" for z in c2.zones], pad(mix1)], dtype=np.int32)
    zwr = np.array([wr1, [z.alb_aer for z in c2.zones], wr1])
    zdt = np.array([pad(dta1), [z.dtau_aer for z in c2.zones], pad(dta1)])
    rows, mom = _pair(L, N, 3, False)
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(Pa, Pr)
            s.set_columns_zones(zr0, zmix, 0.6, [0.1, c2.grd_alb, 0.5], 1.0, 0.124 / L, zwr, zdt, [0.424, c2.tauStar_tot, 0.424], nz=[3, 5, 3])
            res.append(s.solve(np.stack([tau1, c2.tau, tau1]), np.tile(P0a, (3, 1)), np.tile(P0r, (3, 1))))
        assert mom.phase_rank()[2] and mom.plan_scan_moments(3, 3, zones=3) and not mom.plan_scan_moments(3, 3, zones=5)
        _mode_off(rows, mom, "five zones")
        assert (res[0].status == _lib.COL_OK).all()
        _same_bits(res[0], res[1], "five zones")
    finally:
        rows.close(); mom.close()
