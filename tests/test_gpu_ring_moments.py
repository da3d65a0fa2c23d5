"""The ring kernel's moment mode against rows of Jn, bit for bit (csrc/transport_ring.hip, MOM; csrc/jn_gemm_tile.hpp:
lowrank_rows with GemmArgs::mom; csrc/transport_util.hpp: lr_expand, the one expansion both sides call).  Every case solves the
same columns to tolerance on two handles of one process -- one created with SOSRT_RING_MOMENTS=0, one without, both with
SOSRT_TRANSPORT=ring so that a batch of three columns takes the ring kernel -- and requires the field, the order counts and the
status words to be equal bit for bit.  Every case also requires that the mode RAN: sosrt_ring_moments_stats counts the orders
of the last solve whose contraction wrote records and whose ring launch expanded them -- more than none on the second handle,
none on the first.  (The plan query alone would not do: it answers for a plan, and a solve also keeps the mode off while some
|mu| < 0.01 lane keeps its k_smallmu value -- at N = 128 and 256 whenever a zone's reference depth is at most 0.0625, I1_In:124.)

Optical depths: every zone's reference depth (the depth at the last row of the top zone and of the slab) must lie above 0.0625 for
that, also where the slab starts at row 1.  So the columns start at depth TOP = 0.07 -- below an absorbing layer that is not part
of the column -- instead of at 0; all depths stay below 1, the next bucket's end.

Slab positions: a slab lies strictly inside its column (1 <= idx_up, idx_down <= L - 2: sosrt_set_columns refuses anything else),
so "the top rows" are rows 1-3, "the last rows" are rows L-4 .. L-2, and "exactly one chunk" ends at row L-2 where L = 16."""
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

SHAPES = [(16, 64), (37, 128), (40, 128), (24, 256)]      # one computing wave; ragged last chunk; whole chunks; two pieces per half row
RANKS = (0, 1, 2, 3, 4)
TATM = 0.124
TOP = 0.07                                                 # depth at row 0: above the first extrapolation bucket (0.0625)
# three columns, the second of which converges several orders before the others (the transport's grid comes from the live list)
MU0 = np.array([0.35, 0.9, 0.6]); TAER = np.array([0.6, 0.02, 0.6]); RHO = np.array([0.5, 0.05, 0.7])


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


def _pair(L, N, B, **env):
    """(handle with rows of Jn, handle in moment mode): knobs are read when a handle is created"""
    keep = {k: os.environ.get(k) for k in ("SOSRT_RING_MOMENTS", "SOSRT_TRANSPORT", "SOSRT_GROUPS")}
    out = []
    try:
        for moments in ("0", None):
            os.environ.pop("SOSRT_RING_MOMENTS", None)
            os.environ["SOSRT_TRANSPORT"] = "ring"
            os.environ.update(env)
            if moments is not None:
                os.environ["SOSRT_RING_MOMENTS"] = moments
            s = Solver(L, N, max_batch=B, max_orders=200)
            s.set_grid(inputs.direction_grid(N))
            out.append(s)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def _mode_ran(rows, mom, what):
    """The last solve of `mom` ran every order after the first in moment mode, that of `rows` none.  (Every order: with
    SOSRT_TRANSPORT=ring the ring kernel transports each of them, and the device's verdict that no |mu| < 0.01 lane keeps its
    k_smallmu value is there before the second order is planned.)"""
    m, r = mom.ring_moments_stats(), rows.ring_moments_stats()
    assert 0 < m[0] == m[1] and r[0] == 0 and r[1] == m[1], (what, m, r)


def _same_bits(a, b, what):
    assert torch.equal(torch.from_numpy(a.n), torch.from_numpy(b.n)), (what, a.n, b.n)
    assert torch.equal(torch.from_numpy(a.status), torch.from_numpy(b.status)), what
    same = torch.equal(torch.from_numpy(a.I), torch.from_numpy(b.I))
    if not same:
        d = np.argwhere(a.I != b.I)
        print(what, "differing elements:", len(d), "first (column, row, direction):", d[0], a.I[tuple(d[0])], b.I[tuple(d[0])])
    assert same, what


@pytest.mark.parametrize("slab", list(_slabs(16)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d_N%d" % s)
def test_three_zone_columns_at_every_rank_and_surface(shape, slab):
    L, N = shape
    iu, idn = _slabs(L)[slab]
    rows, mom = _pair(L, N, 3)
    try:
        tau = np.stack([_tau(L, iu, idn, t) for t in TAER])
        spread = 0
        for r in RANKS:
            Pa, Pr, P0a, P0r = _phase(N, r)
            for s in (rows, mom):
                s.set_phase(Pa, Pr)
            assert mom.phase_rank()[0] == r and mom.phase_rank()[2]
            for surface in ("specular", "lambertian"):
                res = []
                for s in (rows, mom):
                    s.set_columns(np.full(3, iu), np.full(3, idn), MU0, RHO, 1.0, 0.95, TATM / L, TAER / (idn + 1 - iu), TOP + TATM + TAER,
                                  surface=surface)
                    res.append(s.solve(tau, P0a, P0r))
                assert mom.plan_launch(3, 3, surface=surface)["transport"] == _lib.PLAN_TRANSPORT_RING
                what = "L=%d N=%d slab %d-%d rank %d %s" % (L, N, iu, idn, r, surface)
                _mode_ran(rows, mom, what)
                # (a thick one-row slab stops a column with the reference's IndexError: the status words must agree as well)
                assert (res[0].status == _lib.COL_OK).any() and res[0].n.min() >= 2
                spread = max(spread, int(res[0].n.max() - res[0].n.min()))
                _same_bits(res[0], res[1], what)
        assert spread >= 2                                  # a column left the live list orders before the others
    finally:
        rows.close(); mom.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d_N%d" % s)
def test_columns_without_a_surface_at_every_rank(shape):
    """The single-slab geometry: every row plain, no surface, no seam barrier."""
    L, N = shape
    rows, mom = _pair(L, N, 3)
    try:
        tau = np.stack([np.arange(L) * t / (L - 1) for t in (0.3, 0.08, 0.8)])     # (tauStar is the reference depth: above 0.0625)
        for r in RANKS:
            Pa, _, P0a, _ = _phase(N, r)
            res = []
            for s in (rows, mom):
                s.set_phase(Pa, None)
                s.set_columns_single_slab(MU0, np.array([0.95, 0.5, 1.0]), tau[:, -1])
                res.append(s.solve(tau, P0a, None))
            _mode_ran(rows, mom, "single slab L=%d N=%d rank %d" % (L, N, r))
            assert (res[0].status == _lib.COL_OK).all()
            _same_bits(res[0], res[1], "single slab L=%d N=%d rank %d" % (L, N, r))
    finally:
        rows.close(); mom.close()


def test_rows_whose_search_leaves_the_first_wave():
    """The input of tests/test_gpu_parity.py::test_split_scan_redo_reads_the_other_halfs_rows_fresh made flip-symmetric (the
    oscillation over the first 70 upward directions mirrored onto the last 70 downward ones), so that the Rayleigh matrix keeps
    its symmetric low-rank form: the mu -> 0+ search leaves wave 0 in most orders -- rows finished one by one, and the row-by-row
    redo of the upward sweep, whose plain rows then come from the records as well.  The oracle says that the blends are long."""
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
    rows, mom = _pair(L, N, 3)
    try:
        res = []
        for s in (rows, mom):
            s.set_phase(P_atm, P_aer)
            s.set_columns(np.full(3, iu), np.full(3, idn), m0, rh, 1.0, 0.95, TATM / L, ta / (idn + 1 - iu), TATM + ta)
            res.append(s.solve(tau, P0a, P0r))
        assert mom.phase_rank()[2] and mom.phase_asymmetry()[1]
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


def test_the_default_plan_goes_from_records_to_rows_as_columns_converge():
    """260 columns at L = 16, N = 64 in one column group with the default transport policy: the ring kernel with records while
    more than 200 columns are live (the dense tiling of the contraction, then the tiles over the live columns), the
    chunk-parallel kernel with rows of Jn after that.  Against SOSRT_RING_MOMENTS=0 and against SOSRT_TRANSPORT=scan."""
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
    keep = {k: os.environ.get(k) for k in ("SOSRT_RING_MOMENTS", "SOSRT_TRANSPORT", "SOSRT_GROUPS")}
    res = {}
    try:
        for name, env in (("default", {}), ("rows", {"SOSRT_RING_MOMENTS": "0"}), ("scan", {"SOSRT_TRANSPORT": "scan"})):
            for k in keep:
                os.environ.pop(k, None)
            os.environ["SOSRT_GROUPS"] = "1"
            os.environ.update(env)
            s = Solver(L, N, max_batch=B, max_orders=200)
            try:
                s.set_grid(mu); s.set_phase(Pa, Pr)
                s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.95, TATM / L, taer / (idn + 1 - iu), TOP + TATM + taer)
                res[name] = s.solve(tau, P0a, P0r)
                ring = [s.plan_launch(B, live)["transport"] == _lib.PLAN_TRANSPORT_RING for live in (260, 201, 200)]
                moments = [s.plan_ring_moments(B, live) for live in (260, 201, 200)]
                ran = s.ring_moments_stats()
                # (N = 64 has no |mu| < 0.01 lane) records while the ring kernel ran, rows of Jn after that: both in this solve
                assert (0 < ran[0] < ran[1]) if name == "default" else ran[0] == 0, (name, ran)
                assert s.plan_launch(B, B)["groups"] == 1
                assert ring == ([True, True, False] if name != "scan" else [False] * 3), (name, ring)
                assert moments == ([True, True, False] if name == "default" else [False] * 3), (name, moments)
            finally:
                s.close()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    n = res["default"].n
    assert (res["default"].status == _lib.COL_OK).all()
    # both regimes ran: every column was live for some orders, and at most 200 were for the last ones
    assert n.min() >= 3 and np.sum(n == n.max()) <= 200 and 0 < np.sum(n >= n.max() - 1)
    _same_bits(res["rows"], res["default"], "default plan against rows of Jn")
    _same_bits(res["scan"], res["default"], "default plan against the chunk-parallel kernel")
