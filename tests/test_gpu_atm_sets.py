"""Several ATMOSPHERE phase matrices in one batch (sosrt_set_atm_phase_sets / sosrt_set_atmosphere_sets):
a column on set s against the same column on a handle whose set_phase got that set's pair -- bit for bit, in every tiling of
the contraction -- the rank-0 set, the combinations that are refused, and the reset by set_columns."""
import numpy as np
import pytest
import torch

from sosrt import _lib, inputs
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

NMODES = 6                                   # Rayleigh modes 0..5: ranks 2, 1, 1, 0, 0, 0


def _solver(L, N, B, max_orders=64):
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(inputs.direction_grid(N))
    return s


def _columns(s, L, mu0, taer, k=1, surface="specular"):
    """The three-zone columns (mu0, taer) k times over (column index (set, b)); returns their tau [k B, L]."""
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    t = lambda v: np.tile(np.asarray(v, dtype=np.float64), k)
    B = k * len(mu0)
    s.set_columns(np.full(B, iu), np.full(B, idn), t(mu0), 0.15, 1.0, 0.95, 0.124 / L, t(taer) / (idn + 1 - iu),
                  0.124 + t(taer), surface=surface)
    return np.stack([inputs.tau_profile(0.124, x, 120, 25, 17, L) for x in t(taer)])


def _signed_modes(s, mu0, nm=NMODES):
    """(-1)^m P^m and P0^m, m = 0..nm-1, of Rayleigh and HG(0.7): (P_atm [nm, D, D], P0_atm [nm, B, D], P_aer, P0_aer)"""
    sgn = np.where(np.arange(nm) & 1, -1.0, 1.0)[:, None, None]
    out = []
    for kind, g in (("rayleigh", 0.0), ("hg", 0.7)):
        out += [sgn * s.phase_modes(kind, 0, nm, 25, g), s.phase_p0_modes(kind, mu0, 0, nm, 25, g)]
    return out[0], out[1], out[2], out[3]


def _solve(s, tau, P0a, P0r, targets=None, tol=1e-4):
    """solve_device with fixed order counts (targets) or the convergence test: (I, n, status)"""
    dev = torch.device("cuda", 0)
    B = tau.shape[0]
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_tau, d_a, d_r = up(tau), up(P0a), up(P0r)
    d_t = None if targets is None else up(targets, np.int32)
    I = torch.empty((B, s.L, s.D), dtype=torch.float64, device=dev)
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.set_order_targets(None if d_t is None else d_t.data_ptr())
    try:
        s.solve_device(d_tau.data_ptr(), d_a.data_ptr(), d_r.data_ptr(), I.data_ptr(), tol=tol, d_n_orders=n.data_ptr(),
                       d_status=st.data_ptr())
        s.synchronize()
    finally:
        s.set_order_targets(None)
    return I.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def _set_by_set(L, N, mu0, taer, nm):
    """The reference: nm solves of the B columns on a handle whose set_phase got set m's pair, with the order counts of the
    mode-0 solve as targets.  Returns (the modes' arrays, targets, I [nm, B, L, D], n, status)."""
    B = len(mu0)
    h = _solver(L, N, B)
    tau = _columns(h, L, mu0, taer)
    Pa, P0a, Pr, P0r = _signed_modes(h, mu0, nm)
    h.set_phase(Pa[0], Pr[0])
    targets = h.solve(tau, P0a[0], P0r[0], tol=1e-4).n
    assert targets.max() > targets.min() and targets.min() >= 2
    res = []
    for m in range(nm):
        h.set_phase(Pa[m], Pr[m])
        assert h.phase_rank()[0] == (2, 1, 1, 0, 0, 0)[m]
        res.append(_solve(h, tau, P0a[m], P0r[m], targets))
    h.close()
    return (Pa, P0a, Pr, P0r), targets, [np.stack([r[i] for r in res]) for i in range(3)]


def _in_one_batch(s, L, mu0, taer, modes, targets, nm):
    """The same columns as one batch of nm B columns, column (m, b) on atmosphere set m and aerosol set m."""
    Pa, P0a, Pr, P0r = modes
    B = len(mu0)
    tau = _columns(s, L, mu0, taer, k=nm)
    s.set_phase_sets(Pa[0], Pr[:nm])
    s.set_atm_phase_sets(Pa[:nm])
    sets = np.repeat(np.arange(nm, dtype=np.int32), B)
    s.set_aerosol_sets(sets)
    s.set_atmosphere_sets(sets)
    assert s.atm_sets_info() == {"sets": nm, "in_use": True}
    I, n, st = _solve(s, tau, P0a[:nm].reshape(nm * B, -1), P0r[:nm].reshape(nm * B, -1), np.tile(targets, nm))
    return I.reshape(nm, B, L, -1), n.reshape(nm, B), st.reshape(nm, B)


# ---- 1: bits of a set alone ------------------------------------------------------------------
@pytest.mark.parametrize("L,N", [(50, 37), (60, 64)])
def test_a_column_on_a_set_has_the_bits_of_that_set_alone(L, N):
    """Modes 0..5 of Rayleigh + HG(0.7) as 6 atmosphere and 6 aerosol sets, 3 columns each: 18 columns in (m, b) order against six
    solves of 3 columns.  (50, 37): odd N, 2N = 74 is no multiple of the 128-element lane stride and L no multiple of the four
    rows a wave takes, so a wave's rows straddle columns of different sets in the dense row list."""
    mu0, taer = np.array([0.3, 0.6, 0.9]), np.array([0.1, 0.3, 0.2])
    modes, targets, (I_ref, n_ref, st_ref) = _set_by_set(L, N, mu0, taer, NMODES)
    s = _solver(L, N, NMODES * len(mu0))
    I, n, st = _in_one_batch(s, L, mu0, taer, modes, targets, NMODES)
    s.close()
    assert np.array_equal(n, n_ref) and np.array_equal(st, st_ref) and (st == 0).all()
    for m in range(NMODES):
        for b in range(len(mu0)):
            assert np.array_equal(I[m, b], I_ref[m, b]), (m, b)
    assert np.any(I[1]) and np.any(I[2]) and np.any(I[5])        # (the aerosol keeps the vanishing Rayleigh modes alive)


# ---- 2: every tiling -------------------------------------------------------------------------
_TILING_REF = {}


@pytest.mark.parametrize("knobs", ["default", "staged", "dense"])
def test_every_tiling_reads_the_set_of_a_column(knobs, monkeypatch):
    """60 columns (5 sets x 12) at L = 200, N = 128, two column groups of 30: by default the register tile (16 rows) once 13
    columns of a group are live and the deep staged tile before; SOSRT_GEMM_REGS=0: the staged 32-row live-column tiles; SOSRT_GEMM_SMALL=8 on top: the dense tiling first, then the
    64-row live-column tiles -- asserted through plan_launch.  The set-by-set reference is computed once."""
    L, N, nm, C = 200, 128, 5, 12
    rng = np.random.default_rng(3)
    mu0, taer = rng.uniform(0.2, 1.0, C), rng.choice([0.05, 0.12, 0.3], C)
    if not _TILING_REF:
        _TILING_REF["ref"] = _set_by_set(L, N, mu0, taer, nm)
    modes, targets, (I_ref, n_ref, st_ref) = _TILING_REF["ref"]
    if knobs != "default":
        monkeypatch.setenv("SOSRT_GEMM_REGS", "0")
    if knobs == "dense":
        monkeypatch.setenv("SOSRT_GEMM_SMALL", "8")
    B = nm * C
    s = _solver(L, N, B)
    I, n, st = _in_one_batch(s, L, mu0, taer, modes, targets, nm)
    gemms = {s.plan_launch(B, live)["gemm"] for live in (30, 20, 10, 2, 1)}
    if knobs == "dense":
        assert s.plan_launch(B, 30)["gemm"] == _lib.PLAN_GEMM_DENSE and _lib.PLAN_GEMM_LIVE64 in gemms
    elif knobs == "staged":
        assert gemms <= {_lib.PLAN_GEMM_LIVE32, _lib.PLAN_GEMM_LIVE32_DEEP}
    else:
        # (at this shape the register tile takes a group's last 13 live columns, the deep staged tile the orders before)
        assert _lib.PLAN_GEMM_LIVE16_REGS in gemms and gemms <= {_lib.PLAN_GEMM_LIVE16_REGS, _lib.PLAN_GEMM_LIVE32_DEEP}
        assert s.plan_launch(B, 10)["gemm"] == s.plan_launch(B, 1)["gemm"] == _lib.PLAN_GEMM_LIVE16_REGS
    s.close()
    assert np.array_equal(n, n_ref) and np.array_equal(st, st_ref) and (st == 0).all()
    assert np.array_equal(I, I_ref)


# ---- 3: a set of rank 0 ----------------------------------------------------------------------
def test_isotropic_atmosphere_and_a_zero_set():
    """Set 0 isotropic (rank 1), set 1 an all-zero matrix (rank 0): the plain rows of sosrt_source of a column on set 1 are
    exactly 0.0, its slab rows those of a handle with that pair; the column on set 0 is the handle's with the isotropic pair."""
    L, N = 50, 37
    mu0, taer = np.array([0.5, 0.5]), np.array([0.2, 0.2])
    s = _solver(L, N, 2)
    _columns(s, L, mu0, taer)
    Piso, Pr = s.phase_matrix("iso"), s.phase_matrix("hg", 0.7)
    stack = np.stack([Piso, np.zeros_like(Piso)])
    s.set_phase(Piso, Pr)
    assert s.phase_rank()[0] == 1
    s.set_atm_phase_sets(stack)
    s.set_atmosphere_sets(np.array([0, 1], dtype=np.int32))
    In_1 = np.random.default_rng(0).uniform(0.1, 1.0, (2, L, 2 * N))
    J = s.source(In_1)
    s.close()
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    plain = np.r_[0:iu, idn + 1:L]
    assert np.all(J[1][plain] == 0.0)
    assert np.any(J[1][iu:idn + 1]) and np.all(J[0] != 0.0)
    for k in range(2):
        h = _solver(L, N, 2)
        _columns(h, L, mu0, taer)
        h.set_phase(stack[k], Pr)
        assert h.phase_rank()[0] == 1 - k
        assert np.array_equal(h.source(In_1)[k], J[k]), k
        h.close()


# ---- 4: refusals -----------------------------------------------------------------------------
def _pair(s, mu0):
    """Two atmosphere sets a convergence test works with: Rayleigh and isotropic; (stack, P0_atm of a batch on sets 0, 1, ...)"""
    stack = np.stack([s.phase_matrix("rayleigh"), s.phase_matrix("iso")])
    return stack, s.phase_p0("rayleigh", mu0), s.phase_p0("iso", mu0)


def test_refusals_leave_the_handle_as_it_was(monkeypatch):
    L, N, B = 60, 64, 4
    mu0, taer = np.array([0.3, 0.5, 0.7, 0.9]), np.array([0.1, 0.3, 0.1, 0.3])
    s = _solver(L, N, B)
    tau = _columns(s, L, mu0, taer)
    stack, P0ray, P0iso = _pair(s, mu0)
    Pr, P0r = s.phase_matrix("hg", 0.7), s.phase_p0("hg", mu0, 0.7)
    s.set_phase(stack[0], Pr)
    before = s.solve(tau, P0ray, P0r)

    def unchanged():
        r = s.solve(tau, P0ray, P0r)
        assert np.array_equal(r.I, before.I) and np.array_equal(r.n, before.n) and np.array_equal(r.status, before.status)
        assert not s.atm_sets_info()["in_use"]

    with pytest.raises(ValueError, match="not low-rank"):
        s.set_atm_phase_sets(np.stack([stack[0], Pr]))                       # HG(0.7) is no low-rank matrix
    unchanged()
    bad = stack.copy()
    bad[1, 3, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        s.set_atm_phase_sets(bad)
    bad[1, 3, 5] = np.inf
    with pytest.raises(ValueError):
        s.set_atm_phase_sets(bad)
    with pytest.raises(ValueError, match="outside"):
        s.set_atm_phase_sets(np.repeat(stack[:1], _lib.MAX_PHASE_SETS + 1, axis=0))
    assert s.atm_sets_info()["sets"] == 1
    unchanged()
    s.set_atm_phase_sets(stack)
    assert s.atm_sets_info() == {"sets": 2, "in_use": False}
    for wrong in ([0, 2, 0, 1], [0, -1, 0, 1]):
        with pytest.raises(ValueError, match="outside"):
            s.set_atmosphere_sets(np.array(wrong, dtype=np.int32))
    unchanged()
    # the other contractions, in either order with the sets
    for mode in ("f64_dense", "f64_full", "f32"):
        with pytest.raises(ValueError, match="atmosphere"):
            s.set_contraction(mode)
    unchanged()
    s.set_phase(stack[0], Pr)                                                # (one atmosphere set again)
    for mode in ("f64_dense", "f64_full", "f32"):
        s.set_contraction(mode)
        with pytest.raises(ValueError, match="SOSRT_CONTRACT_F64"):
            s.set_atm_phase_sets(stack)
        s.set_atm_phase_sets(stack[:1])                                      # (one set is set_phase's W_atm: allowed)
    s.set_contraction("f64")
    unchanged()
    # the README first order, in either order
    _columns(s, L, mu0, taer, surface="lambertian_readme")
    s.set_first_order("readme")
    with pytest.raises(ValueError, match="README"):
        s.set_atm_phase_sets(stack)
    s.set_first_order("coded")
    s.set_atm_phase_sets(stack)
    with pytest.raises(ValueError, match="README"):
        s.set_first_order("readme")
    _columns(s, L, mu0, taer)
    unchanged()
    # sets in use: the order-loop launch is not planned, set_phase is refused until the columns are reset
    sets = np.array([0, 1, 1, 0], dtype=np.int32)
    s.set_atmosphere_sets(sets)
    P0a = np.where(sets[:, None] == 1, P0iso, P0ray)
    s.set_order_loop(1)
    r = s.solve(tau, P0a, P0r)
    assert s.order_loop_stats()[0] == 0 and (r.status == 0).all()
    s.set_order_loop(0)
    r0 = s.solve(tau, P0a, P0r)
    assert np.array_equal(r0.I, r.I) and np.array_equal(r0.n, r.n)
    assert np.array_equal(r.I[[0, 3]], before.I[[0, 3]]) and not np.array_equal(r.I[1], before.I[1])
    with pytest.raises(ValueError, match="use atmosphere set 1"):
        s.set_phase(stack[0], Pr)
    with pytest.raises(ValueError, match="use atmosphere set 1"):
        s.set_atm_phase_sets(stack[:1])
    with pytest.raises(ValueError, match="atmosphere"):
        s.set_contraction("f64_dense")
    _columns(s, L, mu0, taer)
    s.set_phase(stack[0], Pr)
    unchanged()
    s.close()
    # a cache of one combined matrix (SOSRT_MIX_GROUPS=1) and two groups: the two-pass form is not available with sets
    monkeypatch.setenv("SOSRT_MIX_GROUPS", "1")
    s = _solver(L, N, 2)
    tau2 = _columns(s, L, mu0[:2], taer[[0, 0]])
    s.set_phase(stack[0], Pr)
    assert s.phase_sets_info()["group_cap"] == 1 and s.phase_sets_info()["single_pass"]
    b2 = s.solve(tau2, P0ray[:2], P0r[:2])
    s.set_atm_phase_sets(stack)
    with pytest.raises(ValueError, match="two-pass"):
        s.set_atmosphere_sets(np.array([0, 1], dtype=np.int32))
    assert not s.atm_sets_info()["in_use"] and s.phase_sets_info()["single_pass"]
    r2 = s.solve(tau2, P0ray[:2], P0r[:2])
    assert np.array_equal(r2.I, b2.I) and np.array_equal(r2.n, b2.n)
    s.set_atmosphere_sets(np.array([1, 1], dtype=np.int32))                  # (one group: fits)
    assert s.atm_sets_info()["in_use"]
    s.close()


# ---- 5: reset --------------------------------------------------------------------------------
def test_set_columns_puts_every_column_back_on_set_zero():
    L, N, B = 60, 64, 4
    mu0, taer = np.array([0.3, 0.5, 0.7, 0.9]), np.array([0.1, 0.3, 0.1, 0.3])
    res = []
    for used in (True, False):
        s = _solver(L, N, B)
        tau = _columns(s, L, mu0, taer)
        stack, P0ray, _ = _pair(s, mu0)
        Pr, P0r = s.phase_matrix("hg", 0.7), s.phase_p0("hg", mu0, 0.7)
        s.set_phase(stack[0], Pr)
        if used:
            s.set_atm_phase_sets(stack)
            s.set_atmosphere_sets(np.array([1, 0, 1, 1], dtype=np.int32))
            assert s.atm_sets_info()["in_use"]
            tau = _columns(s, L, mu0, taer)
            assert s.atm_sets_info() == {"sets": 2, "in_use": False}
        res.append(s.solve(tau, P0ray, P0r))
        s.close()
    assert np.array_equal(res[0].I, res[1].I) and np.array_equal(res[0].n, res[1].n)
    assert np.array_equal(res[0].status, res[1].status) and (res[0].status == 0).all()
