"""Azimuth-resolved radiance on the device: the Fourier-mode builders against the azimuth-averaged ones and
the NumPy restatement (tests/azimuth_np.py), fixed order counts in the order loop (sosrt_set_order_targets), mode solves
against the oracle driven with the mode matrices, the synthesized first order against its closed form, and the invariants
of SOS_Aer_batch(..., azimuths=...)."""
import numpy as np
import pytest
import torch

import azimuth_np as A
import sos_oracle as O
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from sosrt.solver import Solver
from util import RTOL

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):
    """max |a - b| / max |b|: the modes m >= 1 of a field cross zero, so an element-wise relative error means nothing there."""
    assert not np.isnan(a).any(), "%s has NaN" % what
    e = np.max(np.abs(a - b)) / np.max(np.abs(b))
    assert e <= tol, "%s: error %.3e > %.1e of the field maximum" % (what, e, tol)


def _solver(L, N, B=1, max_orders=64):
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(inputs.direction_grid(N))
    return s


def _kind(s, name, g=0.0):
    """(device kind, NumPy p) of a named phase function; sets the handle's table for the tabulated ones."""
    if name == "iso":
        return "iso", (lambda c: np.ones_like(c))
    fn, (kind, tab) = inputs._scalar_phase(name, g)
    if tab is not None:
        s.set_phase_table(*tab)
    return kind, fn


# ---- 1-3: builders ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,g", [("rayleigh", 0.0), ("hg", 0.7), ("fwc", 0.0), ("eva", 0.0)])
def test_mode_zero_is_the_azimuth_averaged_builder_bit_for_bit(name, g):
    N = 32
    s = _solver(4, N, B=3)
    kind, _ = _kind(s, name, g)
    mu0 = np.array([0.3, 0.5, 0.95])
    P, P0 = s.phase_matrix(kind, g), s.phase_p0(kind, mu0, g)
    for nphi in (25, 41):                       # mode 0 keeps the reference's 25-point ring whatever nphi the other modes use
        assert np.array_equal(s.phase_modes(kind, 0, 3, nphi, g)[0], P)
        assert np.array_equal(s.phase_p0_modes(kind, mu0, 0, 3, nphi, g)[0], P0)
    s.close()


@pytest.mark.parametrize("name,g", [("hg", 0.7), ("fwc", 0.0)])
@pytest.mark.parametrize("N", [32, 37, 128])
def test_higher_modes_match_numpy(name, g, N):
    s = _solver(4, N, B=2)
    kind, fn = _kind(s, name, g)
    mu = inputs.direction_grid(N)
    mu0 = np.array([0.45, 0.8])
    ms, nphi = [1, 2, 3, 4, 5, 6, 7, 8], 31
    ref = A.phase_modes(fn, mu, ms, nphi)
    scale = np.max(np.abs(A.phase_modes(fn, mu, [0], nphi)))
    got = s.phase_modes(kind, 1, len(ms), nphi, g)
    assert np.max(np.abs(got - ref)) <= 1e-12 * scale
    got = s.phase_modes(kind, 3, 2, nphi, g)                    # a range that does not start at 1
    assert np.max(np.abs(got - ref[2:4])) <= 1e-12 * scale
    P0 = s.phase_p0_modes(kind, mu0, 1, len(ms), nphi, g)
    for b in range(2):
        r0 = A.phase_p0_modes(fn, mu, mu0[b], ms, nphi)
        sc = np.max(np.abs(A.phase_p0_modes(fn, mu, mu0[b], [0], nphi)))
        assert np.max(np.abs(P0[:, b] - r0)) <= 1e-12 * sc
    # the flip symmetry survives: set_phase takes the symmetric contraction for a mode by itself
    s.set_phase(got[0], got[1])
    assert s.phase_asymmetry()[1]
    s.close()


def test_vanishing_modes():
    N = 32
    s = _solver(4, N, B=2)
    mu0 = np.array([0.4, 0.9])
    P = s.phase_modes("rayleigh", 0, 9, 25)
    P0 = s.phase_p0_modes("rayleigh", mu0, 0, 9, 25)
    assert not np.any(P[3:]) and not np.any(P0[3:])            # (exact zeros: p is quadratic in cos phi)
    s.set_phase(P[3], P[3])
    assert s.phase_asymmetry()[1]                               # (so a vanishing mode keeps the symmetric contraction)
    assert np.max(np.abs(P[1:3])) > 1e-3 * np.max(np.abs(P[0]))
    Pi = s.phase_modes("iso", 0, 4, 25)
    P0i = s.phase_p0_modes("iso", mu0, 0, 4, 25)
    assert not np.any(Pi[1:]) and not np.any(P0i[1:])
    with pytest.raises(ValueError):
        s.phase_modes("hg", 1, 24, 25, 0.5)                   # mode 24 aliases on 25 nodes
    with pytest.raises(ValueError):
        s.phase_modes("hg", 60, 6, 201, 0.5)                  # above SOSRT_MAX_MODES
    s.close()


# ---- 4: order targets ------------------------------------------------------------------------
def _three_zone(s, B, mu0, aer="hg", g_aer=0.7, L=60, N=64, tau_aer=0.3):
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    tau = np.stack([inputs.tau_profile(0.124, tau_aer, 120, 25, 17, L)] * B)
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, 0.15, 1.0, 0.95, 0.124 / L, tau_aer / (idn + 1 - iu), 0.124 + tau_aer)
    return tau, iu, idn


def _solve_targets(s, tau, P0a, P0r, targets, order_loop=0):
    dev = torch.device("cuda", 0)
    B = tau.shape[0]
    d = dict(tau=torch.from_numpy(tau).to(dev), a=torch.from_numpy(np.ascontiguousarray(P0a)).to(dev),
             r=torch.from_numpy(np.ascontiguousarray(P0r)).to(dev), t=torch.tensor(np.asarray(targets, dtype=np.int32)).to(dev))
    I = torch.empty((B, s.L, s.D), dtype=torch.float64, device=dev)
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.set_order_loop(order_loop)
    s.set_order_targets(d["t"].data_ptr())
    try:
        s.solve_device(d["tau"].data_ptr(), d["a"].data_ptr(), d["r"].data_ptr(), I.data_ptr(), d_n_orders=n.data_ptr(),
                       d_status=st.data_ptr())
        s.synchronize()
    finally:
        s.set_order_targets(None)
        s.set_order_loop(0)
    return I.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def test_order_targets():
    L, N, B = 60, 64, 6
    s = _solver(L, N, B=B, max_orders=40)
    mu0 = np.linspace(0.2, 0.9, B)
    tau, iu, idn = _three_zone(s, B, mu0)
    P0a, Pa = s.phase_p0("rayleigh", mu0), s.phase_matrix("rayleigh")
    P0r, Pr = s.phase_p0("hg", mu0, 0.7), s.phase_matrix("hg", 0.7)
    s.set_phase(Pa, Pr)
    ref = s.solve(tau, P0a, P0r, tol=1e-4)
    assert (ref.status == 0).all()
    # targets equal to the n of the tol-solve: the same bits
    I, n, st = _solve_targets(s, tau, P0a, P0r, ref.n)
    assert np.array_equal(n, ref.n) and np.array_equal(st, ref.status) and np.array_equal(I, ref.I)
    # other targets, one per column (1: the first order alone), also with the order-loop launch allowed (it is not planned)
    k = np.array([1, 2, 3, 7, 11, 40])
    for ol in (0, 1):
        I, n, st = _solve_targets(s, tau, P0a, P0r, k, order_loop=ol)
        assert np.array_equal(n, k) and (st == _lib.COL_OK).all() and np.isfinite(I).all()
        if ol:
            assert s.order_loop_stats()[0] == 0
    # a target above the budget is the only way to SOSRT_COL_MAXORDERS
    s.set_order_budget(10)
    I, n, st = _solve_targets(s, tau, P0a, P0r, [10, 10, 11, 5, 12, 10])
    assert list(n) == [10, 10, 10, 5, 10, 10]
    assert list(st) == [0, 0, _lib.COL_MAXORDERS, 0, _lib.COL_MAXORDERS, 0]
    s.set_order_budget(40)
    # vanishing modes: Rayleigh m = 3 and isotropic m = 1 fields (the In/I ratio is 0/0 there) run exactly k orders, no NaN
    for name, m in (("rayleigh", 3), ("iso", 1)):
        P = s.phase_modes(name, m, 1, 25)[0]
        P0 = s.phase_p0_modes(name, mu0, m, 1, 25)[0]
        s.set_phase(P, P)
        I, n, st = _solve_targets(s, tau, P0, P0, k)
        assert np.array_equal(n, k) and (st == _lib.COL_OK).all()
        assert not np.isnan(I).any()
        assert not np.any(I)
    s.close()


# ---- 5: mode solves against the oracle -------------------------------------------------------
def _oracle_fixed(c, k):
    I1 = O.first_order(c)
    In_1, I = I1, I1.copy()
    for _ in range(2, k + 1):
        In_1 = O.transport(c, O.source_function(c, In_1), literal=False)
        I = I + In_1
    return I


def test_driver_three_zone_signed_modes_against_the_oracle():
    """SOS_Aer_batch(..., azimuths=...) at TOA and surface against the oracle's mode fields synthesized the same way
    (g3-style Rayleigh + HG, L = 60, N = 64, three columns, M = 3), the oracle solving mode m with (-1)^m P^m, the sign of
    the reference's fold (azimuth_np.solve_modes; tests/test_azimuth_host.py checks it against a direct azimuth solve)."""
    L, N, M, nphi = 60, 64, 3, 25
    mu0 = np.array([0.35, 0.6, 0.85])
    phi = np.linspace(0, 2 * np.pi, 9)
    r = SOS_Aer_batch(mu0, 0.3, 0.15, alb_aer=0.95, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg",
                      g_aer=0.7, max_orders=64, azimuths=phi, n_modes=M)
    assert r.I_azimuth.shape == (3, 2, 2 * N, len(phi)) and r.mode_status.shape == (M + 1, 3) and not r.mode_status.any()
    mu = inputs.direction_grid(N)
    ray, hg = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.7)[0]
    Pa, Pr = A.solve_modes(ray, mu, range(1, M + 1), nphi), A.solve_modes(hg, mu, range(1, M + 1), nphi)
    for b in range(3):
        P0a = A.phase_p0_modes(ray, mu, mu0[b], range(1, M + 1), nphi)
        P0r = A.phase_p0_modes(hg, mu, mu0[b], range(1, M + 1), nphi)
        syn = r.I[b][[0, L - 1]][..., None] * np.ones(len(phi))
        for m in range(1, M + 1):
            c = O.make_column(mu0[b], 120, 25, 17, L, 0.124, 0.3, 0.15, 1.0, 0.95, N, P0a[m - 1], Pa[m - 1], P0r[m - 1], Pr[m - 1])
            Im = _oracle_fixed(c, int(r.n[b]))
            syn = syn + 2 * Im[[0, L - 1]][..., None] * np.cos(m * phi)
        _close(r.I_azimuth[b], syn, RTOL, "I(phi), column %d" % b)


@pytest.mark.parametrize("case", ["single_slab", "eva"])
def test_mode_solve_against_the_oracle(case):
    """A mode m >= 1 solved with the order count of its mode-0 solve, against the oracle driven with the mode matrices:
    the single-slab geometry (HG, m = 2) and one EVA column at L = 200, N = 128 (m = 1)."""
    if case == "single_slab":
        L, N, m, name, g = 40, 48, 2, "hg", 0.6
    else:
        L, N, m, name, g = 200, 128, 1, "eva", 0.0
    s = _solver(L, N, B=1, max_orders=200)
    mu = inputs.direction_grid(N)
    mu0 = np.array([0.55])
    kind, _ = _kind(s, name, g)
    P, P0 = s.phase_matrix(kind, g), s.phase_p0(kind, mu0, g)
    Pm, P0m = s.phase_modes(kind, m, 1, 25, g)[0], s.phase_p0_modes(kind, mu0, m, 1, 25, g)[0]
    if case == "single_slab":
        tau = np.linspace(0.0, 0.5, L)[None]
        s.set_columns_single_slab(mu0, 0.95, 0.5)
        s.set_phase(P)
        n = int(s.solve(tau, P0).n[0])
        s.set_phase(Pm)
        I, nn, st = _solve_targets(s, tau, P0m, P0m, [n])
        ref = O.I1_NumInt(tau[0], mu, 0.5, 0.55, P0m[0], 0.95, N)
        In_1, Iref = ref, ref.copy()
        for k in range(2, n + 1):
            Jn = O.Jn_NumInt(k, In_1, tau[0], mu, 0.5, 0.55, Pm, 0.95, N)
            In_1 = O.In_NumInt(k, Jn, In_1, tau[0], mu, 0.5, 0.55, Pm, 0.95, N, literal=False)
            Iref = Iref + In_1
    else:
        Pa, P0a = s.phase_matrix("rayleigh"), s.phase_p0("rayleigh", mu0)
        Pam, P0am = s.phase_modes("rayleigh", m, 1, 25)[0], s.phase_p0_modes("rayleigh", mu0, m, 1, 25)[0]
        tau, iu, idn = _three_zone(s, 1, mu0, L=L, N=N, tau_aer=0.5)
        s.set_phase(Pa, P)
        n = int(s.solve(tau, P0a, P0).n[0])
        s.set_phase(Pam, Pm)
        I, nn, st = _solve_targets(s, tau, P0am, P0m, [n])
        c = O.make_column(0.55, 120, 25, 17, L, 0.124, 0.5, 0.15, 1.0, 0.95, N, P0am[0], Pam, P0m[0], Pm)
        Iref = _oracle_fixed(c, n)
    assert int(nn[0]) == n and st[0] == 0
    _close(I[0], Iref, RTOL, "%s mode %d" % (case, m))
    s.close()


# ---- 6: first order against its closed form --------------------------------------------------
@pytest.mark.parametrize("name,g,M,nphi,tol", [("rayleigh", 0.0, 2, 25, 1e-12), ("hg", 0.7, 60, 401, 1e-9)])
def test_first_order_against_the_closed_form(name, g, M, nphi, tol):
    """Budget 1: I(phi) is the first order of p(c(mu, mu0, phi)) / Z0 (Rayleigh: all of it, exact on 25 nodes; HG g = 0.7:
    the part of the modes m >= 1, against the first order of p(c) / Z0 minus the nphi-node mode 0)."""
    L, N = 60, 64
    mu0 = 0.6
    phi = np.array([0.0, 0.5, 1.7, 2.6, np.pi])
    r = SOS_Aer_batch(mu0, 0.3, 0.15, alb_aer=0.95, nb_layers=L, nb_angles=N, atm_phase_fun=name, g_atm=g, aer_phase_fun=name,
                      g_aer=g, max_orders=1, azimuths=phi, n_modes=M, nphi_modes=nphi)
    assert list(r.n) == [1]
    mu = inputs.direction_grid(N)
    fn = inputs._scalar_phase(name, g)[0]
    rows = [0, L - 1]
    P = np.zeros((2 * N, 2 * N))
    base = np.zeros((2, 2 * N)) if name == "rayleigh" else r.I[0][rows]
    if name != "rayleigh":
        P0_nphi = A.phase_p0_modes(fn, mu, mu0, [0], nphi)[0]
        c = O.make_column(mu0, 120, 25, 17, L, 0.124, 0.3, 0.15, 1.0, 0.95, N, P0_nphi, P, P0_nphi, P)
        minus = O.first_order(c)[rows]
    for j, f in enumerate(phi):
        Pd = A.p0_direct(fn, mu, mu0, f, 25 if name == "rayleigh" else nphi)
        c = O.make_column(mu0, 120, 25, 17, L, 0.124, 0.3, 0.15, 1.0, 0.95, N, Pd, P, Pd, P)
        ref = O.first_order(c)[rows]
        got = r.I_azimuth[0][..., j]
        if name != "rayleigh":
            ref, got = ref - minus, got - base
        assert np.max(np.abs(got - ref)) <= tol * np.max(np.abs(ref)), "phi = %g" % f


# ---- 7: invariants ---------------------------------------------------------------------------
def test_invariants_of_the_azimuth_call():
    L, N, M = 60, 64, 4
    mu0 = np.array([0.3, 0.7])
    kw = dict(nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.5, max_orders=64)
    plain = SOS_Aer_batch(mu0, 0.3, 0.15, **kw)
    tight = SOS_Aer_batch(mu0, 0.3, 0.15, tol=1e-7, **kw)
    phi = 2 * np.pi * np.arange(2 * M + 1) / (2 * M + 1)
    az = SOS_Aer_batch(mu0, 0.3, 0.15, azimuths=phi, n_modes=M, levels=(0, 10, -1), **kw)
    assert np.array_equal(az.I, plain.I) and np.array_equal(az.n, plain.n) and np.array_equal(az.status, plain.status)
    assert plain.I_azimuth is None and plain.mode_status is None
    # the mean over 2M + 1 uniform azimuths is mode 0
    ref = az.I[:, [0, 10, L - 1]]
    assert np.max(np.abs(az.I_azimuth.mean(axis=-1) - ref)) <= 1e-13 * np.max(np.abs(ref))
    # the cached handle is left as it was: the plain call again gives the same bits
    again = SOS_Aer_batch(mu0, 0.3, 0.15, **kw)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n)
    # and its order targets are cleared: another tolerance runs its own orders again
    t2 = SOS_Aer_batch(mu0, 0.3, 0.15, tol=1e-7, **kw)
    assert np.array_equal(t2.n, tight.n) and np.array_equal(t2.I, tight.I) and (tight.n > plain.n).all()
