"""Delta-M on the device (csrc/deltam.hip, csrc/api_deltam.hip, k_phase_p0_normaliser of csrc/phase.hip),
through the C ABI: the two kernels against the NumPy model of tests/deltam_np.py, the normaliser entry against the table itself,
the drivers against the chain built by hand and against the model chain on the oracle, the TMS first order, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import deltam_np as DM
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import _lib, deltam, inputs
from sosrt.main import SOS_Aer, SOS_Aer_batch, solve_batch_device
from sosrt.solver import Solver
from util import assert_close

pytestmark = pytest.mark.gpu

NTABS = (2, 33, 257, 1001, 6001)
LMAXS = (1, 16, 128)
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def solver():
    s = Solver(40, 32, max_batch=8, max_orders=64)
    s.set_grid(inputs.direction_grid(32))
    yield s
    s.close()


def table(ntab, seed=0):
    """(non-uniform ascending abscissa, S = 3 positive forward-peaked tables): 1001 points are the reference's cloud table and
    two siblings of it."""
    rng = np.random.default_rng(100 + ntab + seed)
    if ntab == 1001:
        x, p = inputs.fwc_table()
        return x, np.stack([p, p[::-1] * 0.5 + 1.0, np.sqrt(p)])
    x = np.sort(np.concatenate(([-1.0, 1.0], rng.uniform(-1, 1, ntab - 2))))
    if ntab > 2:
        assert np.all(np.diff(x) > 0)
    return x, np.stack([DM.hg(g)(x) * (1 + 0.1 * rng.uniform(size=ntab)) for g in (0.85, 0.3, -0.5)])


# ---- the moments kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntab", NTABS)
def test_moments_against_the_model(solver, ntab):
    x, P = table(ntab)
    for lmax in LMAXS:
        for tab_mu in (x, None):
            chi, norm = solver.phase_moments(P, lmax, tab_mu)
            again = solver.phase_moments(P, lmax, tab_mu)
            assert np.array_equal(chi, again[0]) and np.array_equal(norm, again[1])          # the same call, the same bits
            assert np.all(chi[:, 0] == 1.0)
            worst = 0.0
            for s in range(3):
                want, wn = DM.moments(tab_mu, P[s], lmax)
                worst = max(worst, np.max(np.abs(chi[s] - want)))
                assert np.max(np.abs(chi[s] - want)) <= 1e-11, (ntab, lmax, s)
                assert abs(norm[s] - wn) <= 1e-11 * wn
                one, n1 = solver.phase_moments(P[s], lmax, tab_mu)                            # S = 1: the batch's bits
                assert np.array_equal(one, chi[s]) and n1 == norm[s]
            print("ntab=%d lmax=%d %s: |chi - model| <= %.2e" % (ntab, lmax, "caller's abscissa" if tab_mu is not None else "uniform", worst))


def test_moments_device_form_has_the_host_form_bits(solver):
    x, P = table(257)
    d_x, d_P = torch.from_numpy(x).to(DEV), torch.from_numpy(P).to(DEV)
    d_chi, d_norm = torch.empty((3, 17), dtype=torch.float64, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    solver.phase_moments_device(d_P.data_ptr(), 3, 257, 16, d_chi.data_ptr(), d_norm.data_ptr(), d_tab_mu=d_x.data_ptr())
    solver.synchronize()
    chi, norm = solver.phase_moments(P, 16, x)
    assert np.array_equal(d_chi.cpu().numpy(), chi) and np.array_equal(d_norm.cpu().numpy(), norm)


def test_moments_refusals(solver):
    for ntab, lmax in ((1, 4), (65537, 4), (9, 0), (9, 129)):
        chi = np.full((1, max(lmax, 0) + 1), -7.0)
        p = np.ones((1, ntab))
        rc = _lib.lib().sosrt_phase_moments(solver._h, 1, None, p.ctypes.data_as(ctypes.c_void_p), ntab, lmax,
                                            chi.ctypes.data_as(ctypes.c_void_p), None)
        assert rc == _lib.E_INVALID and _lib.lib().sosrt_last_error() and np.all(chi == -7.0)
    with pytest.raises(ValueError, match="ascending"):
        solver.phase_moments(np.ones(4), 2, np.array([-1.0, 0.0, 0.0, 1.0]))
    assert solver.phase_moments(np.ones(65536), 1)[0][1] == pytest.approx(0.0, abs=1e-12)     # the cap itself is served


# ---- the delta-M kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntab", NTABS)
def test_delta_m_table_against_the_model(solver, ntab):
    x, P = table(ntab)
    for lmax in (16, 128):
        chi = np.stack([DM.moments(x, P[s], lmax)[0] for s in range(3)])
        if lmax == 128:
            chi[1] = deltam.hg_moments(0.6, lmax)            # (moments that do not die out before the cap)
        for order in sorted({1, 2, 16, lmax}):
            for tab_mu in (x, None):
                xx = DM.abscissa(ntab, tab_mu)
                got, f = solver.delta_m_table(chi, order, ntab=ntab, tab_mu=tab_mu)
                for s in range(3):
                    want, wf = DM.delta_m_table(chi[s], order, xx)
                    assert f[s] == wf == chi[s, order]
                    assert np.max(np.abs(got[s] - want)) <= 1e-11 * DM.table_bound(chi[s], order), (ntab, lmax, order, s)
                    one, f1 = solver.delta_m_table(chi[s], order, ntab=ntab, tab_mu=tab_mu)
                    assert np.array_equal(one, got[s]) and f1 == f[s]


def test_delta_m_reproduces_hg(solver):
    chi = deltam.hg_moments(0.7, 128)
    for ntab in NTABS:
        x = np.linspace(-1, 1, ntab)
        got, f = solver.delta_m_table(chi, 128, ntab=ntab)
        assert f == 0.7 ** 128
        assert np.max(np.abs(got - DM.hg(0.7)(x))) <= 1e-11 * 18.9, ntab


def test_delta_m_refusals(solver):
    good = deltam.hg_moments(0.7, 16)
    cases = {"f >= 1 - 1e-6": (np.where(np.arange(17) == 8, 1 - 5e-7, good), 8, "1 - 1e-6"),
             "order > lmax": (good, 17, "order"),
             "order 0": (good, 0, "order"),
             "NaN": (np.where(np.arange(17) == 3, np.nan, good), 8, "not finite"),
             "inf beyond the order": (np.where(np.arange(17) == 12, np.inf, good), 8, "not finite")}
    for what, (chi, order, msg) in cases.items():
        chi = np.ascontiguousarray(chi)
        out, f = np.full(33, -7.0), np.full(1, -7.0)
        rc = _lib.lib().sosrt_phase_delta_m(solver._h, 1, chi.ctypes.data_as(ctypes.c_void_p), 16, order, None, 33,
                                            out.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p))
        assert rc == _lib.E_INVALID and msg in _lib.lib().sosrt_last_error().decode(), what
        assert np.all(out == -7.0) and f[0] == -7.0, what
        # the device form: the same refusal, the same untouched outputs
        d_chi, d_out, d_f = torch.from_numpy(chi).to(DEV), torch.full((33,), -7.0, dtype=torch.float64, device=DEV), \
            torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match=msg):
            solver.delta_m_table_device(d_chi.data_ptr(), 1, 16, order, 33, d_out.data_ptr(), d_f.data_ptr())
        solver.synchronize()
        assert torch.all(d_out == -7.0).item() and d_f.item() == -7.0, what
    # a slightly negative f, a converged series, is served
    t, f = solver.delta_m_table(np.where(np.arange(17) == 16, -1e-9, good), 16, ntab=33)
    assert f == -1e-9 and np.all(np.isfinite(t))


# ---- the normaliser entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 5))
def test_normaliser_gives_back_the_table(solver, B):
    """value of P0_rows_azimuth x Z = the function at that scattering cosine.  The lanes, suns and azimuths keep the cosines
    away from the forward peak, where a last-bit difference of the cosine itself moves the value by more than the bound."""
    mu0 = np.array([0.25, 0.4, 0.6, 0.75, 0.95])[:B] if B > 1 else np.array([0.6])
    sgn, phi = np.array([-0.8, -0.35, 0.35, 0.8]), np.array([0.0, 0.7, 2.1])
    mt, pt = inputs.fwc_table()
    solver.set_phase_table(mt, pt)
    d_mu0, d_phi = torch.from_numpy(mu0).to(DEV), torch.from_numpy(phi).to(DEV)
    c = -(sgn[None, None, :] * mu0[None, :, None]
          + np.sqrt(1 - sgn * sgn)[None, None, :] * np.sqrt(1 - mu0 * mu0)[None, :, None] * np.cos(phi)[:, None, None])
    for kind, g, fn in (("table", 0.0, lambda x: O.interpolate_table(mt, pt, x)), ("hg", 0.7, DM.hg(0.7))):
        d_out = torch.empty((len(phi), B, len(sgn)), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        solver.phase_p0_rows_azimuth_device(kind, d_mu0.data_ptr(), sgn, d_phi.data_ptr(), len(phi), d_out.data_ptr(), B, g)
        solver.synchronize()
        Z = solver.p0_normaliser(kind, mu0, g)
        got, want = d_out.cpu().numpy() * Z[None, :, None], fn(c)
        err = np.max(np.abs(got - want) / np.abs(want))
        print("%s B=%d: |value Z - p(c)| / p(c) <= %.2e" % (kind, B, err))
        assert err <= 1e-14
        # and Z is the normaliser of the model
        Zm = VA._trapz(O._azimuth_average(fn, inputs.direction_grid(32), mu0) / (4 * np.pi), inputs.direction_grid(32), axis=0)
        assert np.max(np.abs(Z - Zm) / Zm) <= 1e-12


# ---- the drivers -------------------------------------------------------------------------------------------------------------
L, N = 40, 32
MU0 = np.array([0.3, 0.45, 0.6, 0.8, 1.0])
TAER = np.array([0.05, 0.2, 0.5, 0.75, 1.0])
RHO = np.array([0.1, 0.0, 0.3, 0.1, 0.2])
COL = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.99, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh")


def hand_chain(s, name, g, order):
    """(abscissa or None, truncated table, f, tau', w') by the solver's methods."""
    if name == "hg":
        x, chi = None, deltam.hg_moments(g, order)
        t, f = s.delta_m_table(chi, order, ntab=deltam.HG_NTAB)
    else:
        x, p = inputs.fwc_table()
        chi, _ = s.phase_moments(p, order, x)
        t, f = s.delta_m_table(chi, order, tab_mu=x)
    return (x, t, f) + deltam.scale_optics(TAER, COL["alb_aer"], f)


@pytest.mark.parametrize("name,g", (("fwc", 0.0), ("hg", 0.85)))
def test_driver_equals_the_hand_chain(solver, name, g):
    # (HG 0.85 at Lambda = 16 keeps f = 0.074 only and its truncated table rings below zero: on the oracle two of the five
    # columns leave the mu -> 0 search, and so they must here -- the status is part of what is compared)
    order = 16
    r = SOS_Aer_batch(MU0, TAER, RHO, aer_phase_fun=name, g_aer=g, delta_m=order, raise_on_error=False, **COL)
    x, t, f, tau2, w2 = hand_chain(solver, name, g, order)
    xx = DM.abscissa(len(t), x)
    solver.set_phase_table(xx, t)
    P0, P = solver.phase_p0("table", MU0), solver.phase_matrix("table")
    hand = SOS_Aer_batch(MU0, tau2, RHO, P_aer=P, P0_aer=P0, raise_on_error=False, **dict(COL, alb_aer=w2))
    assert r.delta_m_f == f and np.array_equal(r.tauStar_aer_scaled, tau2) and np.array_equal(r.alb_aer_scaled, w2)
    assert np.array_equal(r.I, hand.I, equal_nan=True) and np.array_equal(r.n, hand.n) and np.array_equal(r.status, hand.status)
    assert np.array_equal(r.tau, hand.tau)
    # the model chain through the oracle
    exact = inputs.fwc_table() if name == "fwc" else (xx, DM.hg(g)(xx))
    chi = deltam.hg_moments(g, order) if name == "hg" else DM.moments(*exact, order)[0]
    tm, fm = DM.delta_m_table(chi, order, xx)
    for b in range(len(MU0)):
        c = DM.oracle_column(MU0[b], L, N, TAER[b], (xx, tm), fm, grd_alb=RHO[b])
        try:
            sol = O.solve_column(c, literal=False, max_orders=256)
        except IndexError:
            assert r.status[b] == _lib.COL_INDEXERROR, "%s column %d: the oracle leaves the mu -> 0 search" % (name, b)
            continue
        assert r.status[b] == 0 and sol.n == r.n[b]
        assert_close(r.I[b], sol.I, what="%s column %d" % (name, b))
    assert not r.status.any() or name == "hg"
    # the same through the other drivers
    one = SOS_Aer(mu0=MU0[1], tauStar_aer=TAER[1], grd_alb=RHO[1], aer_phase_fun=name, g_aer=g, delta_m=order, z0=120, z_up=25, z_down=17,
                  **COL)
    assert np.array_equal(one.I, r.I[1]) and one.n == r.n[1] and one.delta_m_f == f and one.tauStar_aer_scaled == tau2[1]
    dev, _ = solve_batch_device(MU0, TAER, RHO, aer_phase_fun=name, g_aer=g, delta_m=order, **COL)
    assert np.array_equal(dev["I"].cpu().numpy(), r.I, equal_nan=True) and dev["delta_m_f"] == f and np.array_equal(dev["alb_aer_scaled"], w2)


def test_delta_m_none_is_the_plain_call():
    a = SOS_Aer_batch(MU0, TAER * 0.2, RHO, aer_phase_fun="hg", g_aer=0.7, **COL)
    b = SOS_Aer_batch(MU0, TAER * 0.2, RHO, aer_phase_fun="hg", g_aer=0.7, delta_m=None, **COL)
    assert np.array_equal(a.I, b.I) and np.array_equal(a.n, b.n) and b.delta_m_f is None and b.tauStar_aer_scaled is None


def test_forcing_takes_the_scaled_column(solver):
    from sosrt import forcing
    geo = dict(nb_layers=L, nb_angles=N, aer_phase_fun="fwc")
    got = forcing.toa_net_flux(0.6, 0.124, TAER[:3], 0.1, 1.0, 0.99, delta_m=16, **geo)
    x, t, f, tau2, w2 = hand_chain(solver, "fwc", 0.0, 16)
    solver.set_phase_table(x, t)
    mu = inputs.direction_grid(N)
    P0a, Pa = inputs.phase_function_device("rayleigh", N, mu, 0.6, solver=solver)
    phases = (P0a, Pa, solver.phase_p0("table", [0.6])[0], solver.phase_matrix("table"))
    want = forcing.toa_net_flux(0.6, 0.124, tau2[:3], 0.1, 1.0, w2[:3], phases=phases, **geo)
    assert np.array_equal(got, want)
    rf = forcing.radiative_forcing(0.6, 0.124, TAER[:2], 0.1, 1.0, 0.99, delta_m=16, **geo)
    assert rf.shape == (2,) and np.all(np.isfinite(rf))


def test_the_point_of_it():
    """The oracle's result of tests/test_deltam_host.py on the device: the raw cloud table leaves the reference's mu -> 0 search
    (its own status code), the delta-M column solves."""
    kw = dict(COL, nb_angles=64, aer_phase_fun="fwc")
    raw = SOS_Aer_batch([0.6], [0.5], [0.1], raise_on_error=False, **kw)
    assert raw.status[0] == _lib.COL_INDEXERROR
    dm = SOS_Aer_batch([0.6], [0.5], [0.1], raise_on_error=False, delta_m=8, **kw)
    assert dm.status[0] == 0 and np.all(np.isfinite(dm.I))
    print("tauStar_aer = 0.5, N = 64: raw status %d, delta_m=8 status 0 in %d orders" % (raw.status[0], dm.n[0]))


# ---- TMS ---------------------------------------------------------------------------------------------------------------------
def test_tms_first_order(solver):
    order, mu = 16, inputs.direction_grid(N)
    mu0, taer, rho = MU0[1:4], TAER[1:4], RHO[1:4]
    vmu = np.array([0.35, mu[N + 9], 0.9])                   # (one is a node)
    phi = np.array([0.0, 0.9, 2.4, np.pi])
    rows = [0, L - 1]
    kw = dict(COL, aer_phase_fun="fwc", delta_m=order)
    r = SOS_Aer_batch(mu0, taer, rho, view_mu=vmu, view_azimuths=phi, **kw)
    base = SOS_Aer_batch(mu0, taer, rho, view_mu=vmu, **kw)
    plain = SOS_Aer_batch(mu0, taer, rho, **kw)
    assert r.view_mode_status.shape == (order, 3) and not r.view_mode_status.any()            # n_modes = Lambda - 1
    assert np.array_equal(r.I, plain.I) and np.array_equal(r.n, plain.n) and np.array_equal(base.I, plain.I)
    assert np.array_equal(r.I_view, base.I_view) and np.array_equal(r.I_view_first, base.I_view_first)
    assert np.array_equal(r.I_view_azimuth, r.I_view_azimuth_first + r.I_view_azimuth_scattered)
    # the hand chain: the truncated table as a named table, the scaled optics, the series up to Lambda - 1
    x, t, f, tau2, w2 = hand_chain(solver, "fwc", 0.0, order)
    tau2, w2 = tau2[1:4], w2[1:4]
    hkw = dict(COL, aer_phase_fun="table", mie_aer=dict(table=(x, t)), alb_aer=w2)
    hand = SOS_Aer_batch(mu0, tau2, rho, view_mu=vmu, view_azimuths=phi, n_modes=order - 1, **hkw)
    assert np.array_equal(r.I_view_azimuth_scattered, hand.I_view_azimuth_scattered)
    assert np.array_equal(r.I_view_scattered, hand.I_view_scattered) and np.array_equal(r.I_view_first, hand.I_view_first)
    modes = SOS_Aer_batch(mu0, taer, rho, view_mu=vmu, view_azimuths=phi, view_first_order="modes", **kw)
    hmodes = SOS_Aer_batch(mu0, tau2, rho, view_mu=vmu, view_azimuths=phi, n_modes=order - 1, view_first_order="modes", **hkw)
    assert np.array_equal(modes.I_view_azimuth_first, hmodes.I_view_azimuth_first)            # 'modes' stays the truncated series
    # the model: the view-azimuth first order fed the scaled optics and the aerosol values p_exact / ((1 - f) Z_trunc)
    mt, pt = inputs.fwc_table()
    norm = solver.phase_moments(pt, order, mt)[1]
    sgn = VN.signed(vmu)
    ray = VN.phase_fn("rayleigh")
    Zt = VA._trapz(O._azimuth_average(lambda c: O.interpolate_table(x, t, c), mu, mu0) / (4 * np.pi), mu, axis=0)
    cs = -(sgn[None, None, :] * mu0[None, :, None]
           + np.sqrt(1 - sgn * sgn)[None, None, :] * np.sqrt(1 - mu0 * mu0)[None, :, None] * np.cos(phi)[:, None, None])
    Ea = VA.p0_exact(ray, mu, mu0, sgn, phi)
    Er = O.interpolate_table(mt, pt / norm, cs) / ((1 - f) * Zt[None, :, None])
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    for b in range(3):
        c = O.make_column(mu0[b], 120, 25, 17, L, 0.124, tau2[b], rho[b], 1.0, w2[b], N, Z1, Z2, Z1, Z2)
        want = np.moveaxis(np.stack([VN.first_order(c, Ea[i, b], Er[i, b], vmu)[rows] for i in range(len(phi))]), 0, -1)
        err = np.max(np.abs(r.I_view_azimuth_first[b] - want)) / np.max(np.abs(want))
        print("TMS first order, column %d: within %.2e of its maximum; the truncated series misses it by %.2e"
              % (b, err, np.max(np.abs(modes.I_view_azimuth_first[b] - want)) / np.max(np.abs(want))))
        assert err <= 1e-13


def test_device_refusals():
    """What needs a handle to be refused, and the view call that stays refused."""
    with pytest.raises(ValueError):
        SOS_Aer_batch(MU0, TAER, RHO, aer_phase_fun="fwc", delta_m=16, view_mu=[0.5], azimuths=[0.0], **COL)
    s = Solver(4, 4)
    try:
        with pytest.raises(ValueError):
            deltam.delta_m(s, "iso", 8)
        with pytest.raises(ValueError):
            deltam.delta_m(s, "rayleigh", 8)
        f, addr, keep = deltam.delta_m(s, "fwc", 8)
        assert 0 < f < 1 and addr == keep["exact"].data_ptr() and keep["ntab"] == 1001
        f2, addr2, _ = deltam.delta_m(s, "hg", 8, g=0.85)
        assert f2 == 0.85 ** 8 and addr2 == 0
    finally:
        s.close()
