"""Mie and log-normal ensemble phase tables built ON THE DEVICE (csrc/epilogue.hip: k_mie_coefficients, k_mie_angles,
k_mie_integrate) against the host series of sosrt/mie.py, published efficiencies, and through the solver.
Needs an MI355X.

Distances measured while this file was written (CPU, NumPy): the host's float64 efficiencies (Q_ext, Q_sca, g) lie within
1.5e-16 (m = 0.75, x = 1000) and 1.8e-16 (m = 1.5, x = 2000) of the same formulas evaluated in numpy.longdouble / clongdouble
(`_efficiencies_longdouble`); the device is given ten times the distance the test itself measures for the case
(measured on an MI355X: device 1.2e-16 at x = 1000, 1.8e-16 at x = 2000; tables 2.6e-15 eva, 1.8e-15 wildfire, 3.6e-15 one sphere
from the host series)."""
import numpy as np
import pytest

from sosrt import _lib, inputs, mie
from sosrt.main import SOS_Aer_batch, SOS_Aer_spectrum, get_solver
from sosrt.solver import Solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu

_trapz = getattr(np, "trapezoid", None) or np.trapz

# Bohren & Huffman appendix A (five digits) and Wiscombe 1979, NCAR/TN-140+STR (six digits; absorbing cases as n + ik):
# (m, x, Q_ext, Q_sca, g)
BH = (1.55 + 0j, 2 * np.pi * 0.525 / 0.6328, (3.10543, 3.10543, 2.92534, 0.63314))
WISCOMBE = (((1.5 + 0j), 10.0, (2.881999, 2.881999, 0.742913)),
            ((0.75 + 0j), 10.0, (2.232265, 2.232265, 0.896473)),
            ((0.75 + 0j), 1000.0, (1.997908, 1.997908, 0.844944)),
            ((1.5 + 1j), 1.0, (2.336321, 0.663454, 0.192136)),
            ((1.5 + 1j), 100.0, (2.097502, 1.283697, 0.850252)),
            ((10 + 10j), 1.0, (2.532993, 2.049405, -0.110664)),
            ((10 + 10j), 100.0, (2.071124, 1.836785, 0.556215)))


@pytest.fixture(scope="module")
def solver():
    s = Solver(2, 4, max_batch=1, max_orders=1)
    yield s
    s.close()


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def _efficiencies_longdouble(m, x):
    """mie.mie_coefficients and the sums of mie.efficiencies retyped in numpy.longdouble / clongdouble: (Q_ext, Q_sca, g)"""
    LD, CLD = np.longdouble, np.clongdouble
    nmax = int(np.round(x + 4.0 * x ** (1.0 / 3.0) + 2.0))
    nmx = int(max(nmax, abs(m * x)) + 16)
    m, x = CLD(m), LD(x)
    mx = m * x
    D = np.zeros(nmx + 1, dtype=CLD)
    for n in range(nmx, 0, -1):
        D[n - 1] = LD(n) / mx - LD(1) / (D[n] + LD(n) / mx)
    psi0, psi1 = np.cos(x), np.sin(x)
    chi0, chi1 = -np.sin(x), np.cos(x)
    a, b = np.zeros(nmax, dtype=CLD), np.zeros(nmax, dtype=CLD)
    for n in range(1, nmax + 1):
        c = LD(2 * n - 1) / x
        psi, chi = c * psi1 - psi0, c * chi1 - chi0
        xi, xi1 = CLD(psi) - CLD(1j) * chi, CLD(psi1) - CLD(1j) * chi1
        da, db = D[n] / m + LD(n) / x, D[n] * m + LD(n) / x
        a[n - 1] = (da * psi - psi1) / (da * xi - xi1)
        b[n - 1] = (db * psi - psi1) / (db * xi - xi1)
        psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
    n = np.arange(1, nmax + 1).astype(LD)
    qext = 2 / x ** 2 * np.sum((2 * n + 1) * (a + b).real)
    qsca = 2 / x ** 2 * np.sum((2 * n + 1) * (np.abs(a) ** 2 + np.abs(b) ** 2))
    g = 4 / (qsca * x ** 2) * (np.sum(n[:-1] * (n[:-1] + 2) / (n[:-1] + 1) * (a[:-1] * np.conj(a[1:]) + b[:-1] * np.conj(b[1:])).real)
                               + np.sum((2 * n + 1) / (n * (n + 1)) * (a * np.conj(b)).real))
    return np.array([qext, qsca, g])


# ---- 1. table against the host series -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eva", "wildfire"])
def test_ensemble_table_matches_host_series(solver, name):
    """README parameters, 100 radii, 6001 abscissae: element-wise relative 1e-12 against mie.log_normal_bulk_phase."""
    kw = mie.SCENARIOS[name]
    mu_h, p_h = mie.log_normal_bulk_phase(**kw)
    mu_d, p_d, bulk = mie.log_normal_bulk_phase_device(solver, **kw)
    assert np.array_equal(mu_d, mu_h) and p_d.shape == (6001,) and np.all(p_d > 0)
    e = _relmax(p_d, p_h)
    print("%s: device table vs host series, max relative %.3e" % (name, e))
    assert e <= 1e-12
    # the same through inputs.scenario_table(device=), cached under its own key
    mt, pt = inputs.scenario_table(name, device=solver)
    assert np.array_equal(pt, p_d) and np.array_equal(mt, mu_h)
    assert inputs.scenario_table(name, device=True)[1] is pt
    assert inputs.scenario_table(name)[1] is not pt


def test_single_sphere_table_matches_host_series(solver):
    r, wl, m = 0.4, 0.55, 1.44 + 0j
    mu = np.linspace(-1, 1, 6001)
    p_h = mie.i_unpolarized(m, 2 * np.pi * r / wl, mu)
    mu_d, p_d, bulk = mie.log_normal_bulk_phase_device(solver, wl, m, nb_radius=1, r_min=r)
    e = _relmax(p_d, p_h)
    print("one sphere: device table vs host series, max relative %.3e" % e)
    assert np.array_equal(mu_d, mu) and e <= 1e-12
    qe, qs, _, g = mie.efficiencies(m, 2 * np.pi * r / wl)
    assert bulk[0] == pytest.approx(qs / qe, rel=1e-12) and bulk[1] == pytest.approx(g, rel=1e-12)
    assert bulk[2] == pytest.approx(np.pi * r * r * qe, rel=1e-12)
    tab = inputs._scalar_phase("mie", r=r, lambda0=wl, indx=m, device=solver)[1][1]
    assert np.array_equal(tab[1], p_d)


# ---- 2. published values ---------------------------------------------------------------------------------------------------
def test_efficiencies_match_published_values_and_host(solver):
    """Six digits of Wiscombe's tables (five of Bohren & Huffman's); 1e-12 against mie.efficiencies for x <= 100; the
    Rayleigh-regime values test_host.py pins; x down to 0.02."""
    q = solver.mie_efficiencies(BH[0], BH[1])[0]
    assert tuple(round(v, 5) for v in q) == BH[2]
    ms, xs = [c[0] for c in WISCOMBE], [c[1] for c in WISCOMBE]
    Q = solver.mie_efficiencies(np.array(ms), np.array(xs))
    for (m, x, pub), q in zip(WISCOMBE, Q):
        assert (round(q[0], 6), round(q[1], 6), round(q[3], 6)) == pub, (m, x, q)
        assert np.array_equal(q, solver.mie_efficiencies(m, x)[0])                     # a batch is its single calls
        if x <= 100:
            h = mie.efficiencies(m, x)
            e = max(abs(q[k] - h[k]) / abs(h[k]) for k in (0, 1, 3))
            print("m = %s x = %g: device vs host efficiencies %.3e" % (m, x, e))
            assert e <= 1e-12
    small = solver.mie_efficiencies([0.75 + 0j, 1.5 + 1j, 1.5 + 0j], [0.099, 0.055, 0.02])
    assert small[0, 0] == pytest.approx(7.417859e-06, rel=1e-6)
    assert tuple(small[1, :2]) == pytest.approx((0.101491, 1.1e-05), abs=5e-7)
    h = mie.efficiencies(1.5 + 0j, 0.02)
    assert max(abs(small[2, k] - h[k]) / abs(h[k]) for k in (0, 1, 3)) <= 1e-12


@pytest.mark.parametrize("m,x", [(0.75 + 0j, 1000.0), (1.5 + 0j, 2000.0)])
def test_large_size_parameters_against_extended_precision(solver, m, x):
    """x = 1000 and 2000 (the extinction paradox case; the D recurrence starts near 3 016): the device's (Q_ext, Q_sca, g) no
    further from the long-double evaluation of the same formulas than ten times the host float64's distance from it
    (measured: host 1.5e-16 at x = 1000, 1.8e-16 at x = 2000)."""
    ld = _efficiencies_longdouble(m, x)
    h = mie.efficiencies(m, x)
    q = solver.mie_efficiencies(m, x)[0]
    d_host = max(float(abs(np.longdouble(h[k]) - ld[j]) / abs(ld[j])) for j, k in enumerate((0, 1, 3)))
    d_dev = max(float(abs(np.longdouble(q[k]) - ld[j]) / abs(ld[j])) for j, k in enumerate((0, 1, 3)))
    print("m = %s x = %g: host vs long double %.3e, device vs long double %.3e" % (m, x, d_host, d_dev))
    assert d_dev <= 10 * d_host
    if x == 2000.0:
        assert q[0] == pytest.approx(2.0, abs=0.03)


# ---- 3. bulk numbers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eva", "wildfire"])
def test_bulk_numbers_match_numpy_integrals(solver, name):
    kw = mie.SCENARIOS[name]
    _, _, bulk = mie.log_normal_bulk_phase_device(solver, **kw)
    r = np.linspace(0.01, 10.0, 100)
    n_r = (1.0 / r) * np.exp(-((np.log(r) - np.log(kw["r_m"])) ** 2) / (2 * np.log(kw["sig"]) ** 2))
    q = np.array([mie.efficiencies(kw["m"], 2 * np.pi * ri / kw["wl"]) for ri in r])
    w = n_r * r * r
    omega = _trapz(w * q[:, 1], r) / _trapz(w * q[:, 0], r)
    g = _trapz(w * q[:, 1] * q[:, 3], r) / _trapz(w * q[:, 1], r)
    cext = np.pi * _trapz(w * q[:, 0], r) / _trapz(n_r, r)
    print("%s: omega %.15g g %.15g C_ext %.15g (device %s)" % (name, omega, g, cext, bulk))
    assert bulk[0] == pytest.approx(omega, rel=1e-12) and bulk[1] == pytest.approx(g, rel=1e-12)
    assert bulk[2] == pytest.approx(cext, rel=1e-12)
    if name == "eva":
        assert abs(bulk[0] - 1.0) <= 1e-12                   # no absorption: two different sums of the same coefficients
    else:
        assert bulk[0] < 1.0 - 1e-3


# ---- 4. batch = singles, repeatable ------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(solver):
    wl = np.array([0.35, 0.44, 0.55, 0.67, 0.87, 1.02, 1.6, 2.1])
    m = 1.5 + 1j * np.array([0.0, 0.001, 0.01, 0.03, 0.1, 0.0, 0.3, 0.02])
    r_m = np.array([0.506, 0.3, 0.065, 0.1, 0.8, 0.2, 0.05, 1.0])
    sig = np.array([1.2, 1.5, 1.8, 1.3, 1.25, 2.0, 1.5, 1.4])
    p, bulk = solver.mie_ensembles(wl, m, r_m, sig, nb_radius=37, ntab=1201)
    p2, bulk2 = solver.mie_ensembles(wl, m, r_m, sig, nb_radius=37, ntab=1201)
    assert np.array_equal(p, p2) and np.array_equal(bulk, bulk2)
    assert np.all(np.isfinite(p)) and np.all(p > 0)
    for k in range(8):
        pk, bk = solver.mie_ensembles(wl[k], m[k], r_m[k], sig[k], nb_radius=37, ntab=1201)
        assert np.array_equal(pk[0], p[k]) and np.array_equal(bk[0], bulk[k]), k


# ---- 5. through the solver -----------------------------------------------------------------------------------------------------
def test_device_table_through_the_solver():
    """C2 column (L = 200, N = 128) with the EVA aerosol from the device builder against the host-table run; and the azimuth
    builders on a table handed over on the device against the same table uploaded from the host, bit for bit."""
    import torch
    kw = dict(tauStar_atm=0.124, alb_aer=0.97, nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", aer_phase_fun="eva")
    host = SOS_Aer_batch(0.5, 0.120, 0.15, **kw)
    dev = SOS_Aer_batch(0.5, 0.120, 0.15, mie_aer=dict(device=True), **kw)
    assert np.array_equal(dev.n, host.n) and np.all(dev.status == _lib.COL_OK)
    assert_close(dev.I, host.I, RTOL, "field with the device-built table vs the host-built one")
    s = get_solver(200, 128, 1, 256)
    sc = mie.SCENARIOS["eva"]
    d_p = torch.empty((1, 6001), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    s.mie_ensembles_device(d_p.data_ptr(), 0, sc["wl"], sc["m"], sc["r_m"], sc["sig"])
    s.set_phase_table_dev(d_p.data_ptr(), 6001)
    mu0 = np.array([0.2, 0.5, 1.0])
    P0_d, P_d = s.phase_p0("table", mu0), s.phase_matrix("table")
    s.synchronize()
    p = d_p.cpu().numpy()[0]
    assert np.array_equal(p, s.mie_ensembles(sc["wl"], sc["m"], sc["r_m"], sc["sig"])[0][0])
    s.set_phase_table(np.linspace(-1, 1, 6001), p)
    assert np.array_equal(s.phase_p0("table", mu0), P0_d) and np.array_equal(s.phase_matrix("table"), P_d)


# ---- 6. spectrum driver --------------------------------------------------------------------------------------------------------
def test_spectrum_equals_batches_by_hand():
    wl = np.array([0.44, 0.55, 0.67, 0.87])
    aer = dict(m=1.5 + 0.01j, r_m=0.3, sig=1.5)
    mu0, rho = np.array([0.5, 0.6, 0.8]), np.array([0.05, 0.15, 0.3])
    shape = dict(nb_layers=50, nb_angles=32, raise_on_error=False)
    res, bulk = SOS_Aer_spectrum(wl, mu0, 0.2, rho, aer, angstrom=1.3, tauStar_atm_ref=0.1, nb_radius=40, ntab=2001, **shape)
    assert len(res) == 4 and bulk.shape == (4, 3) and np.all(bulk[:, 0] < 1)
    s = get_solver(50, 32, 3, 256)
    t_aer, t_atm = 0.2 * (wl / 0.55) ** -1.3, 0.1 * (0.55 / wl) ** 4           # Angstrom law; Rayleigh ~ wl^-4
    for w in range(4):
        p, b = s.mie_ensembles(wl[w], aer["m"], aer["r_m"], aer["sig"], nb_radius=40, ntab=2001)
        assert np.array_equal(b[0], bulk[w])
        byhand = SOS_Aer_batch(mu0, t_aer[w], rho, tauStar_atm=t_atm[w], alb_aer=b[0, 0],
                               aer_phase_fun="table", mie_aer=dict(table=(np.linspace(-1, 1, 2001), p[0])), **shape)
        assert np.array_equal(res[w].I, byhand.I) and np.array_equal(res[w].n, byhand.n), w
        assert np.array_equal(res[w].tau, byhand.tau) and np.array_equal(res[w].status, byhand.status)
        assert np.all(res[w].status == _lib.COL_OK)
    assert not np.array_equal(res[0].I, res[3].I)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(solver):
    lib = _lib.lib()
    import ctypes
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = lambda v: np.array([v], dtype=np.float64)
    for what, wl, sig, nb_radius, r_max, ntab in (("x beyond the cap", 1e-4, 1.2, 100, 10.0, 6001), ("sig <= 1", 0.55, 1.0, 100, 10.0, 6001),
                                                  ("sig <= 1", 0.55, 0.8, 100, 10.0, 6001), ("ntab < 2", 0.55, 1.2, 100, 10.0, 1),
                                                  ("nb_radius < 1", 0.55, 1.2, 0, 10.0, 6001), ("workspace", 0.55, 1.2, 1 << 23, 10.0, 6001)):
        p, bulk = np.full(6001, -7.0), np.full(3, -7.0)
        rc = lib.sosrt_mie_ensembles(solver._h, 1, vp(one(wl)), vp(one(1.44)), vp(one(0.0)), vp(one(0.506)), vp(one(sig)),
                                     nb_radius, 0.01, r_max, ntab, vp(p), vp(bulk))
        msg = lib.sosrt_last_error().decode()
        assert rc == _lib.E_INVALID and "Mie" in msg, (what, rc, msg)
        assert np.all(p == -7.0) and np.all(bulk == -7.0), what
        with pytest.raises(ValueError, match="Mie"):
            solver.mie_ensembles(wl, 1.44 + 0j, 0.506, sig, nb_radius=nb_radius, r_max=r_max, ntab=ntab)
    out = np.full((1, 4), -7.0)
    rc = lib.sosrt_mie_efficiencies(solver._h, 1, vp(one(1.5)), vp(one(0.0)), vp(one(1e6)), vp(out))
    assert rc == _lib.E_INVALID and "cap" in lib.sosrt_last_error().decode() and np.all(out == -7.0)
    with pytest.raises(ValueError):
        solver.mie_efficiencies(1.5 + 0j, -1.0)
    with pytest.raises(ValueError):
        solver.set_phase_table_dev(8, 1)
