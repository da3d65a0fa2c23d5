"""Band integration (sosrt.bands), CPU tier: the two symbols of the C ABI, the NumPy model of the Planck stage
(tests/bands_np.py) against quadrature and the Stefan-Boltzmann law, the finding that makes the stage normalise its source (the
order loop is not scale-invariant), the model of the reduce stage, and the checks the Python layer makes before any handle
exists.  No GPU."""
import os
import re

import numpy as np
import pytest

import bands_np as M
import sos_oracle as O
import thermal_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_planck_bands_dev": 11, "sosrt_band_reduce_dev": 9}


def test_symbols_declared_bound_and_exported():
    from sosrt import _lib
    from sosrt.solver import Solver
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    L = _lib.lib()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in sosrt.h" % name
        assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
        assert getattr(L, name) is not None, "%s is not exported" % name
        declared = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert len(_lib.SIGNATURES[name][1]) == declared == nargs, name
    for meth in ("planck_bands_device", "band_reduce_device"):
        assert callable(getattr(Solver, meth))


# ---- the Planck model ------------------------------------------------------------------------------------------------------------
def test_model_against_gauss_legendre_quadrature():
    worst = 0.0
    for t in M.LW_TEMPERATURES:
        for lo, hi in M.LW_BANDS:
            got, ref = float(M.planck_band(t, lo, hi)), M.planck_band_quadrature(t, float(lo), float(hi))
            worst = max(worst, abs(got / ref - 1))
    print("sixteen bands x four temperatures: closed forms vs 64-node Gauss-Legendre %.3e" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("t", M.LW_TEMPERATURES)
def test_model_integrates_to_stefan_boltzmann(t):
    total = np.pi * float(M.planck_band(t, 0.0, 1e6))
    print("T = %g K: pi B(0, 1e6) / (sigma T^4) - 1 = %.3e" % (t, total / (M.SIGMA * t ** 4) - 1))
    assert abs(total / (M.SIGMA * t ** 4) - 1) <= 1e-13
    assert abs(M.SIGMA / 5.670374419e-8 - 1) < 1e-9


def test_the_three_forms_meet_at_the_split():
    # G at x = 1 from below (pi^4/15 - S) and from above (the sum of exponentials)
    assert abs((M.G0 - float(M.S(1.0))) / float(M.G_tail(1.0)) - 1) <= 1e-14
    t = 288.0
    nu1 = t / M.C2                                               # x = 1
    d = 1e-12                                                    # an edge moved across the split changes the form, not the value
    for lo, hi in ((0.5 * nu1, nu1), (nu1, 2 * nu1)):
        a = float(M.planck_band(t, lo * (1 - d) if lo == nu1 else lo, hi * (1 - d) if hi == nu1 else hi))
        b = float(M.planck_band(t, lo * (1 + d) if lo == nu1 else lo, hi * (1 + d) if hi == nu1 else hi))
        # (the band itself moves by 1e-12 of an edge: B_nu dnu / B ~ 1e-11)
        assert abs(a / b - 1) <= 5e-11
    # the three forms on one band cut in two at the split: below + mixed-or-above pieces add up
    whole = float(M.planck_band(t, 0.3 * nu1, 3 * nu1))
    parts = float(M.planck_band(t, 0.3 * nu1, 0.999 * nu1)) + float(M.planck_band(t, 0.999 * nu1, 1.5 * nu1)) + \
        float(M.planck_band(t, 1.5 * nu1, 3 * nu1))
    assert abs(parts / whole - 1) <= 1e-14


def test_narrow_bands_lose_digits_within_the_cancellation_bound():
    # A band of width dnu at nu is a difference of two values of G (or S) that agree to dnu / nu.  The bar is that cancellation's
    # own, eps = 2^-52, not a measured figure:
    #   the edges: x = (c2 nu) / T carries two roundings, <= eps relative, and G' = -g moves the value by g x eps per edge, against a
    #     difference g dx: 2 eps nu / dnu for the two edges;
    #   the two values, each taken to be within 4 eps of exact: 8 eps G / (g dx), where G / g <= 1.2 for x >= 1 (G = g (1 + 3/x +
    #     6/x^2 + ..) (1 - e^-x)) and S / (g x) = 1/3 below it, so <= 9.6 eps nu / dnu.
    # Together 12 eps nu / dnu for every case (6.7e-10 at 2500 cm^-1 and 0.01 cm^-1); DESIGN section 19 quotes the measured worst.
    eps = 2.0 ** -52
    for width in (1.0, 0.01):
        worst = 0.0
        for t in (216.5, 288.0):
            for nu in (100.0, 667.0, 1000.0, 2500.0):
                err = abs(float(M.planck_band(t, nu, nu + width)) / M.planck_band_quadrature(t, nu, nu + width) - 1)
                bar = 12 * eps * (nu + width) / width
                print("T %g K, %g + %g cm^-1: %.3e (bar %.3e)" % (t, nu, width, err, bar))
                assert err <= bar
                worst = max(worst, err)
        print("width %g cm^-1: worst %.3e" % (width, worst))


def test_package_planck_band_equals_the_model():
    from sosrt import bands
    t = np.array(M.LW_TEMPERATURES)[:, None]
    lo, hi = np.array(M.LW_BANDS, dtype=float).T
    assert np.array_equal(bands.planck_band(t, lo, hi), M.planck_band(t, lo, hi))
    assert bands.planck_band(288.0, 0.0, 1e6) == float(M.planck_band(288.0, 0.0, 1e6))
    for bad in ((0.0, 10.0, 20.0), (288.0, 20.0, 20.0), (288.0, -1.0, 20.0), (288.0, 10.0, np.inf)):
        with pytest.raises(ValueError):
            bands.planck_band(*bad)
    lo, hi = bands.wavenumber_bands([4.0, 5.0, 10.0, 20.0])
    assert np.allclose(lo, [2000.0, 1000.0, 500.0]) and np.allclose(hi, [2500.0, 2000.0, 1000.0])
    with pytest.raises(ValueError):
        bands.wavenumber_bands([4.0, 4.0])


def test_model_normalisation():
    Tp = M.temperature_profile(M.L_)
    lo, hi = np.array([p[0] for p in M.THERMAL_POINTS]), np.array([p[1] for p in M.THERMAL_POINTS])
    raw, raw_s, one = M.planck_bands([Tp, Tp - 5.0], [M.T_SURFACE, 300.0], lo, hi, False)
    b, bs, scale = M.planck_bands([Tp, Tp - 5.0], [M.T_SURFACE, 300.0], lo, hi, True)
    assert raw.shape == (5, 2, M.L_) and raw_s.shape == scale.shape == (5, 2) and np.all(one == 1)
    assert np.all(np.maximum(b.max(axis=2), bs) == 1.0)
    assert np.max(np.abs(b * scale[:, :, None] / raw - 1)) <= 4e-16 and np.max(np.abs(bs * scale / raw_s - 1)) <= 4e-16
    assert np.array_equal(scale, np.maximum(raw.max(axis=2), raw_s))


# ---- the finding: the order loop is not scale-invariant ---------------------------------------------------------------------------
def _point_column(point, with_layer=True):
    _, _, t_atm, w_atm, t_aer, w_aer, _, _ = point
    return T.column(O, M.N_, M.L_, M.RHO, t_atm, w_atm, t_aer if with_layer else 0.0, w_aer)


def _point_source(point, normalise):
    b, bs, scale = M.planck_bands(M.temperature_profile(M.L_), M.T_SURFACE, [point[0]], [point[1]], normalise)
    return b[0, 0], float(bs[0, 0]), float(scale[0, 0])


def test_the_order_loop_is_not_scale_invariant():
    point = M.THERMAL_POINTS[3]                                  # 980-1080 cm^-1 on thermal_np's first solve case
    assert point[2:6] == T.SOLVE_CASES[0][3:7] and (M.N_, M.L_, M.RHO) == T.SOLVE_CASES[0][:3]
    c = _point_column(point)
    b, bs, _ = _point_source(point, False)
    print("980-1080 cm^-1: the source in W m-2 sr-1 has the maximum %.4f" % max(b.max(), bs))
    with pytest.raises(IndexError):
        O.solve_column(c, literal=False, I1=T.emission(c, b, bs))
    b, bs, _ = _point_source(point, True)
    assert O.solve_column(c, literal=False, I1=T.emission(c, b, bs)).n == 7


def test_the_points_of_the_table_on_the_normalised_source():
    """Order counts with and without the layer, the band-summed outgoing flux and the forcing, from the oracle."""
    olr = np.zeros(2)
    for point in M.THERMAL_POINTS:
        b, bs, scale = _point_source(point, True)
        for j, with_layer in enumerate((True, False)):
            c = _point_column(point, with_layer)
            r = O.solve_column(c, literal=False, I1=T.emission(c, b, bs))
            assert r.n == point[6 + j], (point, with_layer, r.n)
            olr[j] += scale * T.epilogue_emission(r.I, c.mu, c.N)["flux_up"][0]
    print("band-summed outgoing flux: %.4f with the layer, %.4f without; forcing %.4f" % (olr[0], olr[1], olr[1] - olr[0]))
    assert abs(olr[0] / M.OLR_WITH - 1) <= 1e-4 and abs(olr[1] / M.OLR_WITHOUT - 1) <= 1e-4
    assert abs((olr[1] - olr[0]) - 1.7092) <= 2e-4


# ---- the reduce model --------------------------------------------------------------------------------------------------------------
def test_fma_rounds_once():
    a, b = 1 + 2.0 ** -30, 1 - 2.0 ** -30                        # a b = 1 - 2^-60 exactly
    assert a * b - 1 == 0 and M.fma(a, b, -1.0) == -2.0 ** -60
    assert M.fma(0.1, 3.0, 0.2) == float(np.float64(np.longdouble(0.1) * 3 + np.longdouble(0.2)))


def test_reduce_model_order_and_split():
    rng = np.random.default_rng(7)
    K, C, Mm = 5, 3, 7
    x = rng.standard_normal((K, C, Mm)) * 10.0 ** rng.integers(-3, 4, (K, C, Mm))
    w, s = rng.uniform(0.1, 2, (K, C)), rng.uniform(1, 30, (K, C))
    one = M.band_reduce(x, w, s)
    # ascending k, one fma per point: spelled out for one element
    acc = 0.0
    for k in range(K):
        acc = M.fma(w[k, 1] * s[k, 1], x[k, 1, 4], acc)
    assert one[1, 4] == acc
    # within 1e-15 of the sum of magnitudes of the sum in extended precision
    ld = np.sum((w * s).astype(np.longdouble)[:, :, None] * x.astype(np.longdouble), axis=0)
    mag = np.sum(np.abs((w * s)[:, :, None] * x), axis=0)
    assert np.all(np.abs(one - ld.astype(np.float64)) <= 1e-15 * mag)
    # the order matters in the last bits, so it is part of the definition
    assert not np.array_equal(one, M.band_reduce(x[::-1], w[::-1], s[::-1]))
    # a split with accumulate equals one pass, bit for bit
    for cut in (1, 2, 4):
        two = M.band_reduce(x[cut:], w[cut:], s[cut:], out=M.band_reduce(x[:cut], w[:cut], s[:cut]))
        assert np.array_equal(one, two)
    each = None
    for k in range(K):
        each = M.band_reduce(x[k:k + 1], w[k:k + 1], s[k:k + 1], out=each)
    assert np.array_equal(one, each)
    # NULL weight and NULL scale stand for ones
    assert np.array_equal(M.band_reduce(x), M.band_reduce(x, np.ones((K, C)), np.ones((K, C))))


# ---- refusals of the Python layer, before any handle exists -------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
BANDS = (np.array([350.0, 630.0, 820.0]), np.array([500.0, 700.0, 980.0]))
TEMP = M.temperature_profile(24)
TH_OK = dict(tauStar_atm=[2.0, 4.0, 0.3], alb_atm=0.0, alb_aer=0.5)
THERMAL_REFUSALS = [
    (dict(want=("flux_up", "diffusivity")), "ratio"),
    (dict(want=("flux_sideways",)), "want"),
    (dict(want=()), "want"),
    (dict(beam="spherical"), "spherical"),
    (dict(azimuths=[0.0]), "azimuths"),
    (dict(view_azimuths=[0.0]), "azimuths"),
    (dict(devices=[0, 1]), "devices"),
    (dict(first_order="readme"), "readme"),
    (dict(tauStar_atm=[2.0, 4.0]), "broadcast"),
    (dict(alb_aer=np.ones((2, 2))), "broadcast"),
    (dict(weights=np.ones((3, 2, 1))), "per-point"),
    (dict(surface_emissivity=np.ones((2, 2))), "per-column"),
    (dict(bands=(np.array([350.0, 700.0, 820.0]), np.array([500.0, 700.0, 980.0]))), "nu_hi <= nu_lo"),
    (dict(bands=(np.array([350.0, -1.0, 820.0]), np.array([500.0, 700.0, 980.0]))), "finite"),
    (dict(bands=np.ones(3)), "bands"),
    (dict(temperature=np.ones(23) * 250), "temperature"),
    (dict(temperature=np.where(np.arange(24) == 3, 0.0, TEMP)), "> 0 K"),
    (dict(surface_temperature=-1.0), "> 0 K"),
    (dict(points_per_solve=0), "points_per_solve"),
]


def _no_handle(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))


@pytest.mark.parametrize("bad,word", THERMAL_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_band_thermal_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import bands
    _no_handle(monkeypatch)
    kw = dict(TH_OK, **KW)
    pos = dict(bands=BANDS, temperature=TEMP, surface_temperature=288.0, tauStar_aer=0.1, grd_alb=0.1)
    for k, v in bad.items():
        (pos if k in pos else kw)[k] = v
    with pytest.raises(ValueError) as ei:
        bands.band_thermal(pos["bands"], pos["temperature"], pos["surface_temperature"], pos["tauStar_aer"], pos["grd_alb"], **kw)
    assert word in str(ei.value), str(ei.value)


def test_columns_that_disagree_are_refused(monkeypatch):
    from sosrt import bands
    _no_handle(monkeypatch)
    with pytest.raises(ValueError, match="broadcast"):
        bands.band_thermal(BANDS, TEMP, [288.0, 290.0], np.ones((3, 4)) * 0.1, 0.1, **TH_OK, **KW)
    with pytest.raises(ValueError, match="broadcast"):
        bands.band_thermal(BANDS, np.tile(TEMP, (3, 1)), [288.0, 290.0], 0.1, 0.1, **TH_OK, **KW)
    with pytest.raises(ValueError, match="broadcast"):
        bands.band_solar([1.0, 2.0], [0.5, 0.8], np.ones((2, 3)) * 0.1, 0.1, tauStar_atm=0.1, alb_atm=1.0, alb_aer=0.9, **KW)


SOLAR_REFUSALS = [
    (dict(want=("diffusivity",)), "ratio"),
    (dict(beam="spherical"), "spherical"),
    (dict(azimuths=[0.0]), "azimuths"),
    (dict(view_azimuths=[0.0]), "azimuths"),
    (dict(devices=[0]), "devices"),
    (dict(first_order="readme"), "readme"),
    (dict(tauStar_atm=[0.1, 0.2, 0.3]), "broadcast"),
    (dict(solar_flux=1.0), "solar_flux"),
    (dict(beam_norm="other"), "beam_norm"),
    (dict(aer_phase_fun=["hg"] * 65, point_aerosol=[0, 1]), "MAX_PHASE_SETS"),
    (dict(aer_phase_fun=["hg", "iso"]), "point_aerosol"),
    (dict(aer_phase_fun=["hg", "iso"], point_aerosol=[0, 2]), "point_aerosol"),
    (dict(aer_phase_fun=["hg", "iso"], point_aerosol=[0, 1, 1]), "point_aerosol"),
    (dict(point_aerosol=[0, 1]), "point_aerosol"),
]


@pytest.mark.parametrize("bad,word", SOLAR_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_band_solar_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import bands
    _no_handle(monkeypatch)
    kw = dict(tauStar_atm=[0.5, 0.124], alb_atm=1.0, alb_aer=0.95, **KW)
    flux = bad.get("solar_flux", [0.4, 0.6])
    kw.update({k: v for k, v in bad.items() if k != "solar_flux"})
    with pytest.raises(ValueError) as ei:
        bands.band_solar(flux, [0.5, 0.8], 0.1, 0.1, **kw)
    assert word in str(ei.value), str(ei.value)


def test_forcing_drivers_refuse_before_any_handle(monkeypatch):
    from sosrt import bands
    _no_handle(monkeypatch)
    with pytest.raises(ValueError, match="spherical"):
        bands.band_thermal_forcing(BANDS, TEMP, 288.0, 0.1, 0.1, beam="spherical", **TH_OK, **KW)
    with pytest.raises(ValueError, match="nu_hi <= nu_lo"):
        bands.band_thermal_forcing((BANDS[1], BANDS[0]), TEMP, 288.0, 0.1, 0.1, **TH_OK, **KW)
    with pytest.raises(ValueError, match="want"):
        bands.band_thermal_forcing(BANDS, TEMP, 288.0, 0.1, 0.1, want=("flux_up",), **TH_OK, **KW)
    with pytest.raises(ValueError, match="readme"):
        bands.band_solar_forcing([0.4, 0.6], 0.5, 0.1, 0.1, tauStar_atm=0.1, alb_atm=1.0, alb_aer=0.9, first_order="readme", **KW)
    with pytest.raises(ValueError, match="broadcast"):
        bands.band_solar_forcing([0.4, 0.6], 0.5, [0.1, 0.2, 0.3], 0.1, tauStar_atm=0.1, alb_atm=1.0, alb_aer=0.9, **KW)


def test_default_points_per_solve_rule():
    from sosrt import bands
    field = lambda C, L, N: C * L * 2 * N * 8
    assert bands._points_per_solve(None, 16, 32, 200, 128) == 16                    # 16 x 13 MB fit 1 GiB
    assert bands._points_per_solve(None, 100, 32, 200, 128) == bands.BAND_FIELD_BYTES // field(32, 200, 128) == 81
    assert bands._points_per_solve(None, 4, 4096, 800, 501) == 1                    # one point is already more: still one
    assert bands._points_per_solve(3, 16, 1, 24, 32) == 3 and bands._points_per_solve(99, 16, 1, 24, 32) == 16
