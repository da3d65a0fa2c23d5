"""Channel radiances and brightness temperatures in the band drivers, CPU tier: the new symbol of the C ABI,
the host form of the brightness iteration (`bands.brightness_temperature`) on its round trip, its NaN cases and against the model
(tests/band_view_np.py), and the checks the drivers make before any handle exists.  No GPU."""
import dataclasses
import os
import re

import numpy as np
import pytest

import band_view_np as V
import bands_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12          # T_b relative: d ln B / d ln T >= 1, and f is evaluated to about 1e-14 for bands of 10 cm^-1 and more

# (nu_lo, nu_hi, weights or None): the cases the iteration was tried on
CASES = {
    "window": ([800.0], [1000.0], None),
    "five longwave bands": ([10.0, 350.0, 700.0, 1080.0, 1800.0], [350.0, 700.0, 1080.0, 1800.0, 2500.0], None),
    "three sub-bands with a response": ([660.0, 670.0, 680.0], [670.0, 680.0, 690.0], [0.25, 0.5, 0.25]),
    "four g-points of one band": ([600.0] * 4, [700.0] * 4, [0.4, 0.3, 0.2, 0.1]),
    "shortwave edge": ([2400.0], [2800.0], None),
    "far infrared": ([10.0], [50.0], None),
    "all of it": ([0.0], [1e5], None),
}


def temperatures():
    rng = np.random.default_rng(31)
    return np.concatenate((rng.uniform(160.0, 340.0, 3000), rng.uniform(60.0, 6000.0, 1000), [60.0, 160.0, 250.0, 288.0, 340.0, 3000.0, 6000.0]))


def channel_radiance(T, lo, hi, w):
    w = np.ones(len(lo)) if w is None else np.asarray(w, dtype=float)
    return sum(w[k] * M.planck_band(T, lo[k], hi[k]) for k in range(len(lo)))


def test_symbol_declared_bound_and_exported():
    from sosrt import _lib
    from sosrt.solver import Solver
    name, nargs = "sosrt_brightness_temperature_dev", 9
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "%s is not declared in sosrt.h" % name
    assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
    assert getattr(_lib.lib(), name) is not None
    declared = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    assert len(_lib.SIGNATURES[name][1]) == declared == nargs
    assert callable(getattr(Solver, "brightness_temperature_device"))
    assert "#define SOSRT_VERSION 105" in header


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip(case):
    from sosrt import bands
    lo, hi, w = CASES[case]
    T = temperatures()
    assert T.size == 4007
    Tb, its = bands.brightness_temperature(channel_radiance(T, lo, hi, w), lo, hi, w, return_iterations=True)
    err = np.max(np.abs(Tb / T - 1))
    print("%s: round trip %.3e, iterations max %d mean %.2f" % (case, err, its.max(), its.mean()))
    assert np.all(np.isfinite(Tb)) and its.max() <= 40 and its.min() >= 1
    assert err <= BAR


def test_monotone_in_the_radiance():
    from sosrt import bands
    lo, hi, w = CASES["three sub-bands with a response"]
    R = np.sort(channel_radiance(temperatures(), lo, hi, w))
    R = R[np.concatenate(([True], np.diff(R) > 1e-9 * R[1:]))]
    Tb = bands.brightness_temperature(R, lo, hi, w)
    assert np.all(np.diff(Tb) > 0)


def test_nan_cases():
    from sosrt import bands
    lo, hi = [630.0, 820.0], [700.0, 980.0]
    good = float(channel_radiance(np.array(260.0), lo, hi, None))
    top = float(channel_radiance(np.array(1e5), lo, hi, None))
    R = np.array([good, 0.0, -1.0, np.nan, np.inf, -np.inf, 2 * top, top, good])
    Tb = bands.brightness_temperature(R, lo, hi)
    assert abs(Tb[0] / 260.0 - 1) <= BAR and Tb[8] == Tb[0] and np.all(np.isnan(Tb[1:8]))
    assert np.isnan(bands.brightness_temperature(good, lo, hi, [0.0, 0.0]))
    assert np.isnan(bands.brightness_temperature(good, lo, hi, [1.0, -1e-3]))
    # per-element weights: only the element with the bad weights is NaN
    w = np.array([[1.0, 0.0, 1.0], [1.0, 0.0, -1.0]])
    Tb = bands.brightness_temperature(np.full(3, good), lo, hi, w)
    assert Tb[0] == bands.brightness_temperature(good, lo, hi) and np.isnan(Tb[1]) and np.isnan(Tb[2])
    # a zero among positive weights is a band left out, not an error
    one = bands.brightness_temperature(float(M.planck_band(260.0, 630.0, 700.0)), lo, hi, [1.0, 0.0])
    assert abs(one / 260.0 - 1) <= BAR
    for bad in (([630.0], [630.0]), ([-1.0], [10.0]), ([10.0], [np.inf]), ([10.0, 20.0], [30.0])):
        with pytest.raises(ValueError):
            bands.brightness_temperature(good, *bad)
    with pytest.raises(ValueError, match="broadcast"):
        bands.brightness_temperature(np.ones(3), lo, hi, np.ones((2, 4)))


def test_g_points_of_one_band_give_the_band():
    from sosrt import bands
    lo, hi, w = CASES["four g-points of one band"]
    assert abs(sum(w) - 1.0) <= 2.0 ** -52
    T = temperatures()[::8]
    R = M.planck_band(T, 600.0, 700.0)
    a, b = bands.brightness_temperature(R, lo, hi, w), bands.brightness_temperature(R, 600.0, 700.0)
    assert np.max(np.abs(a / b - 1)) <= BAR and np.max(np.abs(b / T - 1)) <= BAR


def test_package_against_the_model():
    from sosrt import bands
    rng = np.random.default_rng(5)
    worst = 0.0
    for lo, hi, w in CASES.values():
        T = np.concatenate((rng.uniform(150.0, 350.0, 40), [60.0, 3000.0]))
        R = channel_radiance(T, lo, hi, w) * rng.uniform(0.9, 1.1, T.size)       # (not exactly on a temperature of the grid)
        got, its = bands.brightness_temperature(R, lo, hi, w, return_iterations=True)
        ref, its_ref = V.brightness_temperature(R, lo, hi, w, iterations=True)
        assert np.all(np.isfinite(ref)) and max(its.max(), its_ref.max()) <= 40
        worst = max(worst, np.max(np.abs(got / ref - 1)))
    # weights [K, ...] per element, with the NaN cases in place
    lo, hi = np.array([630.0, 820.0, 980.0]), np.array([700.0, 980.0, 1080.0])
    w = rng.uniform(0.2, 2.0, (3, 4, 5))
    w[1, 2, :] = 0.0
    R = np.einsum("kij,kij->ij", w, M.planck_band(rng.uniform(200.0, 300.0, (1, 4, 5)), lo[:, None, None], hi[:, None, None]))
    R[0, 0], R[3, 4] = -1.0, np.nan
    got, ref = bands.brightness_temperature(R, lo, hi, w), V.brightness_temperature(R, lo, hi, w)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).sum() == 2
    ok = np.isfinite(ref)
    worst = max(worst, np.max(np.abs(got[ok] / ref[ok] - 1)))
    print("bands.brightness_temperature against the model: %.3e" % worst)
    assert worst <= BAR


def test_band_result_view_fields_default_to_none():
    from sosrt import bands
    r = bands.BandResult(flux_down=None, flux_up=None, heating_rate=None, net_toa=None, n=np.zeros((1, 1)), status=np.zeros((1, 1)))
    for name in ("view_mu_signed", "I_view_first", "I_view_scattered", "I_view", "brightness_temperature", "point_I_view"):
        assert getattr(r, name) is None
        assert {f.name: f.default for f in dataclasses.fields(r)}[name] is None


# ---- refusals of the drivers, before any handle exists ------------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
BANDS = (np.array([350.0, 630.0, 820.0]), np.array([500.0, 700.0, 980.0]))
TEMP = M.temperature_profile(24)
TH_OK = dict(tauStar_atm=[2.0, 4.0, 0.3], alb_atm=0.0, alb_aer=0.5)
VIEW = dict(view_mu=[0.05, 0.5, 1.0])


def _no_handle(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))


class _Reached(Exception):
    pass


def _handle_reached(monkeypatch):
    from sosrt import main

    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(main, "get_solver", reached)


def _thermal(**kw):
    from sosrt import bands
    args = dict(TH_OK, **KW)
    args.update(kw)
    b = args.pop("bands", BANDS)
    return bands.band_thermal(b, args.pop("temperature", TEMP), 288.0, args.pop("tauStar_aer", 0.1), 0.1, **args)


def _solar(**kw):
    from sosrt import bands
    args = dict(tauStar_atm=[0.5, 0.124], alb_atm=1.0, alb_aer=0.95, **KW)
    args.update(kw)
    return bands.band_solar([0.4, 0.6], [0.5, 0.8], 0.1, 0.1, **args)


K65 = (np.arange(65) * 20.0 + 100.0, np.arange(65) * 20.0 + 120.0)
THERMAL_REFUSALS = [
    (dict(VIEW, surface="lambertian"), "specular"),
    (dict(VIEW, bands=K65, tauStar_atm=1.0), "brightness=False"),
    (dict(VIEW, weights=[1.0, -0.5, 1.0]), "brightness=True needs weights"),
    (dict(VIEW, weights=np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])), "brightness=True needs weights"),
    (dict(VIEW, brightness=1), "brightness must be"),
    (dict(VIEW, view_levels=(0, 24)), "view_levels"),
    (dict(VIEW, view_levels=()), "view_levels"),
    (dict(view_mu=[0.5, 1.5]), "view_mu"),
    (dict(view_mu=[0.001]), "view_mu"),
    (dict(view_mu=[]), "view_mu"),
    (dict(VIEW, view_quadrature="simpson"), "view_quadrature"),
    (dict(VIEW, aer_phase_fun=["hg", "iso"]), "one aerosol phase function"),
    (dict(VIEW, view_azimuths=[0.0]), "azimuths"),
    (dict(VIEW, azimuths=[0.0]), "azimuths"),
    (dict(VIEW, beam="spherical"), "spherical"),
    (dict(VIEW, devices=[0, 1]), "devices"),
    (dict(VIEW, first_order="readme"), "readme"),
    (dict(VIEW, want=("diffusivity",)), "ratio"),
]


@pytest.mark.parametrize("bad,word", THERMAL_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_band_thermal_view_refusals_before_any_handle(bad, word, monkeypatch):
    _no_handle(monkeypatch)
    with pytest.raises(ValueError) as ei:
        _thermal(**bad)
    assert word in str(ei.value), str(ei.value)


SOLAR_REFUSALS = [
    (dict(VIEW, surface="lambertian"), "specular"),
    (dict(VIEW, aer_phase_fun=["hg", "iso"], point_aerosol=[0, 1]), "point_aerosol"),
    (dict(VIEW, view_levels=(-25,)), "view_levels"),
    (dict(view_mu=[2.0]), "view_mu"),
    (dict(VIEW, view_quadrature="simpson"), "view_quadrature"),
    (dict(VIEW, view_azimuths=[0.0]), "azimuths"),
    (dict(VIEW, beam="spherical"), "spherical"),
    (dict(VIEW, brightness=True), None),
]


@pytest.mark.parametrize("bad,word", SOLAR_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_band_solar_view_refusals_before_any_handle(bad, word, monkeypatch):
    _no_handle(monkeypatch)
    if word is None:                                             # the solar driver forms no brightness temperature: no such keyword
        with pytest.raises(TypeError):
            _solar(**bad)
        return
    with pytest.raises(ValueError) as ei:
        _solar(**bad)
    assert word in str(ei.value), str(ei.value)


def test_want_may_be_empty_with_view_mu_only(monkeypatch):
    # with view_mu every check passes and the driver goes on to ask for a handle ..
    _handle_reached(monkeypatch)
    with pytest.raises(_Reached):
        _thermal(want=(), **VIEW)
    with pytest.raises(_Reached):
        _solar(want=(), **VIEW)
    # .. 65 bands and weights with a zero column pass too where no brightness temperature is asked for
    with pytest.raises(_Reached):
        _thermal(bands=K65, tauStar_atm=1.0, brightness=False, **VIEW)
    with pytest.raises(_Reached):
        _thermal(weights=[1.0, -0.5, 1.0], brightness=False, **VIEW)
    with pytest.raises(_Reached):
        _thermal(weights=[1.0, -0.5, 1.0])                       # brightness=True is inert without view_mu
    # .. and without view_mu the refusal stands word for word
    from sosrt import bands
    msg = "want must name some of %s (got %r)" % (bands.WANT, ())
    for call in (_thermal, _solar):
        with pytest.raises(ValueError) as ei:
            call(want=())
        assert str(ei.value) == msg
