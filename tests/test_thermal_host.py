"""Thermal emission (source='thermal'), CPU tier: the three symbols of the C ABI, the NumPy model of the stage
(tests/thermal_np.py) pinned to its two closed forms, its linearity and its pure-scattering limit, the oracle's order loop fed
the model's field, the Planck function, and the checks the Python layer makes before any handle exists.  No GPU."""
import os
import re

import numpy as np
import pytest

import sos_oracle as O
import thermal_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_emission_dev": 7, "sosrt_emission_view_dev": 11, "sosrt_epilogue_emission_dev": 10}


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
    for meth in ("emission_device", "emission_view_device", "epilogue_emission_device"):
        assert callable(getattr(Solver, meth))


# ---- the model -------------------------------------------------------------------------------------------------------------------
N_, L_ = 32, 24


def test_model_isothermal_known_answer():
    c = T.column(O, N_, L_, 0.0, 1.0, 0.0, 0.3, 0.0)          # omega = 0 everywhere
    I0 = T.emission(c, np.ones(L_), 1.0, 1.0)
    a = np.abs(c.mu[:N_ - 1])
    e_up = np.max(np.abs(I0[:, N_:] - 1))
    e_dn = np.max(np.abs(I0[:, :N_ - 1] - (1 - np.exp(-c.tau[:, None] / a))))
    print("isothermal: upward - 1 %.3e, downward - (1 - e^{-tau/a}) %.3e" % (e_up, e_dn))
    assert e_up <= 1e-13 and e_dn <= 1e-13
    assert np.all(I0[:, N_ - 1] == 1) and np.all(I0[:, N_] == 1)
    # the view lanes: the same answer off the grid
    v = T.emission_view(c, np.ones(L_), 1.0, [0.01, 0.377, 1.0], np.arange(L_), 1.0)
    assert np.max(np.abs(v[:, 3:] - 1)) <= 1e-13


def test_model_linear_planck_known_answer():
    c = T.column(O, N_, L_, 0.0, 1.0, 0.0, 0.3, 0.0)
    I0 = T.emission(c, 0.5 + 0.8 * c.tau, 1.0, 1.0)
    a = np.abs(c.mu[:N_ - 1])
    att = 1 - np.exp(-c.tau[:, None] / a)
    e = np.max(np.abs(I0[:, :N_ - 1] - (0.5 * att + 0.8 * (c.tau[:, None] - a * att))))
    print("b = 0.5 + 0.8 tau: downward lanes vs the closed form %.3e" % e)
    assert e <= 1e-13


def test_model_weights_at_small_x():
    x = np.array([0.0, 1e-12, 1e-6, 0.1, 0.2499999, 0.25, 0.3, 5.0, 800.0])
    w0, w1, E = T.linear_weights(x)
    assert w0[0] == 0 and w1[0] == 0
    # the leading terms x / 2 and x / 2 keep their digits where the direct differences have none left
    assert abs(w0[1] / 0.5e-12 - 1) < 1e-11 and abs(w1[1] / 0.5e-12 - 1) < 1e-11
    # the series and the direct form meet at the switch
    assert abs(w0[4] - w0[5]) < 1e-7 and abs(w1[4] - w1[5]) < 1e-7
    # w0 + w1 = 1 - E: a constant source is attenuated exactly
    assert np.max(np.abs(w0 + w1 - (-np.expm1(-x)))) <= 2e-16


@pytest.mark.parametrize("surface", ["specular", "lambertian", "lambertian_readme"])
def test_model_is_linear_in_the_sources(surface):
    c = T.column(O, N_, L_, 0.3, 1.0, 0.2, 0.3, 0.6, surface)
    b1, b2 = T.planck_profile(L_), 0.3 + np.sin(np.arange(L_)) ** 2
    f = lambda b, bs: T.emission(c, b, bs, 0.8)
    lhs = f(2 * b1 + 0.5 * b2, 2 * 1.0 + 0.5 * 0.7)
    rhs = 2 * f(b1, 1.0) + 0.5 * f(b2, 0.7)
    assert np.max(np.abs(lhs - rhs)) <= 1e-14 * np.max(np.abs(rhs))


@pytest.mark.parametrize("surface", ["specular", "lambertian_readme"])
def test_pure_scattering_leaves_the_ground_term_alone(surface):
    c = T.column(O, N_, L_, 0.3, 1.0, 1.0, 0.3, 1.0, surface)    # omega = 1 everywhere: no layer emits
    I0 = T.emission(c, T.planck_profile(L_), 1.3, 0.6)
    assert np.max(np.abs(I0[:, :N_])) <= 1e-15 and np.max(np.abs(I0[:, N_])) <= 1e-15     # (f_atm + f_aer rounds to 1 - 1e-16)
    up = 0.6 * 1.3 * np.exp(-(c.tau[-1] - c.tau)[:, None] / c.mu[N_ + 1:])
    assert np.max(np.abs(I0[:, N_ + 1:] - up)) <= 1e-14


def test_the_aerosol_layer_takes_its_own_coefficient_in_both_sweeps():
    c = T.column(O, N_, L_, 0.0, 1.0, 0.0, 0.3, 0.6)
    eps = T.zone_eps(c)
    z = c.zones[1]
    fa, fr = c.zone_fractions(z)
    assert np.all(eps[:z.r0] == 1) and np.all(eps[z.r1 + 1:] == 1)
    assert np.allclose(eps[z.r0:z.r1 + 1], 1 - 0.6 * fr, rtol=0, atol=1e-16)
    # an isothermal column with an absorbing-and-scattering layer: every layer (t-1, t) with t in the slab emits eps_t per unit
    # of (1 - E) in both sweeps, so the upward field just above the slab and the downward field just below it carry the same deficit
    I0 = T.emission(c, np.ones(L_), 1.0, 1.0)
    j = 5
    a = c.mu[N_ + 1 + j]
    x = (c.tau[z.r1] - c.tau[z.r0 - 1]) / a
    want_dn = (1 - np.exp(-c.tau[z.r0 - 1] / a)) * np.exp(-x) + eps[z.r0] * (1 - np.exp(-x))
    assert abs(I0[z.r1, N_ - 2 - j] - want_dn) <= 1e-14
    want_up = 1.0 * np.exp(-x) + eps[z.r0] * (1 - np.exp(-x))
    assert abs(I0[z.r0 - 1, N_ + 1 + j] - want_up) <= 1e-14


# ---- the oracle's order loop fed the model's field ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SOLVE_CASES, ids=lambda c: "N%d-L%d-%s%s" % (c[0], c[1], c[7], "-2slabs" if c[8] else ""))
def test_oracle_runs_on_the_model_field(case):
    c = T.solve_column_case(O, case)
    L = len(c.tau)
    b = T.planck_profile(L)
    r = O.solve_column(c, literal=False, I1=T.emission(c, b, 1.0))
    print("N=%d L=%d %s: the order loop takes n = %d orders; max I = %.4f, max b = %.4f" % (case[0], case[1], case[7], r.n, r.I.max(), b.max()))
    assert r.n == case[-1]
    assert np.all(np.isfinite(r.I))
    # mu0 does not enter: the same column built at another sun angle
    r2 = O.solve_column(T.solve_column_case(O, case, mu0=0.83), literal=False, I1=T.emission(c, b, 1.0))
    assert r2.n == r.n and np.max(np.abs(r2.I - r.I)) <= 1e-13 * np.max(np.abs(r.I))


def test_the_layer_lowers_the_outgoing_flux():
    """Grey tau* = 1, omega = 0, black ground, a 17-25 km layer of omega = 0.3: the layer lowers the outgoing flux by about 4.5 %
    at tau*_aer = 0.12 and about 10 % at 0.3 (the figures move in the third digit with N and L; this grid gives 4.6 and 10.5 %)."""
    out = []
    for t_aer in (0.0, 0.12, 0.3):
        c = T.column(O, 32, 24, 0.0, 1.0, 0.0, t_aer, 0.3)
        r = O.solve_column(c, literal=False, I1=T.emission(c, T.planck_profile(24), 1.0))
        out.append(T.epilogue_emission(r.I, c.mu, c.N)["flux_up"][0])
    drop = [1 - out[1] / out[0], 1 - out[2] / out[0]]
    print("outgoing flux at tau*_aer = 0, 0.12, 0.3: %.4f %.4f %.4f (2 x: %.4f %.4f %.4f); drops %.2f %% and %.2f %%"
          % (tuple(out) + tuple(2 * x for x in out) + (100 * drop[0], 100 * drop[1])))
    assert 0.04 < drop[0] < 0.05 and 0.095 < drop[1] < 0.11


# ---- the Planck function ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_k", [216.5, 288.0])
def test_planck_integrates_to_stefan_boltzmann(T_k):
    from sosrt import thermal
    lam = np.exp(np.linspace(np.log(0.1), np.log(1000.0), 20001))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    total = np.pi * trapz(thermal.planck_radiance(T_k, lam), lam)
    sigma = 5.670374419e-8
    print("T = %g K: pi int B dlambda / (sigma T^4) - 1 = %.3e" % (T_k, total / (sigma * T_k ** 4) - 1))
    assert abs(total / (sigma * T_k ** 4) - 1) <= 1e-4
    assert abs(thermal.STEFAN_BOLTZMANN / sigma - 1) < 1e-9


def test_planck_value_from_the_constants():
    from sosrt import thermal
    h, c, k = 6.62607015e-34, 299792458.0, 1.380649e-23
    lam = 10e-6
    want = 2 * h * c * c / lam ** 5 / (np.exp(h * c / (lam * k * 300.0)) - 1) * 1e-6      # W m-2 sr-1 um-1: 9.924
    got = thermal.planck_radiance(300.0, 10.0)
    assert abs(got / want - 1) <= 1e-14 and 9.9 < got < 9.95
    assert thermal.planck_radiance([250.0, 300.0], [[10.0], [12.0]]).shape == (2, 2)
    with pytest.raises(ValueError):
        thermal.planck_radiance(0.0, 10.0)


# ---- refusals of the Python layer, before any handle exists ----------------------------------------------------------------------------
PL, BS = np.ones(24), 1.0
OK = dict(source="thermal", planck=PL, planck_surface=BS)
BATCH_REFUSALS = [
    (dict(source="thermal"), "planck"),
    (dict(source="thermal", planck=PL), "planck_surface"),
    (dict(source="thermal", planck_surface=BS), "planck"),
    (dict(OK, planck=np.ones(23)), "shape"),
    (dict(OK, planck=np.ones((2, 24))), "shape"),
    (dict(OK, planck=np.ones((3, 24, 1))), "shape"),
    (dict(OK, planck_surface=np.ones(2)), "planck_surface"),
    (dict(OK, surface_emissivity=np.ones(2)), "surface_emissivity"),
    (dict(OK, azimuths=[0.0]), "m = 0"),
    (dict(OK, azimuths=[0.0], mode_batch=True), "m = 0"),
    (dict(OK, view_mu=[0.5], view_azimuths=[0.0]), "m = 0"),
    (dict(OK, beam="spherical"), "spherical"),
    (dict(OK, first_order="readme"), "readme"),
    (dict(OK, devices=[0, 1]), "devices"),
    (dict(planck=PL), "thermal"),
    (dict(planck_surface=BS), "thermal"),
    (dict(surface_emissivity=0.9), "thermal"),
    (dict(source="solar", planck=PL, planck_surface=BS), "thermal"),
    (dict(source="lunar"), "source"),
    (dict(source=None), "source"),
]
KW = dict(nb_layers=24, nb_angles=32)


@pytest.mark.parametrize("bad,word", BATCH_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_batch_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import dist, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, **KW, **bad)
    assert word in str(ei.value), str(ei.value)


OTHER_REFUSALS = [(dict(source="thermal"), "planck"), (dict(OK, planck=np.ones(23)), "shape"), (dict(OK, beam="spherical"), "spherical"),
                  (dict(planck=PL), "thermal"), (dict(source="lunar"), "source")]


@pytest.mark.parametrize("bad,word", OTHER_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_other_drivers_refuse_before_any_handle(bad, word, monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    calls = [lambda: main.solve_batch_device([0.5, 0.6], 0.3, 0.1, **KW, **bad),
             lambda: main.SOS_Aer_layers([0.5, 0.6], 0.1, [(25, 17, 0.3, 0.9)], **KW, **bad),
             lambda: main.SOS_Aer(**KW, **bad)]
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), str(ei.value)


def test_single_column_driver_refuses_the_readme_first_order(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="readme"):
        main.SOS_Aer(first_order="readme", **KW, **OK)


def test_thermal_module_refuses_before_any_handle(monkeypatch):
    from sosrt import main, thermal
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="shape"):
        thermal.thermal_toa_flux([0.1, 0.2], 0.1, np.ones(23), 1.0, **KW)
    with pytest.raises(ValueError, match="planck_surface"):
        thermal.thermal_forcing([0.1, 0.2], 0.1, np.ones(24), None, **KW)


def test_solar_is_the_default_everywhere():
    import inspect
    from sosrt import main
    for f in (main.SOS_Aer_batch, main.solve_batch_device, main.SOS_Aer_layers, main.SOS_Aer):
        p = inspect.signature(f).parameters
        assert p["source"].default == "solar"
        assert all(p[k].default is None for k in ("planck", "planck_surface", "surface_emissivity"))
