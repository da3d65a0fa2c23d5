"""Per-level weights on the source function on the host: the symbols, the NumPy model of tests/profile_np.py
pinned to the oracle by its identities (unit weights, a constant weight, the unit-weight first order and emission), the rule
that turns a gas absorption profile into weights, what a stepped profile does to the column, and every refusal of the Python
layer before a handle exists."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import profile_np as P
import sos_oracle as O
import spherical_np as S
import thermal_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_set_row_weights_dev": 4, "sosrt_first_order_profile_dev": 7, "sosrt_emission_profile_dev": 7}
N_, L_, MU0 = 32, 40, 0.6                 # mu0 is 1.3e-2 from the nearest node: the closed forms' limit branch is not in play


def test_symbols_declared_bound_and_exported():
    from sosrt import _lib
    from sosrt.solver import Solver
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    lib = _lib.lib()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in sosrt.h" % name
        assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
        assert getattr(lib, name) is not None, "%s is not exported" % name
        declared = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert len(_lib.SIGNATURES[name][1]) == declared == nargs, name
    for meth in ("set_row_weights_device", "first_order_profile_device", "emission_profile_device"):
        assert callable(getattr(Solver, meth))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_mu0_is_away_from_the_nodes():
    assert S.node_distance(N_, MU0) > 1e-3


@pytest.mark.parametrize("slabs", [None, S.TWO_SLABS], ids=["three_zones", "five_zones"])
def test_unit_weights_are_the_oracle_bit_for_bit(slabs):
    L = 48 if slabs else L_
    c = P.column(O, N_, L, MU0, 0.3, slabs)
    ones = np.ones(L)
    ref = O.solve_column(c, literal=False)
    got = P.solve_column(O, c, ones, ones, O.first_order(c))
    assert got.n == ref.n
    assert np.array_equal(got.I, ref.I)
    x = ref.I_saved[1]
    assert np.array_equal(P.source_function(O, c, x, ones, ones), O.source_function(c, x))


@pytest.mark.parametrize("slabs", [None, S.TWO_SLABS], ids=["three_zones", "five_zones"])
def test_unit_weight_first_order_is_first_order_beam(slabs):
    L = 48 if slabs else L_
    c = P.column(O, N_, L, MU0, 0.3, slabs)
    ones = np.ones(L)
    for sigma in (S.plane_path(c.tau, MU0), S.slant_path(c.tau, S.altitudes(L), MU0)):
        assert np.array_equal(P.first_order_profile(c, sigma, ones, ones), S.first_order_beam(c, sigma))


@pytest.mark.parametrize("surface", ["specular", "lambertian", "lambertian_readme"])
def test_unit_weight_emission_is_the_emission_model(surface):
    c = T.column(O, N_, 24, 0.2, 1.0, 0.3, surface=surface)
    b, ones = T.planck_profile(24), np.ones(24)
    assert np.array_equal(P.emission_profile(c, b, 1.1, ones, ones), T.emission(c, b, 1.1))


def test_constant_weight_is_the_scaled_albedo_column():
    """w == 0.8 on the column whose optical depths are divided by w is the ordinary oracle solve of the column with both albedos
    times w on those depths.  Fed the same (layer-by-layer) first order the two differ by rounding only: bar 1e-14 of the field
    maximum (measured 5.5e-16), equal order counts.  Against the oracle's own closed-form first order the difference is that of
    the two first orders (1e-14 at this mu0): the bar of the beam stage against its model, 1e-12."""
    w = 0.8
    c = P.column(O, N_, L_, MU0, 0.3)
    cs = P.stretched(c, w)                                     # albedos times w, optical depths over w
    cw = dataclasses.replace(c, tau=c.tau / w, tauStar_tot=c.tauStar_tot / w)
    wv = np.full(L_, w)
    sigma = S.plane_path(cw.tau, MU0)
    got = P.solve_column(O, cw, wv, wv, P.first_order_profile(cw, sigma, wv, wv))
    ref = O.solve_column(cs, literal=False, I1=S.first_order_beam(cs, sigma))
    closed = O.solve_column(cs, literal=False)
    scale = np.max(np.abs(ref.I))
    err = np.max(np.abs(got.I - ref.I)) / scale
    err_closed = np.max(np.abs(got.I - closed.I)) / scale
    print("constant w: orders %d / %d / %d, %.2e of the maximum (closed-form first order: %.2e)" % (got.n, ref.n, closed.n, err, err_closed))
    assert got.n == ref.n == closed.n
    assert err <= 1e-14
    assert err_closed <= 1e-12


def test_constant_weight_emission_is_the_scaled_albedo_emission():
    w = 0.7
    c = T.column(O, N_, 24, 0.2, 1.0, 0.8, 0.3, 0.9)
    b, wv = T.planck_profile(24), np.full(24, w)
    got, ref = P.emission_profile(c, b, 1.1, wv, wv), T.emission(P.scaled(c, w), b, 1.1)
    assert np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref))


def test_weights_are_per_row_and_per_constituent():
    """A weight moves its own row's source and nothing else; w_atm moves a clear row, w_aer does not."""
    c = P.column(O, N_, L_, MU0, 0.3)
    x = O.solve_column(c, literal=False).I_saved[1]
    ones = np.ones(L_)
    base = P.source_function(O, c, x, ones, ones)
    z = c.zones[1]
    wa = ones.copy(); wa[3] = 0.5; wa[z.r0] = 0.25
    got = P.source_function(O, c, x, wa, ones)
    rows = np.flatnonzero(np.any(got != base, axis=1))
    assert list(rows) == [3, z.r0]
    assert np.allclose(got[3], 0.5 * base[3], rtol=1e-15)
    wr = ones.copy(); wr[3] = 0.5; wr[z.r0] = 0.0
    got = P.source_function(O, c, x, ones, wr)
    assert list(np.flatnonzero(np.any(got != base, axis=1))) == [z.r0]
    ca, _ = P.split(c)
    assert np.array_equal(got[z.r0], O.source_function(ca, x)[z.r0])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_gas_rule_weights_lie_in_0_1():
    from sosrt.inputs import gas_row_weights, tau_profile
    rng = np.random.default_rng(7)
    tau0 = np.stack([tau_profile(0.124, t, 120, 25, 17, L_) for t in (0.0, 0.3, 2.0)])
    gas = np.concatenate((np.zeros((3, 1)), np.cumsum(rng.uniform(0, 0.05, (3, L_ - 1)) * (rng.uniform(size=(3, L_ - 1)) > 0.3), axis=1)), axis=1)
    tau, w = gas_row_weights(tau0, gas)
    assert tau.shape == w.shape == (3, L_)
    assert np.all(w > 0) and np.all(w <= 1)
    assert np.array_equal(w[:, 0], w[:, 1])
    assert np.array_equal(tau, tau0 + gas)
    for b in range(3):
        tm, wm = P.gas_weights(tau0[b], gas[b])
        assert np.array_equal(tau[b], tm) and np.array_equal(w[b], wm)
    # [L] broadcasts over the columns
    t1, w1 = gas_row_weights(tau0, gas[0])
    assert np.array_equal(t1[2], tau0[2] + gas[0]) and np.array_equal(w1[0], w[0])


def test_no_gas_gives_ones_and_the_same_grid():
    from sosrt.inputs import gas_row_weights, tau_profile
    tau0 = tau_profile(0.124, 0.3, 120, 25, 17, L_)
    tau, w = gas_row_weights(tau0, np.zeros(L_))
    assert np.array_equal(tau, tau0)
    assert np.array_equal(w, np.ones(L_))


def test_the_rule_recovers_a_constant_weight():
    from sosrt.inputs import gas_row_weights, tau_profile
    tau0 = tau_profile(0.124, 0.3, 120, 25, 17, L_)
    tau, w = gas_row_weights(tau0, tau0 * (1 / 0.8 - 1))
    assert np.allclose(w, 0.8, rtol=0, atol=1e-13)
    assert np.allclose(tau, tau0 / 0.8, rtol=1e-15)


def test_a_stepped_profile_darkens_the_column():
    """Gas in rows 5-15 and 30-39 lowers the upward flux at the top and raises the fraction the column absorbs (atmosphere and
    aerosol themselves conserve: what is absorbed is absorbed by the gas and by the ground)."""
    c = P.column(O, N_, L_, MU0, 0.3, alb_aer=1.0)
    w = np.ones(L_)
    w[5:16], w[30:40] = 0.5, 0.7
    gas = np.concatenate(([0.0], np.cumsum(np.diff(c.tau) * (1 / w[1:] - 1))))
    cg, wg = P.with_gas(c, gas)
    assert np.allclose(wg[1:], w[1:], rtol=0, atol=1e-13)
    ref = O.solve_column(c, literal=False)
    got = P.solve_column(O, cg, wg, wg, P.first_order_profile(cg, S.plane_path(cg.tau, MU0), wg, wg))
    assert got.n <= ref.n
    fd0, fu0 = O.fluxes(ref.I, c.mu, c.tau, N_, MU0, c.grd_alb)
    fd1, fu1 = O.fluxes(got.I, cg.mu, cg.tau, N_, MU0, cg.grd_alb)
    assert fu1[0] < 0.95 * fu0[0]
    absorbed = lambda fd, fu: 1 - fu[0] / -fd[0]               # of the flux that enters at the top
    assert absorbed(fd1, fu1) > absorbed(fd0, fu0) + 0.02


# ---- refusals of the Python layer, before any handle exists ---------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
GAS = np.linspace(0, 0.2, 24)
BATCH_REFUSALS = [
    (dict(azimuths=[0.0]), "azimuths"),
    (dict(view_mu=[0.5]), "view_mu"),
    (dict(view_mu=[0.5], view_azimuths=[0.0]), "view_mu"),
    (dict(azimuths=[0.0], mode_batch=True), "azimuths"),
    (dict(mode_batch=True), "mode_batch"),
    (dict(surface="brdf", brdf="lambertian"), "brdf"),
    (dict(delta_m=8), "delta_m"),
    (dict(first_order="readme"), "readme"),
    (dict(save_orders=True), "save_orders"),
    (dict(devices=[0, 1]), "devices"),
]
SHAPE_REFUSALS = [
    (np.linspace(0, 0.2, 23), "shape"),
    (np.zeros((2, 24)), "shape"),
    (np.zeros((3, 24, 1)), "shape"),
    (np.linspace(0.1, 0.2, 24), "0 at level 0"),
    (np.linspace(0.2, 0, 24) - 0.2, "decrease"),
    (np.where(np.arange(24) == 5, np.nan, GAS), "finite"),
    (np.where(np.arange(24) == 23, np.inf, GAS), "finite"),
    ("ozone", "numbers"),
]


def _no_handle(monkeypatch):
    from sosrt import dist, forcing, main
    for mod in (main, forcing):
        monkeypatch.setattr(mod, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))


@pytest.mark.parametrize("bad,word", BATCH_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_batch_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import main
    _no_handle(monkeypatch)
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, **KW, **bad)
    assert "gas_tau" in str(ei.value) and word in str(ei.value), str(ei.value)


@pytest.mark.parametrize("gas,word", SHAPE_REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(SHAPE_REFUSALS)])
def test_profile_refusals_before_any_handle(gas, word, monkeypatch):
    from sosrt import forcing, main, thermal
    _no_handle(monkeypatch)
    calls = [lambda: main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=gas, **KW),
             lambda: main.solve_batch_device([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=gas, **KW),
             lambda: forcing.toa_net_flux(0.5, 0.124, [0.1, 0.2, 0.3], 0.1, 1.0, 0.9, gas_tau=gas, **KW),
             lambda: thermal.thermal_toa_flux([0.1, 0.2, 0.3], 0.1, np.ones(24), 1.0, gas_tau=gas, **KW)]
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), str(ei.value)


def test_other_drivers_refuse_before_any_handle(monkeypatch):
    from sosrt import bands, forcing, main
    _no_handle(monkeypatch)
    with pytest.raises(ValueError, match="SOS_Aer_layers"):
        main.SOS_Aer_layers([0.5, 0.6], 0.1, [(25, 17, 0.3, 0.9)], gas_tau=GAS, **KW)
    with pytest.raises(ValueError, match="SOS_Aer_spectrum"):
        main.SOS_Aer_spectrum([0.5, 0.6], 0.5, 0.3, 0.1, dict(m=1.5 + 0.01j, r_m=0.2, sig=1.5), gas_tau=GAS, **KW)
    for bad, word in ((dict(delta_m=8), "delta_m"), (dict(first_order="readme"), "readme"), (dict(surface="brdf", brdf="lambertian"), "brdf")):
        with pytest.raises(ValueError) as ei:
            main.SOS_Aer(gas_tau=GAS, **KW, **bad)
        assert "gas_tau" in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(ValueError, match="shape"):
        main.SOS_Aer(gas_tau=np.zeros((2, 24)), **KW)
    for bad, word in ((dict(delta_m=8), "delta_m"), (dict(surface="brdf", brdf="lambertian"), "brdf")):
        with pytest.raises(ValueError) as ei:
            forcing.toa_net_flux(0.5, 0.124, [0.1, 0.2], 0.1, 1.0, 0.9, gas_tau=GAS, **KW, **bad)
        assert "gas_tau" in str(ei.value) and word in str(ei.value), str(ei.value)
    # the band drivers: each spectral point its own profile, [K, L] or [K, C, L]
    bk = dict(tauStar_atm=0.5, alb_atm=0.2, alb_aer=0.9, **KW)
    edges = (np.array([500.0, 700.0]), np.array([700.0, 900.0]))
    for gas, word in ((GAS, "shape"), (np.zeros((3, 24)), "shape"), (np.zeros((2, 2, 23)), "shape"), (np.tile(-GAS, (2, 1)), "decrease")):
        with pytest.raises(ValueError) as ei:
            bands.band_thermal(edges, 250 * np.ones(24), 288.0, 0.3, 0.1, gas_tau=gas, **bk)
        assert word in str(ei.value), str(ei.value)
        with pytest.raises(ValueError) as ei:
            bands.band_solar([1.0, 2.0], 0.5, 0.3, 0.1, gas_tau=gas, **bk)
        assert word in str(ei.value), str(ei.value)
        with pytest.raises(ValueError) as ei:
            bands.band_thermal_forcing(edges, 250 * np.ones(24), 288.0, 0.3, 0.1, gas_tau=gas, **bk)
        assert word in str(ei.value), str(ei.value)
        with pytest.raises(ValueError) as ei:
            bands.band_solar_forcing([1.0, 2.0], 0.5, 0.3, 0.1, gas_tau=gas, **bk)
        assert word in str(ei.value), str(ei.value)


def test_no_gas_is_the_default_everywhere():
    from sosrt import bands, forcing, main, thermal
    for f in (main.SOS_Aer_batch, main.solve_batch_device, main.SOS_Aer_layers, main.SOS_Aer, forcing.toa_net_flux,
              thermal.thermal_toa_flux, bands.band_thermal, bands.band_solar, bands.band_thermal_forcing, bands.band_solar_forcing):
        assert inspect.signature(f).parameters["gas_tau"].default is None, f.__name__
    assert main._gas_args(None, lambda: pytest.fail("the batch width was taken"), 24) is None


def test_float64_holds_the_stage_bound_at_the_profile_cap():
    """tests/test_gpu_stage_shapes.py compares the two profile stage kernels at L = 1024 with the float64 models: their distance
    from their own long double evaluation stays under a tenth of the bound of 1e-12 (stage_shape_cases.profile_float64_gaps)"""
    import stage_shape_cases as C
    gaps = C.profile_float64_gaps()
    assert {shape for _, shape, _ in gaps} == set(C.PROFILE_CAP_L) and len(gaps) == 17
    for model, shape, gap in gaps:
        assert gap <= 1e-13, (model, shape, gap)
