"""Per-level weights in the view stage on the host: the three symbols, the identities the feature rests on
checked with the NumPy models (tests/profile_view_np.py on view_np, profile_np, spherical_view_np, thermal_np), and every
refusal of the Python layer before a handle exists."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import profile_np as P
import profile_view_np as PV
import sos_oracle as O
import spherical_np as S
import spherical_view_np as SV
import thermal_np as T
import view_np as VN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_view_radiance_profile_dev": 12, "sosrt_view_first_order_profile_dev": 12, "sosrt_emission_view_profile_dev": 11}
CASES = {"A": VN.case_A, "B": VN.case_B}


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
    for meth in ("view_radiance_profile_device", "view_first_order_profile_device", "emission_view_profile_device"):
        assert callable(getattr(Solver, meth))


# ---- the weighted columns of the identities ------------------------------------------------------------------------------------
def stepped_gas(c):
    """A cumulative gas profile with two steps: rows 5-15 and the lowest quarter of the column."""
    L = len(c.tau)
    w = np.ones(L)
    w[5:16], w[3 * L // 4:] = 0.5, 0.7
    return np.concatenate(([0.0], np.cumsum(np.diff(c.tau) * (1 / w[1:] - 1))))


@functools.lru_cache(maxsize=None)
def weighted(case, kind):
    """(column, w_atm, w_aer): 'random' = profile_np.random_weights(c, 3) on the case's column, 'gas' = a stepped gas profile
    through profile_np.with_gas (tau carries the gas, one weight for both constituents)."""
    c = CASES[case]()
    if kind == "random":
        return (c,) + P.random_weights(c, 3)
    cg, w = P.with_gas(c, stepped_gas(c))
    return cg, w, w


@functools.lru_cache(maxsize=None)
def weighted_solve(case, kind):
    c, wa, wr = weighted(case, kind)
    I1 = P.first_order_profile(c, S.plane_path(c.tau, c.mu0), wa, wr)
    I, I_last, n = PV.solve_column_last(O, c, wa, wr, I1)
    assert n >= 3
    return I, I1, I_last


# ---- 1. node consistency of the scattered term ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "gas"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_scattered_term_at_the_nodes_is_the_weighted_grid_solve(case, kind):
    """view_np.transport(QUAD_GRID) of the weighted view source built on I - I_last, at the node cosines, is I - I1 of the
    weighted grid solve: 1e-12 of the field maximum on the downward lanes the a4b extrapolation did not rewrite and on the upward
    lanes the blend left alone (measured 3.7e-15 and 3e-16).  With the weights forgotten the same comparison is off by > 0.05."""
    c, wa, wr = weighted(case, kind)
    I, I1, I_last = weighted_solve(case, kind)
    mv, lanes = VN.node_views(c.mu, c.N)
    V = len(mv)
    ref = (I - I1)[:, lanes]
    scale = np.max(np.abs(ref))
    Sv = PV.view_source_profile(c, c.P_atm[lanes], c.P_aer[lanes], I - I_last, wa, wr)
    err = np.abs(VN.transport(c, Sv, mv, VN.QUAD_GRID) - ref) / scale
    rew = VN.rewritten_down(c, lanes[:V])
    up = VN.untouched_up(err)
    print("case %s %s: down %.2e (%d lane-rows untouched), up %.2e on %d of %d lanes"
          % (case, kind, err[:, :V][~rew].max(), (~rew).sum(), err[:, V:][:, up].max(), up.sum(), V))
    assert err[:, :V][~rew].max() < 1e-12
    assert up.sum() >= V // 2 and err[:, V:][:, up].max() < 1e-12
    forgot = np.abs(VN.transport(c, VN.source(c, c.P_atm[lanes], c.P_aer[lanes], I - I_last), mv, VN.QUAD_GRID) - ref) / scale
    assert forgot[:, :V][~rew].max() > 0.05


# ---- 2. node consistency of the first term -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plane", "slant"])
@pytest.mark.parametrize("kind", ["random", "gas"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_first_term_at_the_nodes_is_the_grid_profile_first_order(case, kind, path):
    c, wa, wr = weighted(case, kind)
    L = len(c.tau)
    sigma = S.plane_path(c.tau, c.mu0) if path == "plane" else S.slant_path(c.tau, S.altitudes(L), c.mu0)
    mv, lanes = VN.node_views(c.mu, c.N)
    ref = P.first_order_profile(c, sigma, wa, wr)[:, lanes]
    scale = np.max(np.abs(ref))
    got = PV.view_first_order_profile(c, sigma, c.P0_atm[lanes], c.P0_aer[lanes], mv, wa, wr)
    err = np.max(np.abs(got - ref)) / scale
    print("case %s %s %s: %.2e" % (case, kind, path, err))
    assert err < 1e-13
    ones = np.ones(L)
    unit = PV.view_first_order_profile(c, sigma, c.P0_atm[lanes], c.P0_aer[lanes], mv, ones, ones)
    assert np.array_equal(unit, SV.view_first_order_beam(c, sigma, c.P0_atm[lanes], c.P0_aer[lanes], mv))
    assert np.max(np.abs(unit - ref)) / scale > 0.1          # the weights forgotten


# ---- 3. emission ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emissivity", [None, 0.6])
@pytest.mark.parametrize("kind", ["random", "gas"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_emission_at_the_nodes_is_the_grid_profile_emission(case, kind, emissivity):
    c, wa, wr = weighted(case, kind)
    L = len(c.tau)
    b = T.planck_profile(L)
    mv, lanes = VN.node_views(c.mu, c.N)
    ref = P.emission_profile(c, b, 1.1, wa, wr, emissivity)[:, lanes]
    got = PV.emission_view_profile(c, b, 1.1, mv, wa, wr, emissivity)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("case %s %s: %.2e" % (case, kind, err))
    assert err < 1e-13
    ones = np.ones(L)
    lev = np.arange(L)
    assert np.array_equal(PV.emission_view_profile(c, b, 1.1, mv, ones, ones, emissivity),
                          T.emission_view(c, b, 1.1, mv, lev, emissivity))


# ---- the constant-w identity at view lanes off the grid ---------------------------------------------------------------------------
OFF_GRID = np.array([0.01, 0.05, 0.33, 0.6, 0.871, 1.0])     # 0.6 is mu0 of both cases: the phi(0) branch


@pytest.mark.parametrize("case", ["A", "B"])
def test_constant_weight_is_the_scaled_albedo_column_at_view_lanes(case):
    """w == 0.8 on tau / 0.8 against profile_np.stretched(c, 0.8) through the unweighted view_np / spherical_view_np models, at
    view cosines off the grid: 1e-12 of the maximum for the first term and for the scattered term (profile_np measured 5.5e-16
    for the same identity on the grid)."""
    w = 0.8
    c = CASES[case]()
    L = len(c.tau)
    cs = P.stretched(c, w)
    cw = dataclasses.replace(c, tau=c.tau / w, tauStar_tot=c.tauStar_tot / w)
    wv = np.full(L, w)
    sigma = S.plane_path(cw.tau, c.mu0)
    sgn = VN.signed(OFF_GRID)
    fa, fr = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7 if case == "A" else 0.6)
    p0a, p0r = VN.phase_p0_rows(fa, c.mu, c.mu0, sgn)[0], VN.phase_p0_rows(fr, c.mu, c.mu0, sgn)[0]
    got = PV.view_first_order_profile(cw, sigma, p0a, p0r, OFF_GRID, wv, wv)
    ref = SV.view_first_order_beam(cs, sigma, p0a, p0r, OFF_GRID)
    e1 = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    rows_a, rows_r = VN.phase_rows(fa, c.mu, sgn), VN.phase_rows(fr, c.mu, sgn)
    Isrc = P.first_order_profile(cw, sigma, wv, wv)              # a field of the column's own shape
    e2 = 0.0
    for quad in (VN.QUAD_GRID, VN.QUAD_LINEAR):
        got = VN.transport(cw, PV.view_source_profile(cw, rows_a, rows_r, Isrc, wv, wv), OFF_GRID, quad)
        ref = VN.transport(cs, VN.source(cs, rows_a, rows_r, Isrc), OFF_GRID, quad)
        e2 = max(e2, np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print("case %s constant w: first term %.2e, scattered %.2e" % (case, e1, e2))
    assert e1 < 1e-12 and e2 < 1e-12


def test_weights_reach_their_own_rows_of_the_view_source():
    """A weight moves its own row of the view source and nothing else; a row of weight 0 has a source of exactly +0."""
    c = CASES["A"]()
    L = len(c.tau)
    sgn = VN.signed(OFF_GRID)
    rows_a, rows_r = VN.phase_rows(VN.phase_fn("rayleigh"), c.mu, sgn), VN.phase_rows(VN.phase_fn("hg", 0.7), c.mu, sgn)
    Isrc = O.first_order(c)
    ones = np.ones(L)
    base = PV.view_source_profile(c, rows_a, rows_r, Isrc, ones, ones)
    assert np.max(np.abs(base - VN.source(c, rows_a, rows_r, Isrc))) <= 4e-16 * np.max(np.abs(base))
    z = c.zones[1]
    wa = ones.copy(); wa[3] = 0.5; wa[z.r0] = 0.0
    wr = ones.copy(); wr[z.r0] = 0.0
    got = PV.view_source_profile(c, rows_a, rows_r, Isrc, wa, wr)
    assert list(np.flatnonzero(np.any(got != base, axis=1))) == [3, z.r0]
    assert np.all(got[z.r0] == 0) and not np.any(np.signbit(got[z.r0]))


def test_float64_holds_the_entry_bound_at_the_cap():
    """tests/test_gpu_profile_view.py compares the three entries at L = 1024 with the float64 models: their distance from their own
    long double evaluation stays under a tenth of the bound of 1e-12 (profile_view_cases.float64_gaps; measured 1.3e-14 .. 4.8e-14)."""
    import profile_view_cases as C
    gaps = C.float64_gaps()
    assert len(gaps) == 6
    for model, gap in gaps:
        print("%-70s %.1e" % (model, gap))
        assert gap <= 1e-13, (model, gap)


# ---- refusals of the Python layer, before any handle exists ---------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
GAS = np.linspace(0, 0.2, 24)
VIEW = dict(view_mu=[0.5], gas_view=True)
GAS_VIEW_REFUSALS = [
    (dict(view_azimuths=[0.0]), "view_azimuths"),
    (dict(azimuths=[0.0]), "azimuths"),
    (dict(mode_batch=True), "mode_batch"),
    (dict(surface="brdf", brdf="lambertian"), "brdf"),
    (dict(delta_m=8), "delta_m"),
    (dict(first_order="readme"), "readme"),
    (dict(save_orders=True), "save_orders"),
    (dict(devices=[0, 1]), "devices"),
]


def _no_handle(monkeypatch):
    from sosrt import dist, forcing, main
    for mod in (main, forcing):
        monkeypatch.setattr(mod, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))


@pytest.mark.parametrize("bad,word", GAS_VIEW_REFUSALS, ids=[w for _, w in GAS_VIEW_REFUSALS])
def test_gas_view_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import main
    _no_handle(monkeypatch)
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, **VIEW, **KW, **bad)
    assert "gas_tau" in str(ei.value) and word in str(ei.value), str(ei.value)


def test_gas_view_needs_gas_tau_and_view_mu(monkeypatch):
    from sosrt import main
    _no_handle(monkeypatch)
    with pytest.raises(ValueError, match="gas_view=True belongs to gas_tau"):
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_view=True, **KW)
    with pytest.raises(ValueError, match="gas_view=True belongs to gas_tau"):
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, view_mu=[0.5], gas_view=True, **KW)
    with pytest.raises(ValueError, match="give view_mu"):
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, gas_view=True, **KW)
    with pytest.raises(ValueError, match="gas_view must be True or False"):
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, view_mu=[0.5], gas_view="yes", **KW)


def test_without_the_keyword_the_old_refusal_and_its_wording_stand(monkeypatch):
    from sosrt import main
    _no_handle(monkeypatch)
    for kw in (dict(), dict(gas_view=False)):
        with pytest.raises(ValueError) as ei:
            main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, view_mu=[0.5], **KW, **kw)
        assert str(ei.value) == ("gas_tau is not available with view_mu / view_azimuths: the view stage evaluates one scattering "
                                 "coefficient per zone")


def test_the_view_stage_keeps_its_own_refusals_under_gas_view(monkeypatch):
    from sosrt import main
    _no_handle(monkeypatch)
    call = lambda **kw: main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, **VIEW, **KW, **kw)
    with pytest.raises(ValueError, match="aer_set"):
        call(aer_set=[0, 0, 0], aer_phase_fun=["hg", "iso"])
    with pytest.raises(ValueError, match="named phase functions"):
        call(P0_atm=np.ones(64))
    with pytest.raises(ValueError, match="specular"):
        call(surface="lambertian")
    with pytest.raises(ValueError, match="beam='spherical' is not available with view_mu"):
        call(beam="spherical")                               # (the sphere's views need beam_stages=True, with gas as without)
    with pytest.raises(ValueError, match="view_mu must be finite cosines"):
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, gas_tau=GAS, view_mu=[0.001], gas_view=True, **KW)
    with pytest.raises(ValueError, match="view_levels"):
        call(view_levels=[24])


def test_gas_view_is_off_by_default():
    import inspect
    from sosrt import main
    assert inspect.signature(main.SOS_Aer_batch).parameters["gas_view"].default is False
    assert inspect.signature(main._gas_args).parameters["gas_view"].default is False
    assert inspect.signature(main.view_radiance).parameters["profile"].default is False
    assert inspect.signature(main.solve_profile).parameters["post"].default is None
