"""Azimuth-resolved radiance over a BRDF ground (brdf_modes=True), CPU tier: the two symbols of the C ABI, the
NumPy model (tests/brdf_azimuth_np.py) -- the series in ground reflections per Fourier mode against a direct azimuth-resolved
solve with a phi-resolved BRDF ground, in the linear regime -- the model's own properties, and the checks the Python layer makes
before any handle exists.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import azimuth_direct as D
import brdf_azimuth_np as BA
import brdf_np as G
import sos_oracle as O
from sosrt import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_brdf_operator_modes_dev": 9, "sosrt_brdf_beam_modes_dev": 10}
RPV = ("rpv", 0.2, 0.8, -0.1)
SCALE = 1e-6


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
    for meth in ("brdf_operator_modes_device", "brdf_beam_modes_device"):
        assert callable(getattr(Solver, meth))


# ---- the mode series against the direct solve, linear regime ---------------------------------------------------------------------
# P0 and the beam row scaled by 1e-6: every blend search stops at its first test (asserted), the blend is a fixed linear map and
# the solve is linear in the sources.  The direct solve on nq = 2 (nphi - 1) nodes has the builders' quadrature, for the phase
# functions and for the BRDF, so its projection on mode m is the mode series to rounding whatever M leaves out.
CASES = {
    # aerosol, g, BRDF, N, L, nq, M, orders, orders of the reflections
    "rayleigh-N16": ("rayleigh", 0.0, ("rpv", 0.3, 0.7, -0.2), 16, 16, 16, 5, 3, (3, 3)),
    "hg-N24": ("hg", 0.5, RPV, 24, 16, 48, 10, 3, (3, 3)),
    "hg-N37": ("hg", 0.5, RPV, 37, 24, 48, 6, 3, (3, 3, 3)),
}


@functools.lru_cache(maxsize=None)
def linear_case(name):
    """(error of the signed series per mode, of the unsigned one, the ground's share of the mode field), in units of
    max |mode 0|"""
    aer, g, brdf, N, L, nq, M, n, nb = CASES[name]
    fa = inputs._scalar_phase("rayleigh")[0]
    fr = fa if aer == "rayleigh" else inputs._scalar_phase(aer, g)[0]
    gr = BA.black_three_zone(0.6, L, N)
    nphi = nq // 2 + 1
    log = BA.BlendLog()
    with D.record_blend() as oracle_log:
        _, Iq = BA.direct_solve(gr, fa, fr, brdf, nq, n, nb, SCALE, log=log)
        Im, status = BA.mode_series(gr, fa, fr, brdf, M, nphi, n, nb, SCALE, brdf_nphi=nphi, log=log)
        log.oracle = oracle_log
    assert status == 0 and log.first_test_everywhere()
    Iu, _ = BA.mode_series(gr, fa, fr, brdf, M, nphi, n, nb, SCALE, brdf_nphi=nphi, sign=False)
    Ib = D.mode_fields(gr.geo, fa, fr, M, nphi, n, SCALE)                    # the atmosphere alone, over the black ground
    ref = D.project(Iq, M)
    mx = np.max(np.abs(ref[0]))
    err = lambda X: np.array([np.max(np.abs(X[m] - ref[m])) for m in range(M + 1)]) / mx
    return err(Im), err(Iu), err(Ib)


@pytest.mark.parametrize("name", list(CASES))
def test_mode_series_is_the_direct_solve(name):
    """Measured: 3.5e-16 (Rayleigh, N = 16), 4.4e-16 (N = 24), 8.7e-16 (N = 37) in every mode; without the (-1)^m on the operator
    mode 1 misses by 1.0e-2 / 1.3e-2 / 1.3e-2 (modes 3, 5: 2e-4, 1.4e-5; the even modes do not see the sign).  The ground's
    share of the mode field: 0.13 (m = 1) .. 6.5e-3 (m = 5) for the first case, 4.1e-2 (m = 1), 2.0e-3 (m = 5), 5.9e-4 (m = 10)
    for the second."""
    signed, unsigned, ground = linear_case(name)
    print("%s: signed %s\n  unsigned %s\n  ground's share %s" % (name, *(" ".join("%.2e" % e for e in x) for x in (signed, unsigned, ground))))
    assert np.max(signed) <= 1e-13
    assert unsigned[1] > 1e-3                                # the comparison tells the two conventions apart
    assert ground[1] > 1e-2                                  # ... and the ground is a visible part of mode 1


# ---- the model's own properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brdf", ["lambertian", RPV], ids=["lambertian", "rpv"])
@pytest.mark.parametrize("N", [16, 37])
def test_mode_zero_is_the_azimuth_mean(N, brdf):
    mu = O.make_mu(N)
    assert np.array_equal(BA.operator_modes(mu, N, brdf, [0])[0], G.operator(mu, N, brdf))
    assert np.array_equal(BA.beam_modes(mu, N, 0.6, brdf, [0])[0], G.beam_row(mu, N, 0.6, brdf))
    assert np.array_equal(BA.operator_modes(mu, N, brdf, [0], 33)[0], G.operator(mu, N, brdf, 33))


@pytest.mark.parametrize("nphi", [9, 65])
def test_the_modes_sum_to_rho_at_the_nodes(nphi):
    """The trapezoid rule on nphi nodes is a cosine transform: rho at node q is sum_{m <= nphi - 2} (2 - delta_m0) rho^m cos(m phi_q)
    plus the Nyquist term rho^{nphi - 1} (-1)^q, which no call asks for (m <= nphi - 2) and the test adds."""
    up = O.make_mu(16)[17:]
    a, b = up[:, None], up[None, :]
    phi = np.linspace(0, np.pi, nphi)
    ms = list(range(nphi))
    rm = BA.rho_modes(RPV, a, b, ms, nphi)
    w = np.where((np.arange(nphi) == 0) | (np.arange(nphi) == nphi - 1), 1.0, 2.0)
    got = np.einsum("mab,mq->abq", rm * w[:, None, None], np.cos(np.outer(ms, phi)))
    ref = G.rho_rpv(a[..., None], b[..., None], phi, *RPV[1:])
    assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(ref)
    assert np.max(np.abs(rm[-1])) > 1e-6 * np.max(ref)       # (the Nyquist term is not nothing)


def test_lambertian_has_no_mode_above_zero():
    mu = O.make_mu(37)
    for nphi in (9, 65, 300):
        ms = list(range(1, min(64, nphi - 2) + 1))
        assert np.max(np.abs(BA.rho_modes("lambertian", mu[38:, None], mu[None, 38:], ms, nphi))) <= 1e-15
        assert np.max(np.abs(BA.operator_modes(mu, 37, "lambertian", ms, nphi))) <= 1e-15


def test_the_modes_are_reciprocal():
    up = O.make_mu(37)[38:]
    rm = BA.rho_modes(RPV, up[:, None], up[None, :], range(0, 17))
    assert np.max(np.abs(rm - np.swapaxes(rm, 1, 2))) <= 1e-12 * np.max(rm[0])


def test_the_rpv_modes_fall_off_slowly():
    """The hot spot is a cusp at phi = 0 on the diagonal a = b: the modes there fall off as 1 / m^2 (measured at 2001 nodes:
    m^2 rho^m within a factor 1.5 over m = 8 .. 32), where a smooth function's would fall exponentially."""
    a = np.array([0.6])
    rm = np.abs(BA.rho_modes(RPV, a, a, [8, 16, 32], 2001)[:, 0])
    scaled = rm * np.array([8, 16, 32]) ** 2
    print("rho^m(0.6, 0.6) at m = 8, 16, 32: %s; m^2 rho^m %s" % (rm, scaled))
    assert scaled.max() <= 1.5 * scaled.min() and rm[2] > 1e-5 * float(BA.rho_modes(RPV, a, a, [0], 2001)[0, 0])


# ---- refusals of the Python layer, before any handle exists ----------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
OK = dict(surface="brdf", brdf=RPV, grd_alb=1.0, azimuths=[0.0, 1.0], brdf_modes=True)
REFUSALS = [
    (dict(brdf_modes=True), "brdf_modes belongs"),
    (dict(brdf_modes=True, azimuths=[0.0]), "brdf_modes belongs"),
    (dict(surface="lambertian", brdf_modes=True, azimuths=[0.0]), "brdf_modes belongs"),
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, brdf_modes=True), "give azimuths"),
    (dict(OK, brdf_modes=1), "True or False"),
    (dict(OK, mode_batch=True), "mode_batch"),
    (dict(OK, mode_batch=True, mode_chunk=2), "mode_batch"),
    (dict(OK, view_mu=[0.5], view_azimuths=[0.0]), "view_azimuths"),
    (dict(OK, view_mu=[0.5]), "view_mu"),
    (dict(OK, brdf=(np.zeros((31, 31)), np.zeros(31))), "no azimuth information"),
    (dict(OK, beam="spherical"), "spherical"),
    (dict(OK, source="thermal", planck=np.ones(24), planck_surface=1.0), "thermal"),
    (dict(OK, first_order="readme"), "readme"),
    (dict(OK, devices=[0, 1]), "devices"),
    (dict(OK, save_orders=True), "save_orders"),
    (dict(OK, grd_alb=0.5), "omitted or 1"),
    (dict(OK, brdf=("rpv", 0.2, 0.8, 1.0)), "|theta| < 1"),
    (dict(OK, n_modes=64, nphi_modes=131), "n_modes must be <= 63"),
    (dict(OK, n_modes=30, nphi_modes=25), "nphi_modes"),
    (dict(OK, P_atm=np.zeros((64, 64))), "named phase functions"),
    (dict(OK, aer_set=[0, 0, 0]), "aer_set"),
    (dict(OK, levels=[24]), "levels"),
    # as before the keyword: azimuths over a BRDF ground without it
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, azimuths=[0.0]), "only the azimuth mean (mode m = 0) of the BRDF is built"),
    (dict(surface="brdf", brdf="lambertian", azimuths=[0.0], mode_batch=True), "only the azimuth mean (mode m = 0) of the BRDF is built"),
    (dict(surface="brdf", brdf="lambertian", view_mu=[0.5], view_azimuths=[0.0]), "only the azimuth mean (mode m = 0) of the BRDF is built"),
]


@pytest.mark.parametrize("bad,word", REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import dist, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    kw = dict(KW, **bad)
    grd_alb = kw.pop("grd_alb", 0.1)
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, grd_alb, **kw)
    assert word in str(ei.value), str(ei.value)


def test_the_refusal_without_the_keyword_points_to_it(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="brdf_modes=True"):
        main.SOS_Aer_batch([0.5], 0.3, 1.0, surface="brdf", brdf=RPV, azimuths=[0.0], **KW)


def test_the_keyword_and_the_result_field():
    import inspect
    from sosrt import main
    assert inspect.signature(main.SOS_Aer_batch).parameters["brdf_modes"].default is False
    f = {x.name: x for x in __import__("dataclasses").fields(main.BatchResult)}
    assert f["bounce_orders"].default is None
    a = main._brdf_args("brdf", RPV, 1, 32, 3, azimuths=[0.0], brdf_modes=True)
    assert a.modes and a.kind == "rpv" and not main._brdf_args("brdf", RPV, 1, 32, 3).modes
