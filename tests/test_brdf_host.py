"""BRDF ground (surface='brdf'), CPU tier: the five symbols of the C ABI, the NumPy model of the stages
(tests/brdf_np.py) -- the series in ground reflections against the oracle's in-loop Lambertian ground, the RPV azimuth mean
against an independent quadrature, the Lambertian operator against the in-loop scalar -- and the checks the Python layer makes
before any handle exists.  No GPU."""
import functools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import brdf_np as M
import sos_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_brdf_operator_dev": 6, "sosrt_brdf_beam_dev": 8, "sosrt_ground_source_dev": 8, "sosrt_ground_first_order_dev": 6,
           "sosrt_bounce_accumulate_dev": 5}
RPV = ("rpv", 0.2, 0.8, -0.1)


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
    for meth in ("brdf_operator_device", "brdf_beam_device", "ground_source_device", "ground_first_order_device",
                 "bounce_accumulate_device"):
        assert callable(getattr(Solver, meth))


# ---- the series against the in-loop Lambertian ground ---------------------------------------------------------------------------
# The case of the CPU experiment behind the feature: Rayleigh with an HG(0.6) slab, tau*_aer = 0.3, omega_aer = 0.9, mu0 = 0.6,
# N = 64, L = 30.  The in-loop reference is solve_column(surface='lambertian_readme') started from the black column's first
# order plus the ground field of that first order's surface row and of the beam: its orders n >= 2 reflect their own surface rows.
N_, L_, MU0 = 64, 30, 0.6


@functools.lru_cache(maxsize=None)
def series_against_the_loop(rho, p0_scale, tol, blend=True):
    """(distance over the whole field, distance on the TOA and surface rows, bounces), in units of the reference's maximum"""
    c = M.experiment_column(O, N_, L_, MU0, rho, p0_scale)
    R, r0 = M.operator(c.mu, N_, "lambertian"), M.beam_row(c.mu, N_, MU0, "lambertian")[None]
    with np.errstate(all="ignore"):
        I, bounces, _, status, _ = M.bounce_solve(O, [c], R, r0, [rho], tol=tol, beam=p0_scale, blend=blend, max_bounces=64)
        I1b = O.first_order(M.black(c))
        G1 = M.ground_field(M.ground_source(R, I1b[-1], p0_scale * r0[0], c.tau[-1], MU0, rho), c.tau, c.mu, N_, blend)[0]
        ref = O.solve_column(c, tol=tol, literal=False, I1=I1b + G1).I
    assert status[0] == 0
    d, mx = np.abs(I[0] - ref), np.max(np.abs(ref))
    return d.max() / mx, max(d[0].max(), d[-1].max()) / mx, int(bounces[0])


def test_linear_regime_the_series_is_the_loop():
    """With P0 and the beam term scaled by 1e-6 every blend search stops at its first test and the blend is a fixed linear map
    (the trick of DESIGN section 11): the sum over bounces is the in-loop solve to rounding.  Measured 3.6e-13."""
    whole, rows, bounces = series_against_the_loop(0.3, 1e-6, 1e-12)
    print("linear regime: %.3e of the field maximum (%.3e on the TOA and surface rows), %d bounces" % (whole, rows, bounces))
    assert whole <= 1e-11


def test_linear_regime_needs_the_blend_on_the_ground_rows():
    """Without the blend on the rows of the ground field the two differ at the percent level: the loop blends B exp + q as a whole."""
    whole, _, _ = series_against_the_loop(0.3, 1e-6, 1e-12, blend=False)
    print("linear regime, ground rows not blended: %.3e of the field maximum" % whole)
    assert whole > 1e-3


# measured with this model at rho = 0.3: 5.50e-2 of the field maximum overall, 6.26e-3 on the TOA and surface rows (rho = 0.8:
# 3.2e-2 and 9.8e-3); the bounds are twice the rho = 0.3 figures
NATURAL_BOUND, NATURAL_BOUND_ROWS = 2 * 5.50e-2, 2 * 6.26e-3


@pytest.mark.parametrize("rho", [0.3, 0.8])
def test_natural_scale_distance_is_the_blends(rho):
    """At natural scale the blend's search threshold (1e-4, absolute) makes it non-linear: the series and the loop differ by
    the reference's mu -> 0 treatment, as the azimuth modes do."""
    whole, rows, bounces = series_against_the_loop(rho, 1.0, 1e-4)
    print("natural scale rho = %g: %.3e of the field maximum (%.3e on the TOA and surface rows), %d bounces" % (rho, whole, rows, bounces))
    assert whole <= NATURAL_BOUND and rows <= NATURAL_BOUND_ROWS
    if rho == 0.3:
        assert bounces == 4


# ---- the RPV azimuth mean ---------------------------------------------------------------------------------------------------------
def rpv_scalar(a, b, phi, rho0, k, theta):
    """the RPV formula on scalars with math's functions (independent of the model's array code)"""
    sa, sb = math.sqrt(max(0.0, 1 - a * a)), math.sqrt(max(0.0, 1 - b * b))
    ta, tb = sa / a, sb / b
    cosg = a * b + sa * sb * math.cos(phi)
    F = (1 - theta ** 2) / math.pow(1 + 2 * theta * cosg + theta ** 2, 1.5)
    G = math.sqrt(max(0.0, ta * ta + tb * tb - 2 * ta * tb * math.cos(phi)))
    return rho0 * math.pow(a * b * (a + b), k - 1) * F * (1 + (1 - rho0) / (1 + G))


def quadrature_2001(a, b):
    n = 2001
    h = math.pi / (n - 1)
    f = [rpv_scalar(a, b, q * h, *RPV[1:]) for q in range(n)]
    return (math.fsum(f) - 0.5 * (f[0] + f[-1])) * h / math.pi


def test_rpv_mean_against_a_2001_node_quadrature():
    """rho_bar on 2001 nodes against a scalar 2001-node trapezoid sum of the formula, on a spread of pairs that includes the hot
    spot's diagonal a = b.  The default 65 nodes are a coarser rule, not another formula: against 2001 nodes they are within
    2e-3 on the diagonal a = b, where the hot spot has a cusp at phi = 0 that the trapezoid rule converges to only as h^2, and
    within 1e-8 (measured 2e-12) two lanes and more off it."""
    mu = O.make_mu(37)
    up = mu[38:]
    pairs = [(up[i], up[j]) for i in range(0, 36, 5) for j in range(0, 36, 7)] + [(up[i], up[i]) for i in (0, 17, 35)] + [(up[3], 0.6)]
    worst = 0.0
    for a, b in pairs:
        ref = quadrature_2001(a, b)
        worst = max(worst, abs(float(M.rho_bar(RPV, a, b, 2001)) - ref) / ref)
    print("rho_bar(2001 nodes) vs the scalar quadrature: %.3e relative" % worst)
    assert worst <= 1e-8
    a = up[:, None]
    fine, coarse = M.rho_bar(RPV, a, a.T, 2001), M.rho_bar(RPV, a, a.T, 65)
    rel = np.abs(coarse - fine) / fine
    off = rel.copy()
    for d in (-1, 0, 1):
        off[np.arange(max(0, -d), 36 - max(0, d)), np.arange(max(0, d), 36 - max(0, -d))] = 0
    print("65 nodes vs 2001: %.3e on the diagonal, %.3e two lanes and more off it" % (np.max(np.diag(rel)), off.max()))
    assert np.max(rel) <= 1e-2 and off.max() <= 1e-8


@pytest.mark.parametrize("N", [4, 16, 37, 64, 128])
def test_rpv_is_reciprocal_and_finite_at_every_size(N):
    """rho_bar(a, b) = rho_bar(b, a); no NaN at the hot spot, where the geometry factor's square root has the argument 0 to rounding"""
    up = O.make_mu(N)[N + 1:]
    r = M.rho_bar(RPV, up[:, None], up[None, :])
    assert np.all(np.isfinite(r)) and np.all(r > 0)
    assert np.max(np.abs(r - r.T)) <= 1e-12 * np.max(r)
    assert np.all(np.isfinite(M.operator(O.make_mu(N), N, RPV))) and np.all(np.isfinite(M.beam_row(O.make_mu(N), N, 0.6, RPV)))


def test_rpv_series_converges_in_four_bounces():
    """rho0 = 0.2, k = 0.8, Theta = -0.1 at N = 37, L = 24"""
    c = M.experiment_column(O, 37, 24, MU0, 0.0)
    R, r0 = M.operator(c.mu, 37, RPV), M.beam_row(c.mu, 37, MU0, RPV)[None]
    with np.errstate(all="ignore"):
        I, bounces, ratio, status, _ = M.bounce_solve(O, [c], R, r0, [1.0])
    assert np.all(np.isfinite(I)) and status[0] == 0 and bounces[0] == 4 and ratio[0] < 1e-4


# ---- the Lambertian operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 37, 64])
def test_lambertian_operator_is_the_in_loop_scalar(N):
    mu = O.make_mu(N)
    row = np.random.default_rng(N).random(2 * N)
    rev = np.arange(N - 2, -1, -1)
    scalar = 2 * 0.3 * M._trapz(row[rev] * mu[rev], mu[rev])                 # the boundary of the order loop (oracle _transport)
    S = M.ground_source(M.operator(mu, N, "lambertian"), row, None, 0.0, 1.0, 0.3)
    assert S.shape == (N - 1,) and np.max(np.abs(S - scalar)) <= 1e-14 * scalar


def test_ground_field_conventions():
    """lane N and the downward lanes are 0; the blend reads lane N; a source alternating +-1 runs the search off the row"""
    N, L = 37, 24
    c = M.experiment_column(O, N, L, MU0, 0.3)
    S = 0.3 + 0.1 * np.arange(N - 1) / N
    G, status, blended = M.ground_field(S, c.tau, c.mu, N)
    assert status == 0 and np.all(G[:, :N + 1] == 0) and np.array_equal(G[-1, N + 3:], S[2:])
    assert blended[-1, N + 1] and not blended[-1, N + 2:].any()      # the surface row is S itself: the search stops at its first test
    assert blended[0, N + 1:N + 4].all()                     # at the top the lanes next to mu = 0 are attenuated away: it goes on
    G, status, blended = M.ground_field((-1.0) ** np.arange(N - 1), c.tau, c.mu, N)
    assert status == M.COL_INDEXERROR and not blended[-1].any()


def test_a_black_ground_ends_the_series_at_once():
    c = M.experiment_column(O, 37, 24, MU0, 0.0)
    R, r0 = M.operator(c.mu, 37, "lambertian"), M.beam_row(c.mu, 37, MU0, "lambertian")[None]
    with np.errstate(all="ignore"):
        I, bounces, ratio, status, terms = M.bounce_solve(O, [c], R, r0, [0.0])
    assert bounces[0] == 1 and ratio[0] == 0 and status[0] == 0 and not np.any(terms[1][0]) and np.array_equal(I[0], terms[0][0])


# ---- refusals of the Python layer, before any handle exists ----------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
OK = dict(surface="brdf", brdf="lambertian")
R_OK, R0_OK = np.zeros((31, 31)), np.zeros(31)
BATCH_REFUSALS = [
    (dict(surface="brdf"), "needs brdf"),
    (dict(brdf="lambertian"), "surface='brdf'"),
    (dict(surface="lambertian", brdf="lambertian"), "surface='brdf'"),
    (dict(OK, azimuths=[0.0]), "m = 0"),
    (dict(OK, azimuths=[0.0], mode_batch=True), "m = 0"),
    (dict(OK, view_mu=[0.5]), "view_mu"),
    (dict(OK, view_mu=[0.5], view_azimuths=[0.0]), "m = 0"),
    (dict(OK, beam="spherical"), "spherical"),
    (dict(OK, source="thermal", planck=np.ones(24), planck_surface=1.0), "thermal"),
    (dict(OK, first_order="readme"), "readme"),
    (dict(OK, devices=[0, 1]), "devices"),
    (dict(OK, save_orders=True), "save_orders"),
    (dict(surface="brdf", brdf="oceanic"), "brdf must be"),
    (dict(surface="brdf", brdf=("rpv", 0.2, 0.8)), "rpv"),
    (dict(surface="brdf", brdf=("rpv", -0.2, 0.8, 0.0)), "rho0 > 0"),
    (dict(surface="brdf", brdf=("rpv", 0.2, 0.0, 0.0)), "k > 0"),
    (dict(surface="brdf", brdf=("rpv", 0.2, 0.8, 1.0)), "|theta| < 1"),
    (dict(surface="brdf", brdf=("rpv", 0.2, 0.8, float("nan"))), "|theta| < 1"),
    (dict(surface="brdf", brdf=("cox-munk", 5.0, 0.0, 0.0)), "named brdf"),
    (dict(surface="brdf", brdf=(np.zeros((30, 31)), R0_OK)), "R must be"),
    (dict(surface="brdf", brdf=(R_OK, np.zeros(30))), "R must be"),
    (dict(surface="brdf", brdf=(R_OK, np.zeros((2, 31)))), "R must be"),
    (dict(surface="brdf", brdf=(np.full((31, 31), np.nan), R0_OK)), "finite"),
    (dict(OK, nb_angles=3), "nb_angles >= 4"),
]


@pytest.mark.parametrize("bad,word", BATCH_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_batch_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import dist, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, 0.1, **dict(KW, **bad))
    assert word in str(ei.value), str(ei.value)


def test_the_scale_is_checked_before_any_handle(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    for grd_alb, brdf, word in ((-0.1, "lambertian", "grd_alb"), (float("nan"), "lambertian", "grd_alb"),
                                (0.5, RPV, "omitted or 1"), ([0.1, 0.2], "lambertian", "broadcast")):
        with pytest.raises(ValueError) as ei:
            main.SOS_Aer_batch([0.5, 0.6, 0.7], 0.3, grd_alb, surface="brdf", brdf=brdf, **KW)
        assert word in str(ei.value), str(ei.value)


OTHER_REFUSALS = [(dict(surface="brdf"), "needs brdf"), (dict(brdf="lambertian"), "surface='brdf'"), (dict(OK, beam="spherical"), "spherical"),
                  (dict(OK, source="thermal", planck=np.ones(24), planck_surface=1.0), "thermal"),
                  (dict(surface="brdf", brdf=("rpv", 0.2, 0.8, 1.5)), "|theta| < 1")]


@pytest.mark.parametrize("bad,word", OTHER_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_other_drivers_refuse_before_any_handle(bad, word, monkeypatch):
    from sosrt import forcing, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(forcing, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    calls = [lambda: main.solve_batch_device([0.5, 0.6], 0.3, 0.1, **KW, **bad),
             lambda: main.SOS_Aer_layers([0.5, 0.6], 0.1, [(25, 17, 0.3, 0.9)], **KW, **bad),
             lambda: main.SOS_Aer(**KW, **bad)]
    if "source" not in bad:
        calls.append(lambda: forcing.toa_net_flux(0.5, 0.124, [0.1, 0.2], 0.1, 1.0, 0.9, **KW, **bad))
        calls.append(lambda: forcing.radiative_forcing(0.5, 0.124, [0.1, 0.2], 0.1, 1.0, 0.9, **KW, **bad))
        calls.append(lambda: forcing.critical_albedo(0.5, 0.124, [0.1, 0.2], 0.1, 1.0, **KW, **bad))
    for call in calls:
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), str(ei.value)


def test_single_column_driver_refuses_the_readme_first_order(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="readme"):
        main.SOS_Aer(first_order="readme", **KW, **OK)


def test_the_single_slab_is_refused():
    from sosrt import main
    spec = main._brdf_args("brdf", "lambertian", 0.3, 32, 1)
    with pytest.raises(ValueError, match="single slab"):
        main.solve_brdf(SimpleNamespace(single_slab=True), np.zeros((1, 24)), None, None, spec, 0.5)


def test_the_arguments_of_a_valid_ground():
    from sosrt import main
    assert main._brdf_args("specular", None, 0.3, 32, 3) is None
    a = main._brdf_args("brdf", "lambertian", [0.0, 0.3, 0.8], 32, 3)
    assert a.kind == "lambertian" and a.R is None and np.array_equal(a.scale, [0.0, 0.3, 0.8])
    a = main._brdf_args("brdf", RPV, 1, 32, 3)
    assert a.kind == "rpv" and a.params == (0.2, 0.8, -0.1) and np.array_equal(a.scale, np.ones(3))
    a = main._brdf_args("brdf", (R_OK, R0_OK), 0.5, 32, 3)
    assert a.kind is None and a.R.shape == (31, 31) and a.r0.shape == (3, 31) and np.array_equal(a.scale, [0.5] * 3)


def test_the_specular_ground_is_the_default_everywhere():
    import inspect
    from sosrt import forcing, main
    for f in (main.SOS_Aer_batch, main.solve_batch_device, main.SOS_Aer_layers, main.SOS_Aer, forcing.toa_net_flux):
        p = inspect.signature(f).parameters
        assert p["surface"].default == "specular" and p["brdf"].default is None
