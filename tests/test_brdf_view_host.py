"""View radiance over a BRDF ground (brdf_view=True), CPU tier: the four symbols of the C ABI, the NumPy model
(tests/brdf_view_np.py) -- its rows at node cosines, the three-term decomposition per Fourier mode against a direct reference on
uniform azimuth nodes in the linear regime, the azimuth mean, the node pin at natural scale -- and the checks the Python layer
makes before any handle exists.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import azimuth_direct as D
import brdf_azimuth_np as BA
import brdf_np as G
import brdf_view_np as BV
import sos_oracle as O
import view_np as VN
from sosrt import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_brdf_view_rows_modes_dev": 11, "sosrt_brdf_view_beam_modes_dev": 12, "sosrt_brdf_view_beam_azimuth_dev": 11,
           "sosrt_view_ground_dev": 14}
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
    assert L.sosrt_version() == 105
    for meth in ("brdf_view_rows_modes_device", "brdf_view_beam_modes_device", "brdf_view_beam_azimuth_device", "view_ground_device"):
        assert callable(getattr(Solver, meth))


# ---- the model's rows at node cosines are the grid's operators, exactly --------------------------------------------------------------
@pytest.mark.parametrize("brdf", ["lambertian", RPV], ids=["lambertian", "rpv"])
@pytest.mark.parametrize("N", [16, 37])
def test_rows_at_node_cosines_are_the_operator_columns(N, brdf):
    mu = O.make_mu(N)
    up = mu[N + 1:]
    ms = [0, 1, 2, 5]
    for nphi in (33, 65):
        assert np.array_equal(BV.view_rows(mu, N, up, brdf, nphi), G.operator(mu, N, brdf, nphi))
        assert np.array_equal(BV.view_rows_modes(mu, N, up, brdf, ms, nphi), BA.operator_modes(mu, N, brdf, ms, nphi))
        assert np.array_equal(BV.view_rows_modes(mu, N, up, brdf, [0], nphi)[0], BV.view_rows(mu, N, up, brdf, nphi))
        assert np.array_equal(BV.view_beam_row(up, 0.6, brdf, nphi), G.beam_row(mu, N, 0.6, brdf, nphi))
        assert np.array_equal(BV.view_beam_modes(up, 0.6, brdf, ms, nphi), BA.beam_modes(mu, N, 0.6, brdf, ms, nphi))
    # a subset of the nodes, in any order, picks the same rows; the ground source at a node is the grid's
    pick = np.array([N - 2, 0, 5])
    assert np.array_equal(BV.view_rows(mu, N, up[pick], brdf), G.operator(mu, N, brdf)[pick])
    I = np.random.default_rng(3).random(2 * N)
    S = G.ground_source(G.operator(mu, N, brdf), I, G.beam_row(mu, N, 0.6, brdf), 0.4, 0.6, 0.7)
    Sv = G.ground_source(BV.view_rows(mu, N, up[pick], brdf), I, BV.view_beam_row(up[pick], 0.6, brdf), 0.4, 0.6, 0.7)
    assert np.max(np.abs(Sv - S[pick])) <= 1e-15 * np.max(np.abs(S))


def test_exact_beam_rows_and_the_hot_spot():
    """rho at the azimuth itself: finite at the hot spot a = b, phi = 0; its azimuth mean on the builders' nodes is rho_bar; and
    its cosine sum over the modes (plus the Nyquist term) is rho at a node."""
    mv = np.array([0.01, 0.37, 0.6, 1.0])
    nphi = 65
    phi = np.linspace(0, np.pi, nphi)
    r = BV.view_beam_azimuth(mv, 0.6, RPV, phi)
    assert r.shape == (nphi, 4) and np.all(np.isfinite(r)) and np.all(r > 0)
    assert r[0, 2] == np.max(r[:, 2])                        # the hot spot is the lane's maximum
    assert np.max(np.abs(G._trapz(r, phi, axis=0) / np.pi - BV.view_beam_row(mv, 0.6, RPV, nphi))) <= 1e-15
    rm = BV.view_beam_modes(mv, 0.6, RPV, range(nphi), nphi)
    w = np.where((np.arange(nphi) == 0) | (np.arange(nphi) == nphi - 1), 1.0, 2.0)
    back = np.einsum("mv,mq->qv", rm * w[:, None], np.cos(np.outer(np.arange(nphi), phi)))
    assert np.max(np.abs(back - r)) <= 1e-13 * np.max(r)
    assert np.array_equal(BV.view_beam_azimuth(mv, 0.6, "lambertian", phi), np.ones((nphi, 4)))


def test_the_ground_term_is_unblended_and_upward():
    tau = np.linspace(0, 0.4, 7)
    mv = np.array([0.01, 0.5])
    S = np.array([0.3, 0.2])
    g = BV.view_ground(S, tau, mv)
    assert g.shape == (7, 4) and not g[:, :2].any() and np.array_equal(g[-1, 2:], S)
    assert np.max(np.abs(g[0, 2:] - S * np.exp(-0.4 / mv))) <= 1e-16


# ---- the decomposition against the direct reference, linear regime ---------------------------------------------------------------------
# The setup of tests/test_brdf_azimuth_host.py: P0 and the beam row scaled by 1e-6, fixed orders, every blend search stops at its
# first test (asserted); Rayleigh + HG(0.5) over RPV (0.2, 0.8, -0.1), mu0 = 0.6.  The direct reference on nq = 48 nodes has the
# builders' quadrature (nphi = 25), so its modes 0..M are the series' to rounding whatever M leaves out; it is compared on its
# own nodes of [0, pi] (phi = 0 and pi among them) after the projection on those modes.
MU_VIEW = np.array([0.01, 0.37, 0.6])                        # the limb, an ordinary lane, the hot-spot lane mu_view = mu0
CASES = {"N16": (16, 16, 48, 6, 3, (3, 3)), "N24": (24, 16, 48, 10, 3, (3, 3))}       # N, L, nq, M, orders, orders of the reflections


@functools.lru_cache(maxsize=None)
def linear_case(name, quad):
    N, L, nq, M, n, nb = CASES[name]
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    c, gr = BV.black_column(0.6, L, N)
    nphi = nq // 2 + 1
    log = BA.BlendLog()
    with D.record_blend() as oracle_log:
        phi, direct, _ = BV.direct_view_solve(c, gr, fa, fr, RPV, nq, n, nb, MU_VIEW, quad, SCALE, log=log)
        series, status = BV.mode_series_view(c, gr, fa, fr, RPV, M, nphi, n, nb, MU_VIEW, quad, SCALE, brdf_nphi=nphi, log=log)
        log.oracle = oracle_log
    assert status == 0 and log.first_test_everywhere()
    unsigned, _ = BV.mode_series_view(c, gr, fa, fr, RPV, M, nphi, n, nb, MU_VIEW, quad, SCALE, brdf_nphi=nphi, sign=False)
    return phi, direct, series, unsigned, M


@pytest.mark.parametrize("quad", [VN.QUAD_GRID, VN.QUAD_LINEAR], ids=["grid", "linear"])
@pytest.mark.parametrize("name", list(CASES))
def test_mode_series_is_the_direct_view_radiance(name, quad):
    """Measured, in units of the maximum: 1.1e-15 / 7.8e-16 (N = 16, grid / linear), 2.2e-15 / 1.4e-15 (N = 24); each of the
    three terms alone <= 2.0e-15; the ground's term is 0.15 (grid) and 0.57 (linear) of the maximum.  Without the (-1)^m on the
    grid's and the view lanes' operators: 9.0e-3 / 2.8e-2 and 9.2e-3 / 2.8e-2."""
    phi, direct, series, unsigned, M = linear_case(name, quad)
    assert phi[0] == 0 and abs(phi[-1] - np.pi) < 1e-15
    total = lambda d: d["first"] + d["scattered"] + d["ground"]
    ref = D.synthesize(BV.project_half(total(direct), M), phi)
    mx = np.max(np.abs(ref))
    for key in ("first", "scattered", "ground"):
        part = D.synthesize(BV.project_half(direct[key], M), phi)
        e = np.max(np.abs(D.synthesize(series[key], phi) - part)) / mx
        print("%s %s: %s %.2e of the maximum (its share %.2e)" % (name, quad, key, e, np.max(np.abs(part)) / mx))
        assert e <= 1e-13
    assert np.max(np.abs(D.synthesize(BV.project_half(direct["ground"], M), phi))) > 1e-2 * mx      # the ground is a visible part
    e, eu = (np.max(np.abs(D.synthesize(total(s), phi) - ref)) / mx for s in (series, unsigned))
    print("%s %s: signed series %.3e, unsigned %.3e of the maximum" % (name, quad, e, eu))
    assert e <= 1e-13
    assert eu > 1e-4                                         # the comparison tells the two conventions apart
    assert not series["ground"][:, :, :len(MU_VIEW)].any() and not direct["ground"][:, :, :len(MU_VIEW)].any()


@pytest.mark.parametrize("name", list(CASES))
def test_the_azimuth_mean_is_the_view_mu_only_model(name):
    """The mean of the direct reference over its nq nodes is mode 0 of the series, which is what view_mu alone computes."""
    _, direct, series, _, _ = linear_case(name, VN.QUAD_GRID)
    got = series["first"][0] + series["scattered"][0] + series["ground"][0]
    mean = BV.project_half(direct["first"] + direct["scattered"] + direct["ground"], 0)[0]
    assert np.max(np.abs(mean - got)) <= 1e-12 * np.max(np.abs(got))
    for key in ("first", "scattered", "ground"):
        assert np.max(np.abs(BV.project_half(direct[key], 0)[0] - series[key][0])) <= 1e-12 * np.max(np.abs(got))


def test_exact_beam_term_is_the_limit_of_its_modes():
    """view_first_order='exact' takes the beam's single reflection at the azimuth itself: on the builders' nodes it is the sum of
    all the modes of the beam row (with the Nyquist term), which a truncated series only approaches as 1 / m^2."""
    c, gr = BV.black_column(0.6, 16, 16)
    nphi = 25
    phi = np.linspace(0, np.pi, nphi)
    exact = BV.beam_ground(gr, RPV, MU_VIEW, phi, SCALE)
    rm = BV.view_beam_modes(MU_VIEW, 0.6, RPV, range(nphi), nphi) * np.exp(-gr.tau[-1] / 0.6) * SCALE
    w = np.where((np.arange(nphi) == 0) | (np.arange(nphi) == nphi - 1), 1.0, 2.0)
    full = np.stack([BV.view_ground(s, gr.tau, MU_VIEW) for s in np.einsum("mv,mq->qv", rm * w[:, None], np.cos(np.outer(np.arange(nphi), phi)))])
    assert np.max(np.abs(full - exact)) <= 1e-13 * np.max(exact)
    cut = np.stack([BV.view_ground(s, gr.tau, MU_VIEW) for s in np.einsum("mv,mq->qv", (rm * w[:, None])[:11], np.cos(np.outer(np.arange(11), phi)))])
    assert np.max(np.abs(cut - exact)) > 1e-4 * np.max(exact)      # (M = 10 leaves the hot spot's cusp out)


# ---- the node pin at natural scale -------------------------------------------------------------------------------------------------------
# View cosines on the grid's nodes, GRID quadrature, the column of tests/brdf_np.py (Rayleigh + HG(0.6), tau*_aer = 0.3, omega = 0.9)
# at N = 64, L = 30, mu0 = 0.85 over RPV (0.2, 0.8, -0.1): 33 upward lanes that no blend rewrote (mu0 = 0.6: 23, mu0 = 0.35: 31).
NODE_PIN = 1.970e-6          # measured (1.9692e-6, rounded up): max |I_view - I| on those lanes, in units of the field maximum (tol = 1e-4)


def test_node_pin_at_natural_scale():
    """With I_src = I minus every term's last order the three terms reproduce I on the untouched lanes to 1e-12 (that is how the
    lanes are found); with I_src = I, what the drivers pass, the stage adds the series' next term: measured 1.969e-6 of the field
    maximum on 33 lanes (5 reflections after the black solve's 12 orders, 13 orders each).  The device test bounds its own
    figure at twice NODE_PIN."""
    c = G.experiment_column(O, 64, 30, 0.85, 0.0)
    with np.errstate(all="ignore"):
        dist, lanes, ok, r = BV.node_pin(c, RPV)
    print("node pin: %.3e of the field maximum on %d untouched upward lanes; orders %s, status %d" % (dist, lanes, r["orders"], r["status"]))
    assert r["status"] == 0 and 1 <= r["bounces"] < 32
    assert lanes >= 30
    assert 0.5 * NODE_PIN <= dist <= NODE_PIN


# ---- refusals of the Python layer, before any handle exists -----------------------------------------------------------------------------
KW = dict(nb_layers=24, nb_angles=32)
OK = dict(surface="brdf", brdf=RPV, grd_alb=1.0, view_mu=[0.5], brdf_view=True)
AZ = dict(OK, view_azimuths=[0.0, 1.0])
REFUSALS = [
    (dict(brdf_view=True), "brdf_view belongs"),
    (dict(brdf_view=True, view_mu=[0.5]), "brdf_view belongs"),
    (dict(surface="lambertian", brdf_view=True, view_mu=[0.5]), "brdf_view belongs"),
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, brdf_view=True), "give view_mu"),
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, brdf_view=True, view_azimuths=[0.0]), "give view_mu"),
    (dict(OK, brdf_view=1), "True or False"),
    (dict(OK, brdf_view="yes"), "True or False"),
    (dict(OK, azimuths=[0.0]), "azimuths"),
    (dict(OK, azimuths=[0.0], brdf_modes=True), "brdf_modes"),
    (dict(AZ, azimuths=[0.0]), "azimuths"),
    (dict(AZ, mode_batch=True), "mode_batch"),
    (dict(OK, mode_chunk=2), "mode_batch"),
    (dict(OK, aer_set=[0, 0, 0]), "aer_set"),
    (dict(OK, P_atm=np.zeros((64, 64))), "named phase functions"),
    (dict(OK, P0_aer=np.zeros((3, 64))), "named phase functions"),
    (dict(OK, beam="spherical"), "spherical"),
    (dict(OK, source="thermal", planck=np.ones(24), planck_surface=1.0), "thermal"),
    (dict(OK, first_order="readme"), "readme"),
    (dict(OK, save_orders=True), "save_orders"),
    (dict(OK, devices=[0, 1]), "devices"),
    (dict(OK, brdf=(np.zeros((31, 31)), np.zeros(31))), "no rows off the grid"),
    (dict(OK, grd_alb=0.5), "omitted or 1"),
    (dict(OK, view_mu=[0.001]), "[0.01, 1]"),
    (dict(OK, view_mu=np.full(65, 0.5)), "1..64"),
    (dict(OK, view_levels=[24]), "view_levels"),
    (dict(OK, view_quadrature="simpson"), "view_quadrature"),
    (dict(OK, view_first_order="modes"), "give view_azimuths"),
    (dict(AZ, view_first_order="fast"), "view_first_order"),
    (dict(AZ, n_modes=64, nphi_modes=131), "n_modes must be <= 63"),
    (dict(AZ, n_modes=30, nphi_modes=25), "nphi_modes"),
    # as before the keyword
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, view_mu=[0.5]), "the view stage has no ground-reflection term"),
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, view_mu=[0.5], view_azimuths=[0.0]), "only the azimuth mean (mode m = 0) of the BRDF is built"),
    (dict(surface="brdf", brdf=RPV, grd_alb=1.0, azimuths=[0.0], brdf_modes=True, view_mu=[0.5]), "view_mu"),
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
    with pytest.raises(ValueError, match="brdf_view=True"):
        main.SOS_Aer_batch([0.5], 0.3, 1.0, surface="brdf", brdf=RPV, view_mu=[0.5], **KW)


def test_the_keyword_and_the_result_fields():
    import dataclasses
    import inspect
    from sosrt import main
    assert inspect.signature(main.SOS_Aer_batch).parameters["brdf_view"].default is False
    f = {x.name: x for x in dataclasses.fields(main.BatchResult)}
    assert f["I_view_ground"].default is None and f["I_view_azimuth_ground"].default is None
    a = main._brdf_args("brdf", RPV, 1, 32, 3, view_mu=[0.5], brdf_view=True)
    assert a.view and not a.modes and a.kind == "rpv" and not main._brdf_args("brdf", RPV, 1, 32, 3).view
    assert main._brdf_args("brdf", "lambertian", [0.1, 0.2, 0.3], 32, 3, view_mu=[0.5], view_azimuths=[0.0], brdf_view=True).view
