"""Ross-Li ground (brdf=('ross_li', ...)), CPU tier: the two symbols of the C ABI, the NumPy model of
tests/ross_li_np.py -- point values, symmetry, the floor, the white-sky integrals against the published constants by Gauss
quadrature and on the grid's own trapezoid -- and every acceptance and refusal of `_brdf_args`.  No GPU."""
import os
import re

import numpy as np
import pytest

import brdf_np as G
import ross_li_np as RL
import sos_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_ground_source_terms_dev": 9, "sosrt_view_ground_terms_dev": 15}


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
    for meth in ("ground_source_terms_device", "view_ground_terms_device"):
        assert callable(getattr(Solver, meth))
    for name, value in (("SOSRT_BRDF_ROSS_THICK", _lib.BRDF_ROSS_THICK), ("SOSRT_BRDF_LI_SPARSE_R", _lib.BRDF_LI_SPARSE_R),
                        ("SOSRT_BRDF_MAX_TERMS", _lib.BRDF_MAX_TERMS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value
    assert int(re.search(r"#define\s+SOSRT_VERSION\s+(\d+)", header).group(1)) == 105


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_point_values():
    for phi in (0.0, 0.7, np.pi):
        assert abs(RL.k_vol(1.0, 1.0, phi)) <= 1e-15 and abs(RL.k_geo(1.0, 1.0, phi)) <= 1e-15
    for got, ref in ((RL.k_vol(0.5, 0.5, 0.0), np.pi / 4), (RL.k_geo(0.5, 0.5, 0.0), 2.0),
                     (RL.k_vol(0.5, 0.5, np.pi), 0.34242662818613967), (RL.k_geo(0.5, 0.5, np.pi), -3.0)):
        assert abs(got - ref) <= 1e-15, (got, ref)
    assert RL.MU_FLOOR == np.cos(np.radians(80.0)) or abs(RL.MU_FLOOR - np.cos(np.radians(80.0))) <= 1e-16


@pytest.mark.parametrize("mu_floor", [RL.MU_FLOOR, 0.0])
def test_symmetry_in_the_directions(mu_floor):
    rng = np.random.default_rng(7)
    a, b, phi = rng.uniform(0.02, 1, 400), rng.uniform(0.02, 1, 400), rng.uniform(0, np.pi, 400)
    for K in (RL.k_vol, RL.k_geo):
        assert np.array_equal(K(a, b, phi, mu_floor), K(b, a, phi, mu_floor))
    rho = lambda a, b: RL.rho_ross_li(a, b, phi, 0.3, 0.15, 0.04, mu_floor)
    assert np.array_equal(rho(a, b), rho(b, a))


def test_a_pair_below_the_floor_is_the_pair_at_the_floor():
    phi = np.linspace(0, np.pi, 33)
    f = RL.MU_FLOOR
    for K in (RL.k_vol, RL.k_geo):
        assert np.array_equal(K(0.05, 0.6, phi), K(f, 0.6, phi))
        assert np.array_equal(K(0.6, 0.01, phi), K(0.6, f, phi))
        assert np.array_equal(K(0.05, 0.1, phi), K(f, f, phi))
        assert np.array_equal(K(0.05, 0.6, phi, 0.3), K(0.3, 0.6, phi, 0.3)) and np.array_equal(K(0.2, 0.25, phi, 0.3), K(0.3, 0.3, phi, 0.3))
        assert not np.array_equal(K(0.05, 0.6, phi, 0.0), K(f, 0.6, phi, 0.0))       # mu_floor = 0: the formulas as written
    assert np.all(np.isfinite(RL.k_geo(0.01, 0.01, phi, 0.0))) and np.all(np.isfinite(RL.k_vol(0.01, 0.01, phi, 0.0)))


def test_white_sky_constants_by_gauss_quadrature():
    """4 int int rho_bar mu mu' dmu dmu' at mu_floor = 0 on 200 Gauss points against Lucht et al. (2000): measured 2e-6 and 4e-5"""
    x, w = np.polynomial.legendre.leggauss(200)
    x, w = (x + 1) / 2, w / 2
    for kind, ref in RL.WHITE_SKY.items():
        got = 4 * np.einsum("i,j,ij->", w * x, w * x, G.rho_bar((kind, 0.0), x[:, None], x[None, :], 2001))
        print("%s: white-sky integral %.9f (published %.6f), distance %.2e" % (kind, got, ref, abs(got - ref)))
        assert abs(got - ref) <= 1e-4


@pytest.mark.parametrize("N", [64, 66, 128])
def test_white_sky_constants_on_the_grid(N):
    """The same through the grid's own trapezoid (the operator's flux quadrature, the upward nodes' 2 w mu) on 65 azimuth nodes:
    the measured distances of ross_li_np.WHITE_SKY_GRID_DISTANCE with a factor 2, and shrinking with N."""
    mu = O.make_mu(N)
    for kind, ref in RL.WHITE_SKY.items():
        got = RL.white_sky_albedo(mu, N, G.operator(mu, N, (kind, 0.0))[None], np.array([1.0]))
        print("N=%d %s: white-sky albedo on the grid %.9f (published %.6f), distance %.3e" % (N, kind, got, ref, abs(got - ref)))
        assert abs(got - ref) <= 2 * RL.WHITE_SKY_GRID_DISTANCE[kind, N]
    assert all(RL.WHITE_SKY_GRID_DISTANCE[k, 128] < RL.WHITE_SKY_GRID_DISTANCE[k, 64] for k in RL.WHITE_SKY)


def test_the_weighted_source_and_albedos_are_those_of_the_weighted_brdf():
    """the model's sum over terms is the operator of rho = f_iso + f_vol K_vol + f_geo K_geo"""
    N, w, mu0 = 16, np.array([0.30, 0.15, 0.04]), 0.6
    mu = O.make_mu(N)
    Rs = np.stack([G.operator(mu, N, t) for t in RL.terms()])
    r0s = np.stack([G.beam_row(mu, N, mu0, t) for t in RL.terms()])
    whole = ("ross_li",) + tuple(w)
    R, r0 = G.operator(mu, N, whole), G.beam_row(mu, N, mu0, whole)
    I = 0.1 + np.random.default_rng(3).random(2 * N)
    a, b = RL.ground_source_terms(Rs, I, r0s, 0.4, mu0, w), G.ground_source(R, I, r0, 0.4, mu0)
    assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b))
    assert abs(RL.black_sky_albedo(mu, N, r0s, w) - RL.up_weights(mu, N) @ r0) <= 1e-14
    assert abs(RL.white_sky_albedo(mu, N, Rs, w) - RL.up_weights(mu, N) @ R.sum(axis=1)) <= 1e-14


# ---- the checks before any handle exists ----------------------------------------------------------------------------------------------
def args(brdf, grd_alb=1.0, B=3, N=16, **kw):
    from sosrt.main import _brdf_args
    return _brdf_args("brdf", brdf, grd_alb, N, B, **kw)


def test_brdf_args_accepts_ross_li():
    from sosrt.main import ROSS_LI_MU_FLOOR
    assert ROSS_LI_MU_FLOOR == RL.MU_FLOOR
    g = args(("ross_li", 0.3, 0.15, 0.04))
    assert g.kind == "ross_li" and g.params == (RL.MU_FLOOR,) and g.R is None and g.r0 is None
    assert g.terms == (("lambertian", ()), ("ross_thick", (RL.MU_FLOOR,)), ("li_sparse_r", (RL.MU_FLOOR,)))
    assert g.weight.shape == (3, 3) and g.weight.flags.c_contiguous and np.array_equal(g.weight, np.tile([0.3, 0.15, 0.04], (3, 1)))
    g = args(("ross_li", [0.0, 0.3, 0.8], 0.15, np.array([0.0, 0.02, 0.04]), 0.0))
    assert g.params == (0.0,) and np.array_equal(g.weight, [[0.0, 0.15, 0.0], [0.3, 0.15, 0.02], [0.8, 0.15, 0.04]])
    assert args(["ross_li", 0.0, 0.0, 0.1, 0.5]).terms[2] == ("li_sparse_r", (0.5,))
    assert args(("ross_li", [0.1], 0, 0), B=1).weight.shape == (1, 3)
    assert np.array_equal(args(("ross_li", 0.1, 0, 0), grd_alb=[1.0, 1.0, 1.0]).scale, np.ones(3))
    assert args(("ross_li", 0.1, 0, 0), azimuths=[0.0], brdf_modes=True).modes
    assert args(("ross_li", 0.1, 0, 0), view_mu=[0.5], brdf_view=True).view
    assert args(("ross_li", 0.1, 0, 0), view_mu=[0.5], view_azimuths=[0.0], brdf_view=True).view
    for other in ("lambertian", ("rpv", 0.2, 0.8, -0.1)):     # the named grounds of before carry no terms
        g = args(other)
        assert g.terms is None and g.weight is None


@pytest.mark.parametrize("brdf,grd_alb,kw,match", [
    (("ross_li", 0.3, 0.15), 1.0, {}, "Ross-Li"),
    (("ross_li", 0.3, 0.15, 0.04, 0.1, 0.2), 1.0, {}, "Ross-Li"),
    (("ross_li", "x", 0.15, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", 0.3, None, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", 0.3, 0.15, 0.04, "low"), 1.0, {}, "Ross-Li weights"),
    (("ross_li", -0.1, 0.15, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", 0.3, np.nan, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", 0.3, 0.15, np.inf), 1.0, {}, "Ross-Li weights"),
    (("ross_li", [0.1, 0.2], 0.15, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", np.zeros((3, 1)), 0.15, 0.04), 1.0, {}, "Ross-Li weights"),
    (("ross_li", 0.0, [0.0, 0.0, 0.0], 0.0), 1.0, {}, "all zero"),
    (("ross_li", 0.3, 0.15, 0.04, 1.0), 1.0, {}, "mu_floor"),
    (("ross_li", 0.3, 0.15, 0.04, -0.1), 1.0, {}, "mu_floor"),
    (("ross_li", 0.3, 0.15, 0.04, np.nan), 1.0, {}, "mu_floor"),
    (("ross_li", 0.3, 0.15, 0.04), 0.5, {}, "ross_li.*grd_alb must be omitted or 1"),
    (("ross_li", 0.3, 0.15, 0.04), [1.0, 1.0, 0.9], {}, "ross_li.*grd_alb must be omitted or 1"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(azimuths=[0.0]), "brdf_modes=True"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(brdf_modes=True), "give azimuths"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(view_mu=[0.5]), "brdf_view=True"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(brdf_view=True), "give view_mu"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(azimuths=[0.0], brdf_modes=True, mode_batch=True), "mode_batch"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(beam="spherical"), "spherical"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(source="thermal"), "thermal"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(save_orders=True), "save_orders"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(devices=[0, 1]), "devices"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(first_order="readme"), "readme"),
    (("ross_li", 0.3, 0.15, 0.04), 1.0, dict(N=3), "nb_angles >= 4"),
    (("ross-li", 0.3, 0.15, 0.04), 1.0, {}, "ross_li"),
    (("rpv", 0.2, 0.8), 1.0, {}, "ross_li"),
])
def test_brdf_args_refusals(brdf, grd_alb, kw, match):
    with pytest.raises(ValueError, match=match):
        args(brdf, grd_alb, **kw)


def test_ross_li_belongs_to_the_brdf_surface():
    from sosrt.main import _brdf_args
    with pytest.raises(ValueError, match="surface='brdf'"):
        _brdf_args("specular", ("ross_li", 0.3, 0.15, 0.04), 0.3, 16, 3)
    with pytest.raises(ValueError, match="ross_li"):
        _brdf_args("brdf", None, 1.0, 16, 3)


# ---- the model's mode series against the direct azimuth-resolved references, linear regime -------------------------------------------------
# The cases of tests/test_brdf_azimuth_host.py and tests/test_brdf_view_host.py with rho of Ross-Li, weights (0.30, 0.15, 0.04), in
# place of RPV: P0 and the beam row scaled by 1e-6, fixed orders, every blend search stops at its first test (asserted).  The bound
# is theirs, 1e-13 of the maximum.  These are what the device chain and the drivers of tests/test_gpu_ross_li.py stand on.
ROSS_LI = ("ross_li", 0.30, 0.15, 0.04)
SCALE = 1e-6


@pytest.mark.parametrize("N,L,nq,M", [(24, 16, 48, 10), (37, 24, 48, 6)])
def test_mode_series_is_the_direct_solve(N, L, nq, M):
    """Measured: 5.3e-16 (N = 24), 3.9e-16 (N = 37) of max |mode 0| over every mode; the ground is 6.5e-2 of mode 1"""
    import azimuth_direct as D
    import brdf_azimuth_np as BA
    from sosrt import inputs
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    gr = BA.black_three_zone(0.6, L, N)
    nphi, n, nb = nq // 2 + 1, 3, (3, 3)
    log = BA.BlendLog()
    with D.record_blend() as oracle_log:
        _, Iq = BA.direct_solve(gr, fa, fr, ROSS_LI, nq, n, nb, SCALE, log=log)
        Im, status = BA.mode_series(gr, fa, fr, ROSS_LI, M, nphi, n, nb, SCALE, brdf_nphi=nphi, log=log)
        log.oracle = oracle_log
    assert status == 0 and log.first_test_everywhere()
    ref = D.project(Iq, M)
    err = max(np.max(np.abs(Im[m] - ref[m])) for m in range(M + 1)) / np.max(np.abs(ref[0]))
    black = D.mode_fields(gr.geo, fa, fr, M, nphi, n, SCALE)
    share = np.max(np.abs(black[1] - ref[1])) / np.max(np.abs(ref[0]))
    print("N=%d L=%d: mode series vs the direct solve %.2e of max |mode 0|; the ground's share of mode 1 %.2e" % (N, L, err, share))
    assert err <= 1e-13 and share > 1e-3


def test_mode_series_is_the_direct_view_radiance():
    """Measured: first 2.4e-16, scattered 2.0e-15, ground 2.1e-16 of the maximum (N = 24, grid quadrature); the ground's term is
    0.10 of the maximum"""
    import azimuth_direct as D
    import brdf_azimuth_np as BA
    import brdf_view_np as BV
    import view_np as VN
    from sosrt import inputs
    N, L, nq, M, n, nb = 24, 16, 48, 10, 3, (3, 3)
    mv = np.array([0.01, 0.37, 0.6])
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    c, gr = BV.black_column(0.6, L, N)
    nphi = nq // 2 + 1
    log = BA.BlendLog()
    with D.record_blend() as oracle_log:
        phi, direct, _ = BV.direct_view_solve(c, gr, fa, fr, ROSS_LI, nq, n, nb, mv, VN.QUAD_GRID, SCALE, log=log)
        series, status = BV.mode_series_view(c, gr, fa, fr, ROSS_LI, M, nphi, n, nb, mv, VN.QUAD_GRID, SCALE, brdf_nphi=nphi, log=log)
        log.oracle = oracle_log
    assert status == 0 and log.first_test_everywhere()
    total = direct["first"] + direct["scattered"] + direct["ground"]
    mx = np.max(np.abs(D.synthesize(BV.project_half(total, M), phi)))
    for key in ("first", "scattered", "ground"):
        part = D.synthesize(BV.project_half(direct[key], M), phi)
        e = np.max(np.abs(D.synthesize(series[key], phi) - part)) / mx
        print("%s %.2e of the maximum (its share %.2e)" % (key, e, np.max(np.abs(part)) / mx))
        assert e <= 1e-13
    assert np.max(np.abs(D.synthesize(BV.project_half(direct["ground"], M), phi))) > 1e-2 * mx
