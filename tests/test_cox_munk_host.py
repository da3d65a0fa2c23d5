"""Cox-Munk ocean ground (brdf=('cox_munk', ...)), CPU tier: the NumPy model of tests/cox_munk_np.py against
the properties of its formulas and a fine quadrature, the `ocean` helpers, the checks the Python layer makes before any handle
exists and the ground it constructs.  No GPU."""
import functools

import numpy as np
import pytest

import brdf_np as G
import cox_munk_np as CM
import sos_oracle as O

KW = dict(nb_layers=24, nb_angles=32)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("U", [0.0, 2.0, 10.0])
def test_glint_is_symmetric_finite_and_positive(U, shadow):
    up = O.make_mu(37)[38:]
    phi = np.linspace(0, np.pi, 33)
    r = CM.rho_glint(up[:, None, None], up[None, :, None], phi[None, None, :], CM.slope_variance(U), CM.INDEX, shadow)
    assert np.all(np.isfinite(r)) and np.all(r >= 0) and r.max() > 0
    assert np.max(np.abs(r - np.swapaxes(r, 0, 1))) <= 1e-14 * r.max()
    # through the names brdf_np resolves, the composed ground among them
    brdf = ("cox_munk", CM.slope_variance(U), CM.INDEX, shadow)
    assert np.array_equal(G._rho(brdf)(up[:, None], 0.6, 2.0), r_at(up[:, None], 0.6, 2.0, U, shadow))
    ocean = ("ocean", 0.02, 0.9, CM.slope_variance(U), CM.INDEX, shadow)
    assert np.array_equal(G._rho(ocean)(up, 0.6, 2.0), 0.02 + 0.9 * r_at(up, 0.6, 2.0, U, shadow))
    assert G._rho("lambertian") is G.rho_lambertian


def r_at(a, b, phi, U, shadow):
    return CM.rho_glint(a, b, phi, CM.slope_variance(U), CM.INDEX, shadow)


def test_the_peak_is_the_specular_direction():
    """a = b: the facet is level at phi = pi (t2 = 0, the angle of incidence is the zenith angle), and tilted by the zenith angle at
    phi = 0, where rho is the smaller by exp(-tan^2 / sigma2)"""
    s2 = CM.slope_variance(5.0)
    for mu in (0.3, 0.6, 0.9):
        at_pi = CM.rho_glint(mu, mu, np.pi, s2, CM.INDEX, False)
        assert abs(at_pi - CM.fresnel(mu) / (4 * s2 * mu * mu)) <= 1e-14 * at_pi
        assert CM.rho_glint(mu, mu, 0.0, s2, CM.INDEX, False) < 1e-3 * at_pi
        phi = np.linspace(0, np.pi, 181)
        assert np.argmax(CM.rho_glint(mu, mu, phi, s2)) == 180


@pytest.mark.parametrize("n", [1.2, 1.34, 1.5])
def test_fresnel_at_normal_incidence_and_at_grazing(n):
    assert abs(CM.fresnel(1.0, n) - ((n - 1) / (n + 1)) ** 2) <= 1e-16
    assert abs(CM.fresnel(0.0, n) - 1.0) <= 1e-15
    c = np.linspace(0, 1, 101)
    assert np.all(CM.fresnel(c, n) <= 1) and np.all(CM.fresnel(c, n) > 0)


@pytest.mark.parametrize("shadow", [True, False])
def test_no_shadow_at_the_zenith(shadow):
    """Lambda(1) = 0 although cot is infinite there; S(1, 1) = 1 either way, and the glint at the grid's last node is finite"""
    for s2 in (CM.slope_variance(0.0), CM.slope_variance(10.0)):
        assert CM.smith_lambda(1.0, s2) == 0.0 and CM.smith_lambda(np.array([1.0, 0.5]), s2)[0] == 0.0
        assert CM.shadowing(1.0, 1.0, s2, shadow) == 1.0
        assert np.isfinite(CM.rho_glint(1.0, 1.0, 0.3, s2, CM.INDEX, shadow))
        assert np.all(np.isfinite(CM.rho_glint(1.0, np.array([0.01, 0.5, 1.0]), 0.3, s2, CM.INDEX, shadow)))
    lam = CM.smith_lambda(np.array([0.05, 0.2, 0.5, 0.9]), CM.slope_variance(5.0))
    assert np.all(lam >= 0) and np.all(np.diff(lam) < 0)           # shadowing grows toward the horizon


@functools.lru_cache(maxsize=None)
def fine(U, mu0):
    return CM.black_sky_fine(mu0, ("cox_munk", CM.slope_variance(U), CM.INDEX, True))


@pytest.mark.parametrize("U,mu0,N", sorted(CM.BLACK_SKY_GRID_DISTANCE))
def test_black_sky_albedo_against_a_fine_quadrature(U, mu0, N):
    """The glint's directional-hemispherical reflectance on the grid's trapezoid (make_mu(N), 65 azimuth nodes) against 4001 cosines
    x 2049 azimuths: within twice the distance recorded with this model (cox_munk_np.BLACK_SKY_GRID_DISTANCE); the fine value is the
    recorded one to its printed digits."""
    ref = fine(U, mu0)
    got = CM.black_sky_grid(O.make_mu(N), N, mu0, ("cox_munk", CM.slope_variance(U), CM.INDEX, True))
    print("U=%g mu0=%g N=%d: black-sky albedo %.6f on the grid, %.6f fine, distance %.3e" % (U, mu0, N, got, ref, abs(got - ref)))
    assert abs(ref - CM.BLACK_SKY_FINE[U, mu0]) <= 0.6e-5          # (the coarsest record has five decimals)
    assert abs(got - ref) <= 2 * CM.BLACK_SKY_GRID_DISTANCE[U, mu0, N]


def test_a_smooth_sea_at_a_high_sun_reflects_fresnel():
    """U = 2, mu0 = 0.9: the hemispherical integral of the narrow glint is the Fresnel reflectance at mu0 to a percent"""
    assert abs(fine(2, 0.9) - CM.fresnel(0.9)) <= 0.01 * CM.fresnel(0.9)


def test_the_grazing_values_are_not_clamped():
    """N = 128, U = 2, shadowing on: the directional-hemispherical reflectance at the lowest node is 1.07 on the grid's trapezoid"""
    N = 128
    mu = O.make_mu(N)
    dhr = CM.black_sky_grid(mu, N, mu[N + 1], ("cox_munk", CM.slope_variance(2), CM.INDEX, True))
    assert abs(dhr - 1.07) <= 0.005


def test_ocean_helpers():
    from sosrt import ocean
    assert ocean.slope_variance(0) == 0.003 and abs(ocean.slope_variance(10.0) - 0.0542) <= 1e-16
    assert np.allclose(ocean.slope_variance([2, 5]), [CM.slope_variance(2), CM.slope_variance(5)], rtol=0, atol=1e-17)
    assert ocean.whitecap_fraction(0) == 0 and abs(ocean.whitecap_fraction(10.0) - 2.95e-6 * 10 ** 3.52) <= 1e-18
    assert "f_iso" in ocean.__doc__ or "W * 0.22" in ocean.__doc__


# ---- refusals of the Python layer, before any handle exists --------------------------------------------------------------------------------
CM_OK = dict(surface="brdf", brdf=("cox_munk", 5.0))
BATCH_REFUSALS = [
    (dict(surface="brdf", brdf=("cox_munk",)), "brdf must be"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, 1.0, True, 0.0)), "Cox-Munk brdf is"),
    (dict(surface="brdf", brdf=("cox_munk", "fast")), "must be numbers"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, None)), "must be numbers"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, "a")), "must be numbers"),
    (dict(surface="brdf", brdf=("cox_munk", -1.0)), "wind_speed"),
    (dict(surface="brdf", brdf=("cox_munk", float("nan"))), "wind_speed"),
    (dict(surface="brdf", brdf=("cox_munk", float("inf"))), "wind_speed"),
    (dict(surface="brdf", brdf=("cox_munk", [1.0, 2.0])), "wind_speed"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.0)), "refractive_index"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 0.9)), "refractive_index"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, float("nan"))), "refractive_index"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, -0.1)), "f_iso, f_glint"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, float("inf"))), "f_iso, f_glint"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, [0.1, 0.2])), "f_iso, f_glint"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, 0.0)), "both zero"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, [0.0] * 4, [0.0] * 4)), "both zero"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, 1.0, 2)), "shadow"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, 1.0, 0.5)), "shadow"),
    (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.34, 0.0, 1.0, "yes")), "shadow"),
    (dict(surface="brdf", brdf=("cox_munk", [1.0, 2.0, 3.0, 4.0])), "one call per wind"),
    (dict(surface="brdf", brdf=("cox-munk", 5.0, 0.0, 0.0)), "named brdf"),
    (dict(surface="brdf", brdf=("cox_munk ", 5.0)), "named brdf"),
    (dict(surface="brdf", brdf="cox_munk"), "brdf must be"),
    (dict(brdf=("cox_munk", 5.0)), "surface='brdf'"),
    (dict(surface="lambertian", brdf=("cox_munk", 5.0)), "surface='brdf'"),
    # everything ('ross_li', ...) refuses by combination
    (dict(CM_OK, azimuths=[0.0]), "m = 0"),
    (dict(CM_OK, azimuths=[0.0], mode_batch=True), "m = 0"),
    (dict(CM_OK, azimuths=[0.0], brdf_modes=True, mode_batch=True), "mode_batch"),
    (dict(CM_OK, azimuths=[0.0], brdf_modes=True, mode_chunk=2), "mode_batch"),
    (dict(CM_OK, azimuths=[0.0], brdf_modes=True, n_modes=64), "n_modes must be <= 63"),
    (dict(CM_OK, brdf_modes=True), "give azimuths"),
    (dict(CM_OK, view_mu=[0.5]), "view_mu"),
    (dict(CM_OK, view_mu=[0.5], view_azimuths=[0.0]), "m = 0"),
    (dict(CM_OK, brdf_view=True), "give view_mu"),
    (dict(CM_OK, view_mu=[0.5], brdf_view=True, azimuths=[0.0]), "brdf_view=True"),
    (dict(CM_OK, view_mu=[0.5], brdf_view=True, view_azimuths=[0.0], n_modes=64), "n_modes must be <= 63"),
    (dict(CM_OK, beam="spherical"), "spherical"),
    (dict(CM_OK, source="thermal", planck=np.ones(24), planck_surface=1.0), "thermal"),
    (dict(CM_OK, first_order="readme"), "readme"),
    (dict(CM_OK, devices=[0, 1]), "devices"),
    (dict(CM_OK, save_orders=True), "save_orders"),
    (dict(CM_OK, nb_angles=3), "nb_angles >= 4"),
]


@pytest.mark.parametrize("bad,word", BATCH_REFUSALS, ids=lambda x: x if isinstance(x, str) else None)
def test_batch_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import dist, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    with pytest.raises(ValueError) as ei:
        main.SOS_Aer_batch([0.5, 0.6, 0.7, 0.8], 0.3, 1.0, **dict(KW, **bad))
    assert word in str(ei.value), str(ei.value)


def test_the_message_for_too_many_winds_names_the_way_out():
    from sosrt import main
    with pytest.raises(ValueError) as ei:
        main._brdf_args("brdf", ("cox_munk", [1.0, 2.0, 3.0, 4.0]), 1.0, 32, 4)
    assert "at most 3 distinct wind speeds" in str(ei.value) and "got 4" in str(ei.value) and "one call per wind" in str(ei.value)


def test_the_scale_is_checked_before_any_handle(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    for grd_alb in (0.5, [1.0, 1.0, 0.9, 1.0], 0.0):
        with pytest.raises(ValueError, match="omitted or 1"):
            main.SOS_Aer_batch([0.5, 0.6, 0.7, 0.8], 0.3, grd_alb, surface="brdf", brdf=("cox_munk", 5.0), **KW)


def test_other_drivers_refuse_before_any_handle(monkeypatch):
    from sosrt import forcing, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(forcing, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    for bad, word in ((dict(surface="brdf", brdf=("cox_munk", -2.0)), "wind_speed"), (dict(surface="brdf", brdf=("cox_munk", 5.0, 1.0)), "refractive_index"),
                      (dict(CM_OK, beam="spherical"), "spherical")):
        calls = [lambda: main.solve_batch_device([0.5, 0.6], 0.3, 1.0, **KW, **bad),
                 lambda: main.SOS_Aer_layers([0.5, 0.6], 1.0, [(25, 17, 0.3, 0.9)], **KW, **bad),
                 lambda: main.SOS_Aer(grd_alb=1.0, **KW, **bad),
                 lambda: forcing.toa_net_flux(0.5, 0.124, [0.1, 0.2], 1.0, 1.0, 0.9, **KW, **bad),
                 lambda: forcing.radiative_forcing(0.5, 0.124, [0.1, 0.2], 1.0, 1.0, 0.9, **KW, **bad),
                 lambda: forcing.critical_albedo(0.5, 0.124, [0.1, 0.2], 1.0, 1.0, **KW, **bad)]
        for call in calls:
            with pytest.raises(ValueError) as ei:
                call()
            assert word in str(ei.value), str(ei.value)


# ---- the ground a valid call constructs ------------------------------------------------------------------------------------------------------
def test_defaults_of_a_valid_ground():
    from sosrt import main, ocean
    a = main._brdf_args("brdf", ("cox_munk", 5.0), 1.0, 32, 3)
    assert a.kind == "cox_munk" and a.R is None and a.r0 is None and not a.modes and not a.view
    assert a.terms == (("lambertian", ()), ("cox_munk", (float(ocean.slope_variance(5.0)), 1.34, 1.0)))
    assert np.array_equal(a.weight, [[0.0, 1.0]] * 3) and a.weight.flags.c_contiguous and a.weight.dtype == np.float64
    b = main._brdf_args("brdf", ["cox_munk", 5.0, 1.5, 0.02, 0.9, False], 1, 32, 3, azimuths=[0.0], brdf_modes=True)
    assert b.terms[1] == ("cox_munk", (float(ocean.slope_variance(5.0)), 1.5, 0.0)) and b.modes
    assert np.array_equal(b.weight, [[0.02, 0.9]] * 3)
    for shadow, flag in ((True, 1.0), (1, 1.0), (np.bool_(False), 0.0), (0.0, 0.0)):
        assert main._brdf_args("brdf", ("cox_munk", 5.0, 1.34, 0.0, 1.0, shadow), 1.0, 32, 1).terms[1][1][2] == flag
    assert main._brdf_args("brdf", ("cox_munk", 0.0), 1.0, 32, 1).terms[1][1][0] == 0.003          # a calm sea is a valid ground


def test_mixed_winds_are_one_hot_weights_over_ascending_terms():
    from sosrt import main, ocean
    f_iso, f_glint = [0.0, 0.01, 0.02, 0.03], [1.0, 0.9, 0.8, 0.7]
    a = main._brdf_args("brdf", ("cox_munk", [10.0, 2.0, 10.0, 5.0], 1.34, f_iso, f_glint), 1.0, 32, 4)
    assert [t[0] for t in a.terms] == ["lambertian", "cox_munk", "cox_munk", "cox_munk"] and len(a.terms) <= main._lib.BRDF_MAX_TERMS
    assert [t[1][0] for t in a.terms[1:]] == [float(ocean.slope_variance(u)) for u in (2.0, 5.0, 10.0)]
    assert np.array_equal(a.weight, [[0.0, 0, 0, 1.0], [0.01, 0.9, 0, 0], [0.02, 0, 0, 0.8], [0.03, 0, 0.7, 0]])
    # a column's own terms are those of the batch at its wind alone, with the same weights
    one = main._brdf_args("brdf", ("cox_munk", 10.0, 1.34, [0.0, 0.02], [1.0, 0.8]), 1.0, 32, 2)
    assert one.terms == (a.terms[0], a.terms[3]) and np.array_equal(one.weight, a.weight[[0, 2]][:, [0, 3]])
    # a scalar wind with weights per column; f_glint = 0 leaves the isotropic ground
    b = main._brdf_args("brdf", ("cox_munk", [3.0], 1.34, [0.1, 0.2, 0.3, 0.4], 0.0), 1.0, 32, 4)
    assert len(b.terms) == 2 and np.array_equal(b.weight, np.stack([[0.1, 0.2, 0.3, 0.4], [0.0] * 4], axis=1))
