"""Pseudo-spherical beam in the azimuth and view stages (beam='spherical' with beam_stages=True), CPU tier: the
symbol of the C ABI, the NumPy model of the first order at view lanes (tests/spherical_view_np.py) pinned to the grid's model at
the nodes, the Fourier modes on a beam path against a direct azimuth-resolved solve on the same path, the size of the sphere's
effect at a view lane, and the checks the Python layer makes before any handle exists.  No GPU."""
import os
import re

import numpy as np
import pytest

import azimuth_direct as AD
import sos_oracle as O
import spherical_np as S
import spherical_view_np as SV
import view_np as VN
from sosrt import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_symbol_declared_bound_and_exported():
    from sosrt import _lib
    from sosrt.solver import Solver
    name, nargs = "sosrt_view_first_order_beam_dev", 12
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "%s is not declared in sosrt.h" % name
    assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
    assert getattr(_lib.lib(), name) is not None, "%s is not exported" % name
    declared = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    assert len(_lib.SIGNATURES[name][1]) == declared == nargs
    assert callable(Solver.view_first_order_beam_device)


# ---- the view model at the grid's nodes is the grid's model ------------------------------------------------------------------------
NODE_CASES = [(32, 24, 0.6, 0.3), (33, 24, 0.83, 0.5), (32, 24, 0.05, 0.3), (32, 48, 0.6, 0.3, S.TWO_SLABS)]


@pytest.mark.parametrize("path", ["sphere", "plane"])
@pytest.mark.parametrize("case", NODE_CASES, ids=lambda c: "N%d-L%d-mu0_%g-rho%g%s" % (c[:4] + ("-2slabs" if len(c) > 4 else "",)))
def test_view_model_at_the_nodes_is_the_grid_model(case, path):
    """View cosines equal to grid nodes, the grid's P0 values as p0 rows: the rows of spherical_np.first_order_beam at those
    directions.  The two models share their definitions and differ in rounding only (1 / a, the mirror's cosine to an ulp)."""
    c = S.column(O, *case)
    L = case[1]
    sig = S.slant_path(c.tau, S.altitudes(L), c.mu0) if path == "sphere" else S.plane_path(c.tau, c.mu0)
    mv, idx = VN.node_views(c.mu, c.N)
    ref = S.first_order_beam(c, sig)[:, idx]
    got = SV.view_first_order_beam(c, sig, c.P0_atm[idx], c.P0_aer[idx], mv)
    e = _err(got, ref)
    print("%s %s: view model at %d nodes vs grid model %.3e" % (case[:4], path, len(mv), e))
    assert np.all(np.isfinite(got))
    assert e <= 1e-13


def test_view_model_is_finite_and_smooth_across_mu0():
    """A view cosine equal to mu0, and 1e-5 to either side: phi is exact there, so the three lanes agree to the size of the step."""
    c = S.column(O, 32, 24, 0.6, 0.3)
    sig = S.slant_path(c.tau, S.altitudes(24), 0.6)
    mv = np.array([0.6 - 1e-5, 0.6, 0.6 + 1e-5, 0.01, 1.0])
    fn_a, fn_r = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7)
    sgn = VN.signed(mv)
    out = SV.view_first_order_beam(c, sig, VN.phase_p0_rows(fn_a, c.mu, [0.6], sgn)[0], VN.phase_p0_rows(fn_r, c.mu, [0.6], sgn)[0], mv)
    assert np.all(np.isfinite(out))
    top = np.max(np.abs(out))
    assert np.max(np.abs(out[:, [0, 2, 5, 7]] - out[:, [1, 1, 6, 6]])) <= 1e-3 * top


# ---- the size of the effect at a view lane (the figures of DESIGN section 27) -------------------------------------------------------
def effect_at_toa(mu0, N, L=24):
    """(first order, converged radiance) at TOA on the upward grid lanes >= 0.01: the largest |sphere - plane| over the largest
    plane value.  The converged field is the oracle's from the model's first order; at a node the view stage follows the field.
    (N, L, mu0) are whole-solve columns of DESIGN section 17: the reference's mu -> 0+ search stays on the grid on both paths.)"""
    c = S.column(O, N, L, mu0, 0.3)
    plane, sph = S.plane_path(c.tau, mu0), S.slant_path(c.tau, S.altitudes(L), mu0)
    up = np.flatnonzero(c.mu >= 0.01)
    f = [S.first_order_beam(c, p)[0, up] for p in (plane, sph)]
    I = [O.solve_column(c, literal=False, I1=S.first_order_beam(c, p)).I[0, up] for p in (plane, sph)]
    return _err(f[1], f[0]), _err(I[1], I[0])


@pytest.mark.parametrize("mu0,N", [(0.21, 64), (0.6, 32)])
def test_the_sphere_moves_the_toa_view_radiance(mu0, N):
    """The bar of the device test, 1e-3 of the maximum: section 17's grid first order moves by 4 % at mu0 = 0.21 and by 0.3 % at 0.6."""
    assert (N, 24, mu0, 0.3) in S.SOLVE_CASES
    first, conv = effect_at_toa(mu0, N)
    print("mu0 = %g: TOA upward lanes move by %.3e (first order) and %.3e (converged) of their maximum" % (mu0, first, conv))
    assert first > 1e-3 and conv > 1e-3


# ---- the modes on a beam path against a direct azimuth-resolved solve on the same path ------------------------------------------------
SCALE = 1e-6
MODE_CASES = {  # mu0, L, N, aerosol phase function, orders, M, nq
    "rayleigh": (0.6, 60, 64, ("rayleigh", 0.0), 3, 2, 8),
    "rayleigh_hg": (0.6, 60, 64, ("hg", 0.5), 3, 32, 96),
}


@pytest.mark.parametrize("name", list(MODE_CASES))
def test_modes_on_the_sphere_are_the_direct_solve(name):
    mu0, L, N, aer, K, M, nq = MODE_CASES[name]
    fa, fr = inputs._scalar_phase("rayleigh", 0.0)[0], inputs._scalar_phase(*aer)[0]
    geo, _ = SV.sphere_geometry(mu0, L, N)
    plane = AD.three_zone(mu0, L, N)
    with AD.record_blend() as log:
        phi, Iq = AD.direct_solve(geo, fa, fr, nq, K, SCALE)
        Im = AD.mode_fields(geo, fa, fr, M, nq // 2 + 1, K, SCALE)
    assert log and all(log)
    e = _err(AD.project(Iq, M), Im)
    print("%s: modes 0..%d on the sphere vs the direct solve's projection %.3e" % (name, M, e))
    assert e <= 1e-13
    if name == "rayleigh":                                     # no mode above 2: the synthesis is exact too
        assert _err(np.moveaxis(AD.synthesize(Im, phi), -1, 0), Iq) <= 1e-13
        # and the test has teeth: the plane first order is not the sphere's
        assert _err(AD.mode_fields(plane, fa, fr, M, nq // 2 + 1, K, SCALE), Im) > 1e-4


# ---- the Python layer: accepted and refused before any handle exists -------------------------------------------------------------------
class _Reached(Exception):
    pass


def _stub(monkeypatch, reach):
    from sosrt import dist, main

    def got(*a, **k):
        if reach:
            raise _Reached()
        pytest.fail("a handle was requested")
    monkeypatch.setattr(main, "get_solver", got)
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    return main


SPH = dict(beam="spherical", beam_stages=True)
ACCEPTED = [
    dict(SPH),
    dict(SPH, azimuths=[0.0, 1.0]),
    dict(SPH, view_mu=[0.5]),
    dict(SPH, view_mu=[0.5, 0.21], view_azimuths=[0.0, 2.0]),
    dict(SPH, view_mu=[0.5], view_azimuths=[0.0], view_first_order="modes"),
    dict(SPH, earth_radius=1e15, view_mu=[1.0]),
]


@pytest.mark.parametrize("kw", ACCEPTED, ids=[" ".join("%s=%r" % kv for kv in k.items()) for k in ACCEPTED])
def test_stages_are_accepted_with_beam_stages(kw, monkeypatch):
    main = _stub(monkeypatch, reach=True)
    with pytest.raises(_Reached):
        main.SOS_Aer_batch([0.5, 0.6], 0.3, 0.2, nb_layers=24, nb_angles=32, **kw)


REFUSED = [
    (dict(beam="plane", beam_stages=True), "beam_stages"),
    (dict(beam_stages=True), "beam_stages"),
    (dict(beam="plane", beam_stages=True, view_mu=[0.5]), "beam_stages"),
    (dict(SPH, beam_stages=1), "beam_stages"),
    (dict(SPH, azimuths=[0.0], mode_batch=True), "mode_batch"),
    (dict(SPH, azimuths=[0.0], mode_batch=True, mode_chunk=2), "mode_batch"),
    (dict(SPH, view_mu=[0.5], surface="brdf", brdf="lambertian", brdf_view=True), "spherical"),
    (dict(SPH, azimuths=[0.0], surface="brdf", brdf="lambertian", brdf_modes=True), "spherical"),
    (dict(SPH, view_mu=[0.5], source="thermal", planck=np.ones(24), planck_surface=1.0), "spherical"),
    (dict(SPH, first_order="readme"), "readme"),
    (dict(SPH, view_mu=[0.5], first_order="readme"), "readme"),
    (dict(SPH, view_mu=[0.5], devices=[0, 1]), "devices"),
    (dict(SPH, azimuths=[0.0], devices=[0, 1]), "devices"),
    (dict(SPH, earth_radius=-1.0, view_mu=[0.5]), "earth_radius"),
    # what the stages refuse on the plane beam they refuse on the sphere
    (dict(SPH, view_mu=[0.5], azimuths=[0.0]), "view_mu"),
    (dict(SPH, view_mu=[0.001]), "view_mu"),
    (dict(SPH, view_azimuths=[0.0]), "view_mu"),
    (dict(SPH, view_mu=[0.5], surface="lambertian"), "specular"),
    # without the keyword the refusals are those of before, word for word
    (dict(beam="spherical", azimuths=[0.0, 1.0]), "is not available with azimuths / mode_batch: the first order of a Fourier mode m >= 1 is the plane closed form"),
    (dict(beam="spherical", azimuths=[0.0], mode_batch=True), "is not available with azimuths / mode_batch: the first order of a Fourier mode m >= 1 is the plane closed form"),
    (dict(beam="spherical", view_mu=[0.5]), "is not available with view_mu / view_azimuths: the first order at a view cosine is the plane closed form"),
    (dict(beam="spherical", view_mu=[0.5], view_azimuths=[0.0]), "is not available with view_mu / view_azimuths: the first order at a view cosine is the plane closed form"),
    (dict(beam="spherical", beam_stages=False, view_mu=[0.5]), "is not available with view_mu / view_azimuths"),
]


@pytest.mark.parametrize("bad,word", REFUSED, ids=[" ".join("%s=%r" % (k, v if not isinstance(v, np.ndarray) else "array") for k, v in b.items()) for b, _ in REFUSED])
def test_refusals_before_any_handle(bad, word, monkeypatch):
    main = _stub(monkeypatch, reach=False)
    with pytest.raises(ValueError, match=re.escape(word)) as ei:
        main.SOS_Aer_batch([0.5, 0.6], 0.3, 0.2, nb_layers=24, nb_angles=32, **bad)
    assert len(str(ei.value)) > len(word) or ":" in word       # a refusal says why


def test_spectrum_passes_beam_stages_on(monkeypatch):
    main = _stub(monkeypatch, reach=False)
    with pytest.raises(ValueError, match="beam_stages"):
        main.SOS_Aer_spectrum([0.55], [0.5], 0.3, 0.2, dict(m=1.44, r_m=0.5, sig=1.2), beam_stages=True)
    with pytest.raises(ValueError, match="view_mu"):
        main.SOS_Aer_spectrum([0.55], [0.5], 0.3, 0.2, dict(m=1.44, r_m=0.5, sig=1.2), beam="spherical", view_mu=[0.5])


def test_the_keyword_defaults_to_off():
    import inspect
    from sosrt import main
    assert inspect.signature(main.SOS_Aer_batch).parameters["beam_stages"].default is False
    assert inspect.signature(main._beam_args).parameters["beam_stages"].default is False
    for fn in (main.view_radiance, main.azimuth_modes, main.view_azimuth_modes, main._solve_modes):
        assert inspect.signature(fn).parameters["sigma"].default is None, fn.__name__
