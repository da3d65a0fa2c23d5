"""Pseudo-spherical direct beam (beam='spherical'), CPU tier: the three symbols of the C ABI, the NumPy model
of the stage (tests/spherical_np.py) pinned to a closed form, to its plane limit and -- fed the plane path tau / mu0 -- to the
reference's three-zone first order and whole solves, the size of the sphere's effect, and the checks the Python layer makes
before any handle exists.  No GPU."""
import os
import re

import numpy as np
import pytest

import sos_oracle as O
import spherical_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_beam_slant_dev": 7, "sosrt_first_order_beam_dev": 7, "sosrt_epilogue_beam_dev": 12}


def _err(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


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
    for meth in ("beam_slant_device", "first_order_beam_device", "epilogue_beam_device"):
        assert callable(getattr(Solver, meth))


# ---- the slant path -----------------------------------------------------------------------------------------------------------
# Bars.  The model's radicand r_k^2 - r_t^2 (1 - mu0^2) is a difference of two numbers of size r^2 whose value is >= r^2 mu0^2:
# its relative rounding error is up to 2^-52 / mu0^2 (9e-14 at mu0 = 0.05), half of that in the square root, and the closed
# form has the same cancellation.  1e-12 bounds both at every mu0 >= 0.05 of these tests.
@pytest.mark.parametrize("mu0", [0.05, 0.2, 0.9, 1.0])
def test_slant_model_against_the_uniform_closed_form(mu0):
    L = 24
    z = S.altitudes(L)
    tau = np.arange(L) * S.T_ATM / (L - 1)                      # the molecular-only profile: uniform extinction in z
    sig = S.slant_path(tau, z, mu0)
    ref = S.slant_uniform_closed_form(z, mu0, S.T_ATM / S.Z0)
    print("mu0 = %g: slant model vs closed form %.3e" % (mu0, _err(sig, ref)))
    assert sig[0] == 0
    assert _err(sig, ref) <= 1e-12
    if mu0 == 1.0:
        assert np.max(np.abs(sig - tau)) <= 1e-15


@pytest.mark.parametrize("mu0", [0.05, 0.21, 0.6])
def test_slant_model_tends_to_the_plane_path(mu0):
    c = S.column(O, 32, 24, mu0, 0.3)
    z = S.altitudes(24)
    plane = S.plane_path(c.tau, mu0)
    e15 = _err(S.slant_path(c.tau, z, mu0, 1e15), plane)
    print("mu0 = %g: |sigma(R = 1e15) - tau / mu0| = %.3e of the maximum" % (mu0, e15))
    assert e15 <= 1e-10
    # the distance goes as 1 / R
    d9, d12 = (_err(S.slant_path(c.tau, z, mu0, R), plane) for R in (1e9, 1e12))
    assert 0.5e-3 * d9 < d12 < 2e-3 * d9
    # and the sphere shortens the path: never longer than the secant law, shorter at the ground
    sig = S.slant_path(c.tau, z, mu0)
    assert np.all(sig <= plane * (1 + 1e-14)) and sig[-1] < plane[-1]


def test_slant_ratio_at_the_ground():
    """The figures of DESIGN section 17: slant / secant optical path at the ground of the tests' column."""
    for mu0, want in ((0.83, 0.998), (0.6, 0.991), (0.21, 0.913)):
        c = S.column(O, 32, 200, mu0, 0.3)
        r = S.slant_path(c.tau, S.altitudes(200), mu0)[-1] / (c.tau[-1] / mu0)
        assert abs(r - want) < 2e-3, (mu0, r)


# ---- the first order on the plane path is the reference's ---------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FIRST_ORDER_CASES, ids=lambda c: "N%d-L%d-mu0_%g-rho%g%s" % (c[:4] + ("-2slabs" if len(c) > 4 else "",)))
def test_first_order_model_on_the_plane_path_is_the_oracle(case):
    assert S.node_distance(case[0], case[2]) >= 1e-3
    c = S.column(O, *case)
    ref = O.first_order(c)
    got = S.first_order_beam(c, S.plane_path(c.tau, c.mu0))
    e = _err(got, ref)
    print("%s: layer-by-layer model vs oracle.first_order %.3e" % (case[:4], e))
    assert np.all(np.isfinite(got))
    assert e <= 1e-10


def test_first_order_model_near_a_node_differs_by_the_limit_branch_only():
    """mu0 = 0.613 is 9.7e-5 from a node of N = 32: the reference takes its approximate limit form on that lane, the model
    is exact there.  The distance is of the size of that approximation (1e-4 of the maximum), and confined to the lane."""
    N, mu0 = 32, 0.613
    assert S.node_distance(N, mu0) < 1e-4
    c = S.column(O, N, 24, mu0, 0.3)
    ref, got = O.first_order(c), S.first_order_beam(c, S.plane_path(c.tau, mu0))
    d = np.max(np.abs(got - ref), axis=0) / np.max(np.abs(ref))
    near = np.abs(np.abs(c.mu) - mu0) < 1e-4
    assert near.sum() == 2
    assert np.max(d[~near]) <= 1e-10
    assert 1e-7 < np.max(d[near]) <= 2e-4


@pytest.mark.parametrize("case", S.SOLVE_CASES, ids=lambda c: "N%d-L%d-mu0_%g-rho%g%s" % (c[:4] + ("-2slabs" if len(c) > 4 else "",)))
def test_whole_solve_from_the_plane_path_model_is_the_oracle_solve(case):
    c = S.column(O, *case)
    ref = O.solve_column(c, literal=False)
    got = O.solve_column(c, literal=False, I1=S.first_order_beam(c, S.plane_path(c.tau, c.mu0)))
    e = _err(got.I, ref.I)
    print("%s: n = %d / %d, field %.3e" % (case[:4], got.n, ref.n, e))
    assert got.n == ref.n
    assert e <= 1e-10


# ---- the sphere's effect is not zero ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0,least", [(0.6, 1e-3), (0.21, 3e-2)])
def test_the_sphere_moves_the_first_order(mu0, least):
    c = S.column(O, 32, 24, mu0, 0.3)
    plane = S.first_order_beam(c, S.plane_path(c.tau, mu0))
    sph = S.first_order_beam(c, S.slant_path(c.tau, S.altitudes(24), mu0))
    e = _err(sph, plane)
    print("mu0 = %g: the first order moves by %.3e of its maximum" % (mu0, e))
    assert e > least


def test_beam_flux_terms_on_the_plane_path_are_the_oracle_fluxes():
    c = S.column(O, 32, 24, 0.45, 0.3)
    I = O.first_order(c)
    for norm in ("crit", "graphe"):
        fd, fu = O.fluxes(I, c.mu, c.tau, c.N, c.mu0, c.grd_alb, beam_norm=norm)
        e = S.epilogue_beam(I, c.mu, c.tau, S.plane_path(c.tau, c.mu0), c.N, c.mu0, c.grd_alb, beam_norm=norm)
        assert _err(e["flux_down"], fd) <= 1e-13 and _err(e["flux_up"], fu) <= 1e-13
    z = S.altitudes(24)
    e = S.epilogue_beam(I, c.mu, c.tau, S.plane_path(c.tau, c.mu0), c.N, c.mu0, c.grd_alb, z_profile=z, slabs=[(c.idx_up, c.idx_down)])
    assert _err(e["heating_rate"], O.heating_rate(I, c.mu, c.tau, c.N, c.mu0, c.grd_alb, z, c.idx_up, c.idx_down)) <= 1e-10
    assert abs(e["net_toa"] - O.toa_net_flux(I, c.mu, c.tau, c.N, c.mu0, c.grd_alb)) <= 1e-13


# ---- the Python layer refuses before any handle exists -----------------------------------------------------------------------------
BATCH_REFUSALS = [
    (dict(beam="sphere"), "beam must be"),
    (dict(beam=None), "beam must be"),
    (dict(beam="spherical", earth_radius=0.0), "earth_radius"),
    (dict(beam="spherical", earth_radius=-6371.0), "earth_radius"),
    (dict(beam="spherical", earth_radius=float("nan")), "earth_radius"),
    (dict(beam="spherical", earth_radius=float("inf")), "earth_radius"),
    (dict(beam="spherical", azimuths=[0.0, 1.0]), "azimuths"),
    (dict(beam="spherical", azimuths=[0.0], mode_batch=True), "azimuths"),
    (dict(beam="spherical", view_mu=[0.5]), "view_mu"),
    (dict(beam="spherical", view_mu=[0.5], view_azimuths=[0.0]), "view_mu"),
    (dict(beam="spherical", first_order="readme"), "readme"),
    (dict(beam="spherical", devices=[0, 1]), "devices"),
]


@pytest.mark.parametrize("bad,word", BATCH_REFUSALS, ids=[" ".join("%s=%r" % kv for kv in b.items()) for b, _ in BATCH_REFUSALS])
def test_batch_refusals_before_any_handle(bad, word, monkeypatch):
    from sosrt import dist, main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    monkeypatch.setattr(dist, "solve_on_devices", lambda *a, **k: pytest.fail("workers were started"))
    with pytest.raises(ValueError, match=word):
        main.SOS_Aer_batch([0.5, 0.6], 0.3, 0.2, nb_layers=24, nb_angles=32, **bad)


@pytest.mark.parametrize("bad,word", [(dict(beam="round"), "beam must be"), (dict(beam="spherical", earth_radius=-1.0), "earth_radius")])
def test_other_drivers_refuse_before_any_handle(bad, word, monkeypatch):
    from sosrt import forcing, main
    stop = lambda *a, **k: pytest.fail("a handle was requested")
    monkeypatch.setattr(main, "get_solver", stop)
    monkeypatch.setattr(forcing, "get_solver", stop)
    with pytest.raises(ValueError, match=word):
        main.solve_batch_device([0.5], 0.3, 0.2, nb_layers=24, nb_angles=32, **bad)
    with pytest.raises(ValueError, match=word):
        main.SOS_Aer_layers([0.5], 0.2, [(25, 17, 0.12, 0.97)], nb_layers=24, nb_angles=32, **bad)
    with pytest.raises(ValueError, match=word):
        main.SOS_Aer(nb_layers=24, nb_angles=32, **bad)
    with pytest.raises(ValueError, match=word):
        main.SOS_Aer_spectrum([0.55], [0.5], 0.3, 0.2, dict(m=1.44, r_m=0.5, sig=1.2), nb_layers=24, nb_angles=32, **bad)
    for fn in (forcing.toa_net_flux, forcing.radiative_forcing):
        with pytest.raises(ValueError, match=word):
            fn(0.5, 0.124, [0.3], 0.2, 1.0, [0.9], nb_layers=24, nb_angles=32, **bad)
    with pytest.raises(ValueError, match=word):
        forcing.critical_albedo(0.5, 0.124, [0.3], 0.2, 1.0, nb_layers=24, nb_angles=32, **bad)


def test_single_column_driver_refuses_the_readme_first_order(monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="readme"):
        main.SOS_Aer(beam="spherical", first_order="readme", nb_layers=24, nb_angles=32)


def test_spectrum_never_solves_plane_silently(monkeypatch):
    """SOS_Aer_spectrum hands `beam` and `earth_radius` to every batch it solves (or refuses what the batch refuses)."""
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError, match="view_mu"):
        main.SOS_Aer_spectrum([0.55], [0.5], 0.3, 0.2, dict(m=1.44, r_m=0.5, sig=1.2), beam="spherical", view_mu=[0.5])
    import inspect
    src = inspect.getsource(main.SOS_Aer_spectrum)
    assert src.count("**batch_kw") >= 2                       # both of its SOS_Aer_batch calls take the caller's keywords


def test_plane_is_the_default_everywhere():
    import inspect
    from sosrt import forcing, main
    for fn in (main.SOS_Aer_batch, main.solve_batch_device, main.SOS_Aer_layers, main.SOS_Aer, forcing.toa_net_flux):
        p = inspect.signature(fn).parameters
        assert p["beam"].default == "plane" and p["earth_radius"].default == 6371.0, fn.__name__
