"""Azimuth-resolved radiance (SOS_Aer_batch(..., azimuths=...)), CPU tier: the checks the Python layer makes
before any handle exists, the NumPy restatement of the Fourier-mode builders the GPU tests compare against, and that
restatement against a direct azimuth-resolved solve (tests/azimuth_direct.py)."""
import numpy as np
import pytest

import azimuth_direct as D
import azimuth_np as A
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch

PHI = np.linspace(0, np.pi, 7)


@pytest.mark.parametrize("kw", [
    dict(P_atm=np.ones((256, 256))), dict(P_aer=np.ones((256, 256))), dict(P0_atm=np.ones(256)), dict(P0_aer=np.ones(256)),
    dict(surface="lambertian"), dict(surface="lambertian_readme"), dict(first_order="readme"), dict(devices=[0, 1]),
    dict(n_modes=0), dict(n_modes=_lib.MAX_MODES + 1), dict(n_modes=30, nphi_modes=31), dict(levels=(0, 200)),
    dict(levels=()), dict(azimuths=np.zeros((2, 2))), dict(azimuths=[]), dict(azimuths=[0.0, np.nan]),
], ids=lambda kw: ",".join(sorted(kw)) + "=" + str(list(kw.values())[0])[:12])
def test_azimuth_arguments_raise_before_any_handle(kw, monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    kw = dict(kw)
    az = kw.pop("azimuths", PHI)
    with pytest.raises(ValueError):
        SOS_Aer_batch(0.5, 0.2, 0.1, nb_layers=200, nb_angles=128, azimuths=az, **kw)


@pytest.mark.parametrize("name,g", [("rayleigh", 0.0), ("hg", 0.7), ("hg", -0.3), ("fwc", 0.0)])
@pytest.mark.parametrize("N", [8, 13])
def test_numpy_mode_zero_is_the_azimuth_average(name, g, N):
    """Mode 0 of the restated builder at nphi = 25 is inputs.phase_function exactly (P0 and P)."""
    mu = inputs.direction_grid(N)
    fn = inputs._scalar_phase(name, g)[0]
    P0, P = inputs.phase_function(name, N, mu, 0.6, g)
    assert np.array_equal(A.phase_modes(fn, mu, [0], 25)[0], P)
    assert np.array_equal(A.phase_p0_modes(fn, mu, 0.6, [0], 25)[0], P0)


def test_numpy_modes_sum_to_the_phi_resolved_phase_function():
    """sum_m (2 - delta_m0) P0^m cos(m phi) = p(c(mu, mu0, phi)) / Z0 (HG g = 0.7, nphi = 401, M = 60), Rayleigh modes m >= 3
    vanish, and the modes keep the flip symmetry P^m(-mu, -mu') = P^m(mu, mu')."""
    N, mu0 = 16, 0.55
    mu = inputs.direction_grid(N)
    fn = inputs._scalar_phase("hg", 0.7)[0]
    M, nphi = 60, 401
    P0m = A.phase_p0_modes(fn, mu, mu0, range(M + 1), nphi)
    for phi in (0.0, 0.4, 1.3, 2.9, np.pi):
        syn = sum((1 if m == 0 else 2) * P0m[m] * np.cos(m * phi) for m in range(M + 1))
        ref = A.p0_direct(fn, mu, mu0, phi, nphi)
        assert np.max(np.abs(syn - ref)) <= 1e-9 * np.max(np.abs(ref))
    ray = inputs._scalar_phase("rayleigh")[0]
    Pr = A.phase_modes(ray, mu, range(6), 25)
    assert np.max(np.abs(Pr[3:])) <= 1e-14 * np.max(np.abs(Pr[0]))
    Ph = A.phase_modes(fn, mu, [1, 2, 5], 25)
    assert np.max(np.abs(Ph - Ph[:, ::-1, ::-1])) <= 1e-13 * np.max(np.abs(Ph))


# ---- the modes against a direct azimuth-resolved solve (tests/azimuth_direct.py) -------------------------------------------
# P0 is scaled by 1e-6 so that every search of the oracle's mu -> 0+ upward blend stops at its first test: the blend is then a
# fixed linear map and the solve is linear in P0, so the Fourier decomposition is exact (each test asserts that it was so).
SCALE = 1e-6
CASES = {  # geometry, mu0, L, N, atmosphere (or the slab's) phase function, aerosol phase function, orders
    "rayleigh_three_zone": (D.three_zone, 0.6, 60, 64, ("rayleigh", 0.0), ("rayleigh", 0.0), 3),
    "rayleigh_single_slab": (D.single_slab, 0.55, 40, 64, ("rayleigh", 0.0), None, 4),
    "rayleigh_hg_three_zone": (D.three_zone, 0.6, 60, 64, ("rayleigh", 0.0), ("hg", 0.5), 3),
    "hg_single_slab": (D.single_slab, 0.55, 40, 64, ("hg", 0.5), None, 4),
}


def _case(name):
    geo_of, mu0, L, N, atm, aer, K = CASES[name]
    fa = inputs._scalar_phase(*atm)[0]
    fr = None if aer is None else inputs._scalar_phase(*aer)[0]
    return geo_of(mu0, L, N), fa, fr, K


def _err(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


@pytest.mark.parametrize("name,nq", [("rayleigh_three_zone", 8), ("rayleigh_single_slab", 8), ("rayleigh_hg_three_zone", 48),
                                     ("hg_single_slab", 48)])
def test_direct_azimuth_mean_is_the_mode_zero_solve(name, nq):
    """The mean over nq uniform azimuths of the direct solve is the oracle's azimuth-averaged solve with inputs.phase_function
    (nq = 48 is the reference's 25-node ring itself; Rayleigh is exact on any nq >= 3)."""
    geo, fa, fr, K = _case(name)
    with D.record_blend() as log:
        phi, Iq = D.direct_solve(geo, fa, fr, nq, K, SCALE)
        I0 = D.mode_fields(geo, fa, fr, 0, 25, K, SCALE)[0]
    assert log and all(log)
    assert _err(Iq.mean(axis=0), I0) <= 1e-13


@pytest.mark.parametrize("name,M,nq,tol", [
    ("rayleigh_three_zone", 2, 8, 1e-13), ("rayleigh_single_slab", 2, 8, 1e-13),      # Rayleigh has no mode above 2: exact
    ("rayleigh_hg_three_zone", 32, 96, 1e-10), ("hg_single_slab", 32, 96, 1e-10),     # HG g = 0.5: modes > 32 left out
])
def test_modes_synthesize_the_direct_solve(name, M, nq, tol):
    """sum_m (2 - delta_m0) I^m cos(m phi_q) of the NumPy mode solves (modes m >= 1 on nq / 2 + 1 ring nodes, the same
    quadrature as the direct solve's nq nodes) against the direct solve on every node, row and direction.  For HG the bar is
    the truncation at M = 32 (measured 2.4e-12 three-zone, 1.1e-11 single slab)."""
    geo, fa, fr, K = _case(name)
    with D.record_blend() as log:
        phi, Iq = D.direct_solve(geo, fa, fr, nq, K, SCALE)
        Im = D.mode_fields(geo, fa, fr, M, nq // 2 + 1, K, SCALE)
    assert log and all(log)
    syn = np.moveaxis(D.synthesize(Im, phi), -1, 0)
    assert _err(syn, Iq) <= tol
    assert _err(D.project(Iq, M), Im) <= 1e-13                 # (the same statement mode by mode, without truncation)


def test_the_unsigned_modes_miss_the_direct_solve():
    """Solved with P^m itself, without the factor (-1)^m of the fold (the driver before it), odd modes of orders >= 2 have
    the wrong sign: the synthesis misses the direct solve by 2.5e-3 of the field maximum on the Rayleigh three-zone column,
    at TOA and surface rows too.  This guards against a comparison that cannot tell the two conventions apart."""
    geo, fa, fr, K = _case("rayleigh_three_zone")
    with D.record_blend() as log:
        phi, Iq = D.direct_solve(geo, fa, fr, 8, K, SCALE)
        old = D.mode_fields(geo, fa, fr, 2, 5, K, SCALE, fold_sign=False)
    assert log and all(log)
    syn = np.moveaxis(D.synthesize(old, phi), -1, 0)
    rows = [0, syn.shape[1] - 1]
    assert _err(syn[:, rows], Iq[:, rows]) > 1e-4
