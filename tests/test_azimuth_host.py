"""Azimuth-resolved radiance (SOS_Aer_batch(..., azimuths=...)), CPU tier: the checks the Python layer makes
before any handle exists, and the NumPy restatement of the Fourier-mode builders the GPU tests compare against."""
import numpy as np
import pytest

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
