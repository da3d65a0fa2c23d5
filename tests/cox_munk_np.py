"""NumPy model of the Cox-Munk ocean ground, written from the definitions and not from the kernel: the
unpolarised Fresnel reflectance of a real index, Smith's shadowing, the glint of an isotropic Gaussian slope distribution, the
composed ground rho = f_iso + f_glint rho_glint, and its black-sky albedo on the grid's trapezoid and on a fine quadrature.

Importing this module teaches `brdf_np._rho` -- through which brdf_np, brdf_azimuth_np and brdf_view_np resolve a named BRDF --
the names ('cox_munk', sigma2, n, shadow) and ('ocean', f_iso, f_glint, sigma2, n, shadow); every other name goes to the function
it replaced, unchanged (ross_li_np's among them, whichever is imported first)."""
import numpy as np
from scipy.special import erfc

import brdf_np as G

INDEX = 1.34
# |black-sky albedo of the glint (shadow on, n = 1.34) on the grid's trapezoid (make_mu(N), 65 azimuth nodes) - the same on 4001
# cosines x 2049 azimuths|, measured with this model on the CPU; keys (U, mu0, N); the tests assert twice these
BLACK_SKY_FINE = {(5, 0.6): 0.042968, (5, 0.3): 0.13767, (2, 0.9): 0.021840}
BLACK_SKY_GRID_DISTANCE = {(5, 0.6, 64): 1.23e-5, (5, 0.6, 128): 3.01e-6, (5, 0.3, 64): 4.61e-4, (5, 0.3, 128): 1.18e-4,
                           (2, 0.9, 128): 1.09e-5}


def slope_variance(U):
    return 0.003 + 0.00512 * U


def fresnel(c, n=INDEX):
    """F(c) = (r_s^2 + r_p^2) / 2 at the cosine c of the angle of incidence"""
    c = np.asarray(c, dtype=np.float64)
    g = np.sqrt(n * n - 1 + c * c)
    rs, rp = (c - g) / (c + g), (n * n * c - g) / (n * n * c + g)
    return 0.5 * (rs * rs + rp * rp)


def smith_lambda(mu, sigma2):
    """Lambda(mu) = (sqrt(sigma2 / pi) exp(-cot^2 / sigma2) / cot - erfc(cot / sigma)) / 2, cot = mu / sqrt(1 - mu^2); Lambda(1) = 0"""
    mu = np.asarray(mu, dtype=np.float64)
    s = np.sqrt(np.maximum(0.0, 1 - mu * mu))
    with np.errstate(divide="ignore", invalid="ignore"):
        cot = mu / s
        lam = 0.5 * (np.sqrt(sigma2 / np.pi) * np.exp(-cot * cot / sigma2) / cot - erfc(cot / np.sqrt(sigma2)))
    return np.where(s > 0, lam, 0.0)


def shadowing(a, b, sigma2, shadow=True):
    return 1 / (1 + smith_lambda(a, sigma2) + smith_lambda(b, sigma2)) if shadow else np.ones(np.broadcast(a, b).shape)


def rho_glint(a, b, phi, sigma2, n=INDEX, shadow=True):
    """F(cos chi) exp(-t2 / sigma2) (1 + t2)^2 / (4 sigma2 a b) S(a, b); phi = pi is the specular direction.  h2 and cos^2 chi as sums
    of non-negative terms, 1 + cos phi = 2 cos^2(phi / 2): a square of its own and not 2 - 2 sin^2(phi / 2), which next to phi = pi,
    where the glint peaks, is one minus a number next to 1 (3e-12 of the exponent t2 / sigma2 at a = 0.05, b = 0.05004, one node of
    256 from pi: float64 was 9e-13 from long double there, row-wise; tests/brdf_builder_cases.py)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    sa, sb = np.sqrt(np.maximum(0.0, 1 - a * a)), np.sqrt(np.maximum(0.0, 1 - b * b))
    hvc = 2 * np.cos(np.asarray(phi, dtype=np.float64) / 2) ** 2
    h2 = (sa - sb) ** 2 + 2 * sa * sb * hvc
    t2 = h2 / (a + b) ** 2
    cos_chi = np.sqrt((h2 + (a + b) ** 2) / 4)
    return fresnel(cos_chi, n) * np.exp(-t2 / sigma2) * (1 + t2) ** 2 / (4 * sigma2 * a * b) * shadowing(a, b, sigma2, shadow)


def rho_ocean(a, b, phi, f_iso, f_glint, sigma2, n=INDEX, shadow=True):
    return f_iso + f_glint * rho_glint(a, b, phi, sigma2, n, shadow)


_rho_before = G._rho


def _rho(brdf):
    if isinstance(brdf, tuple) and brdf and brdf[0] == "cox_munk":
        return lambda a, b, c: rho_glint(a, b, c, *brdf[1:])
    if isinstance(brdf, tuple) and brdf and brdf[0] == "ocean":
        return lambda a, b, c: rho_ocean(a, b, c, *brdf[1:])
    return _rho_before(brdf)


G._rho = _rho


def up_weights(mu, N):
    """2 w_i mu_i on the upward nodes mu[N+1 ..], w their trapezoid weights"""
    return 2 * G.trapezoid_weights(mu[N + 1:]) * mu[N + 1:]


def black_sky_grid(mu, N, mu0, brdf, nphi=65):
    """sum_i 2 w_i mu_i rho_bar(mu_i, mu0) on the grid's upward nodes"""
    return float(up_weights(mu, N) @ G.beam_row(mu, N, mu0, brdf, nphi))


def black_sky_fine(mu0, brdf, ncos=4001, nphi=2049, chunk=250):
    """2 int_0^1 mu rho_bar(mu, mu0) dmu by the trapezoid rule on ncos cosines of [0, 1] and nphi azimuths of [0, pi]; the integrand
    at mu = 0 is taken at mu = 1e-12 (with shadowing on, mu rho -> 0 there)"""
    x = np.linspace(0.0, 1.0, ncos)
    f = np.concatenate([x[i:i + chunk] * G.rho_bar(brdf, np.maximum(x[i:i + chunk], 1e-12), mu0, nphi) for i in range(0, ncos, chunk)])
    return float(2 * G._trapz(f, x))
