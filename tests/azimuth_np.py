"""NumPy restatement of the Fourier modes in azimuth (include/sosrt.h), for the tests of the azimuth-resolved
solve.  Mode m of a pair of directions, with the reference's scattering cosine c(a, b, phi) = -(mu_a mu_b + s_a s_b cos phi):

    R^m(a, b) = trapz_q [p(c(a, b, phi_q)) + (-1)^m p(c(a, b, phi_q + pi))] cos(m phi_q),   phi_q = linspace(0, pi, nphi)

normalised by the m = 0 ring of the same nphi.  Mode 0 at nphi = 25 is `inputs.phase_function` as written there."""
import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def ring_modes(fn, mu_a, mu_b, ms, nphi, dtype=np.float64):
    """[len(ms), len(mu_a), len(mu_b)]; dtype: the arithmetic (the float64 cosines and azimuth nodes, taken into it exactly)"""
    phi = np.linspace(0, np.pi, nphi).astype(dtype)
    mu_a, mu_b = np.asarray(mu_a).astype(dtype), np.asarray(mu_b).astype(dtype)
    cc = mu_a[:, None] * mu_b[None, :]
    ss = np.sqrt(1 - mu_b * mu_b)[None, :] * np.sqrt(1 - mu_a * mu_a)[:, None]
    cp = np.cos(0 - phi)
    pos = fn(-(cc[..., None] + ss[..., None] * cp))
    neg = fn(-(cc[..., None] - ss[..., None] * cp))
    return np.stack([_trapz(pos + neg if m == 0 else (pos + (-1) ** m * neg) * np.cos(m * phi), phi, axis=-1) for m in ms])


def phase_modes(fn, mu, ms, nphi):
    """P^m [len(ms), 2N, 2N]: R^m / (2 pi) * 4 / Z_n, Z_n = trapz_mu(R^0(., n) / (2 pi)) of the same nphi."""
    R = ring_modes(fn, mu, mu, [0] + list(ms), nphi) / (2 * np.pi)
    Z = _trapz(R[0], mu, axis=0)[None, :]
    return np.stack([4 * R[1 + i] / Z for i in range(len(ms))])


def solve_modes(fn, mu, ms, nphi):
    """The matrices a solve of mode m takes, (-1)^m P^m [len(ms), 2N, 2N]: the source function pairs P[a][flip b] with
    I[b] (the reference's fold), and with the cosine above that pair is the physical scattering cosine at phi + pi, whose
    mode m is (-1)^m times the one at phi.  P0^m has no fold and no factor."""
    return np.stack([(-1) ** m * P for m, P in zip(ms, phase_modes(fn, mu, ms, nphi))])


def phase_p0_modes(fn, mu, mu0, ms, nphi):
    """P0^m [len(ms), 2N] for one mu0: R^m / (4 pi) * 2 / Z0, Z0 = trapz_mu(R^0(., mu0) / (4 pi))."""
    R = ring_modes(fn, mu, np.array([float(mu0)]), [0] + list(ms), nphi)[:, :, 0] / (4 * np.pi)
    Z = _trapz(R[0], mu)
    return np.stack([R[1 + i] / Z * 2 for i in range(len(ms))])


def p0_direct(fn, mu, mu0, phi, nphi=25):
    """p(c(mu, mu0, phi)) / Z0: the phi-resolved single-scattering phase function the modes of P0 sum to, [2N]."""
    R0 = ring_modes(fn, mu, np.array([float(mu0)]), [0], nphi)[0, :, 0] / (4 * np.pi)
    Z = _trapz(R0, mu)
    c = -(mu * mu0 + np.sqrt(1 - mu * mu) * np.sqrt(1 - mu0 * mu0) * np.cos(phi))
    return fn(c) / Z
