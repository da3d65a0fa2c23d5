"""NumPy model of delta-M: the two kernels of csrc/deltam.hip with the same rule -- 4-node Gauss-Legendre on
every table interval, the upward recurrence P_{l+1} = a_l x P_l - b_l P_{l-1}, sums in ascending order -- and the driver chain:
the truncated table through the oracle's azimuth averages into an oracle column with the scaled optics."""
import numpy as np

import sos_oracle as O

GLX = np.array([-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526])
GLW = np.array([0.34785484513745385, 0.6521451548625461, 0.6521451548625461, 0.34785484513745385])


def abscissa(ntab, tab_mu=None):
    return np.linspace(-1, 1, ntab) if tab_mu is None else np.asarray(tab_mu, dtype=np.float64)


def _ascending_sum(t):
    """Sum of a vector, one term after the other (np.sum adds pairwise)."""
    return np.cumsum(t)[-1]


def moments(tab_mu, tab_p, lmax, nodes=4):
    """(chi [lmax + 1], norm) of the piecewise-linear interpolant of (tab_mu, tab_p); tab_mu None: the uniform abscissa.
    `nodes` other than 4: numpy's Gauss-Legendre rule of that size, to measure the rule against."""
    p = np.asarray(tab_p, dtype=np.float64)
    x = abscissa(len(p), tab_mu)
    gx, gw = (GLX, GLW) if nodes == 4 else np.polynomial.legendre.leggauss(nodes)
    x0, x1, p0, p1 = x[:-1], x[1:], p[:-1], p[1:]
    mid, half = 0.5 * (x0 + x1), 0.5 * (x1 - x0)
    xk = mid[:, None] + half[:, None] * gx[None, :]
    q = half[:, None] * gw[None, :] * (p0[:, None] + (xk - x0[:, None]) / (x1 - x0)[:, None] * (p1 - p0)[:, None])
    P, Pm = np.ones_like(xk), np.zeros_like(xk)
    sums = np.zeros(lmax + 1)
    for l in range(lmax + 1):
        t = q * P
        per_interval = t[:, 0]
        for k in range(1, t.shape[1]):
            per_interval = per_interval + t[:, k]
        sums[l] = _ascending_sum(per_interval)
        a, b = (2.0 * l + 1.0) / (l + 1.0), l / (l + 1.0)
        P, Pm = a * xk * P - b * Pm, P
    return sums / sums[0], 0.5 * sums[0]


def coefficients(chi, order):
    """((2l + 1) c_l for l < order, f): c_l = (chi_l - f) / (1 - f), f = chi[order]."""
    chi = np.asarray(chi, dtype=np.float64)
    f = chi[order]
    l = np.arange(order)
    return (2.0 * l + 1.0) * ((chi[:order] - f) / (1.0 - f)), f


def delta_m_table(chi, order, x):
    """(sum_{l < order} (2l + 1) c_l P_l(x), f), l ascending."""
    coef, f = coefficients(chi, order)
    x = np.asarray(x, dtype=np.float64)
    acc, P, Pm = np.zeros_like(x), np.ones_like(x), np.zeros_like(x)
    for l in range(order):
        acc = acc + coef[l] * P
        a, b = (2.0 * l + 1.0) / (l + 1.0), l / (l + 1.0)
        P, Pm = a * x * P - b * Pm, P
    return acc, f


def table_bound(chi, order):
    """sum_{l < order} (2l + 1) |c_l|: the size of the series' terms, what a tolerance on the table scales with."""
    return float(np.sum(np.abs(coefficients(chi, order)[0])))


def scale_optics(tau, w, f):
    k = 1 - w * f
    return tau * k, (1 - f) * w / k


def hg(g):
    return lambda c: (1 - g * g) / ((1 + g * g - 2 * g * c) ** 1.5)


def truncated(tab_mu, tab_p, order):
    """(abscissa, truncated table, f) of a table by the model."""
    x = abscissa(len(tab_p), tab_mu)
    chi, _ = moments(tab_mu, tab_p, order)
    t, f = delta_m_table(chi, order, x)
    return x, t, f


# the issue's column: Rayleigh atmosphere, one aerosol slab
COLUMN = dict(z0=120, z_up=25, z_down=17, tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.99, grd_alb=0.1)


def oracle_column(mu0, L, N, tauStar_aer, aer_table, f=0.0, **over):
    """The oracle column of COLUMN with the aerosol `aer_table` = (abscissa, values) and the optics scaled by f."""
    p = dict(COLUMN, **over)
    mu = O.make_mu(N)
    P0r, Pr = O.phase_rayleigh(N, mu, mu0)
    P0a, Pa = O.phase_table(N, mu, mu0, *aer_table)
    t, w = scale_optics(tauStar_aer, p["alb_aer"], f)
    return O.make_column(mu0, p["z0"], p["z_up"], p["z_down"], L, p["tauStar_atm"], t, p["grd_alb"], p["alb_atm"], w, N, P0r, Pr, P0a, Pa)


def solve(mu0, L, N, tauStar_aer, tab_mu, tab_p, order=None, max_orders=256, **over):
    """The oracle's solve of the column: raw table (order None) or delta-M at `order`.  Returns (Solution, f, column)."""
    if order is None:
        table, f = (abscissa(len(tab_p), tab_mu), np.asarray(tab_p, dtype=np.float64)), 0.0
    else:
        x, t, f = truncated(tab_mu, tab_p, order)
        table = (x, t)
    c = oracle_column(mu0, L, N, tauStar_aer, table, f, **over)
    return O.solve_column(c, literal=False, max_orders=max_orders), f, c


def toa_up(sol, c):
    """Upward flux at the top of the atmosphere (crit:381)."""
    return O.fluxes(sol.I, c.mu, c.tau, c.N, c.mu0, c.grd_alb)[1][0]
