"""Wind-speed laws for the ocean ground brdf=('cox_munk', ...) of `main.SOS_Aer_batch`.  U is the wind speed
in m/s at 10 m, a number or an array.

The usual composition of an open-ocean pixel -- foam of reflectance 0.22 over the whitecap fraction W, the water-leaving
reflectance rho_water under it, the glint on what the foam leaves free:

    W = whitecap_fraction(U)
    brdf = ("cox_munk", U, 1.34, W * 0.22 + rho_water, 1 - W)

No data ships with this module: rho_water and the refractive index are the caller's."""
import numpy as np


def slope_variance(U):
    """sigma^2 = 0.003 + 0.00512 U: the variance of the isotropic Gaussian slope distribution (Cox and Munk 1954)"""
    return 0.003 + 0.00512 * np.asarray(U, dtype=np.float64)


def whitecap_fraction(U):
    """W = 2.95e-6 U^3.52: the fraction of the surface covered by whitecaps (Monahan and O'Muircheartaigh 1980)"""
    return 2.95e-6 * np.asarray(U, dtype=np.float64) ** 3.52
