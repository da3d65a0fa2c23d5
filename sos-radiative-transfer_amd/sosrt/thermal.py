"""Thermal emission: the Planck function, and the outgoing longwave flux and longwave forcing of the aerosol
layer on top of the batched thermal solve (`main.solve_thermal`).

The radiance field never leaves the device: the solve keeps it there and the emission epilogue (csrc/emission.hip: the flux
epilogue without beam terms) returns B numbers.
"""
from __future__ import annotations

import numpy as np

from .main import _batch_width, _gas_args, _prepare_batch, _raise_unconverged, _thermal_args, solve_profile, solve_thermal

# CODATA 2018 (exact since the 2019 redefinition of the SI)
PLANCK_H = 6.62607015e-34          # J s
LIGHT_C = 299792458.0              # m / s
BOLTZMANN_K = 1.380649e-23         # J / K
STEFAN_BOLTZMANN = 2 * np.pi ** 5 * BOLTZMANN_K ** 4 / (15 * PLANCK_H ** 3 * LIGHT_C ** 2)    # 5.670374419e-8 W m-2 K-4


def planck_radiance(T_kelvin, wavelength_um):
    """Planck's spectral radiance B_lambda(T) = 2 h c^2 / lambda^5 / (exp(h c / (lambda k T)) - 1) in W m-2 sr-1 um-1 (host
    NumPy; the arguments broadcast).  pi times its integral over the wavelength is sigma T^4."""
    T = np.asarray(T_kelvin, dtype=np.float64)
    lam = np.asarray(wavelength_um, dtype=np.float64) * 1e-6
    if np.any(T <= 0) or np.any(lam <= 0):
        raise ValueError("planck_radiance needs T > 0 K and wavelength > 0 um")
    with np.errstate(over="ignore"):
        x = PLANCK_H * LIGHT_C / (lam * BOLTZMANN_K * T)
        return 2 * PLANCK_H * LIGHT_C ** 2 / lam ** 5 / np.expm1(x) * 1e-6


def thermal_toa_flux(tauStar_aer, grd_alb, planck, planck_surface, surface_emissivity=None, *, tauStar_atm=0.124, alb_atm=1.0,
                     alb_aer=1.0, z0=120, z_up=25, z_down=17, nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", g_atm=0.0,
                     aer_phase_fun="hg", g_aer=0.7, mie_atm=None, mie_aer=None, surface="specular", tol=1e-4, max_orders=256,
                     device=0, gas_tau=None):
    """Outgoing flux at the top of the atmosphere of B thermal columns, [B], in the unit of `planck` (times a steradian): the
    upward trapezoid flux of the thermal field of `SOS_Aer_batch(source='thermal')`, from the emission epilogue.  The
    per-column arguments (tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer) broadcast; planck [L] or [B, L],
    planck_surface and surface_emissivity scalars or [B].  `gas_tau` ([L] or [B, L]): the absorbing -- and so emitting -- gas of
    `SOS_Aer_batch`, its cumulative absorption optical depth at the levels; `thermal_forcing` passes it on."""
    B = _batch_width(tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer)
    gas = _gas_args(gas_tau, B, nb_layers)
    thermal = _thermal_args("thermal", planck, planck_surface, surface_emissivity, B, nb_layers)
    # (the sun does not enter: any mu0 serves the phase functions' P0 rows, which the thermal solve does not read)
    s, tau, _, _, _, _, _, N = _prepare_batch(np.full(B, 0.5), tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, z0, z_up, z_down,
                                              nb_layers, nb_angles, atm_phase_fun, g_atm, aer_phase_fun, g_aer, mie_atm, mie_aer,
                                              None, None, None, None, surface, max_orders, device, gas=gas)
    if gas is not None:
        r, _, epi = solve_profile(s, tau, None, None, gas.w, thermal=thermal, tol=tol, want=("flux_up",), device=device, fetch_field=False)
    else:
        r, epi = solve_thermal(s, tau, *thermal, tol=tol, want=("flux_up",), device=device, fetch_field=False)
    _raise_unconverged(r.status, N, max_orders)
    return epi["flux_up"][:, 0].copy()


def thermal_forcing(tauStar_aer, grd_alb, planck, planck_surface, surface_emissivity=None, **kw):
    """Longwave forcing of the aerosol layer, [B]: the outgoing flux of the same columns with tauStar_aer = 0 minus the
    outgoing flux with the layer (`thermal_toa_flux`, its keywords) -- positive where the layer keeps radiation in, the sign of
    `forcing.radiative_forcing`, so the two add up to the layer's net forcing."""
    with_layer = thermal_toa_flux(tauStar_aer, grd_alb, planck, planck_surface, surface_emissivity, **kw)
    without = thermal_toa_flux(np.zeros_like(np.asarray(tauStar_aer, dtype=np.float64)), grd_alb, planck, planck_surface,
                               surface_emissivity, **kw)
    return without - with_layer
