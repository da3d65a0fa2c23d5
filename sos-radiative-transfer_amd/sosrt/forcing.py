"""Radiative forcing and critical single-scattering albedo of the aerosol layer: the reference's only
multi-column caller (SOS_Aer_critical_albedo.py:20-410), on top of the batched solve.

Two layers:

* drop-in: `SOS_Aer_radiative_forcing(...)` and `SOS_Aer_critical_albedo(...)` with the reference's positional
  signatures (crit:20, crit:394).  `baseline="coded"` reproduces the file as shipped: its recursion for the
  aerosol-free term passes the *same* optical-depth grid, mixing fractions and phase arrays (crit:388), so it
  recomputes the same column, the forcing is exactly 0.0 and the bisection stops at its first probe, 0.5
  (pinned by tests/golden/g7_*).  The default `baseline="no_aerosol"` is the defined fix: the baseline is the
  same column with the aerosol removed (its own grid tau_atm only, f_aer = 0).
* batched: `toa_net_flux`, `radiative_forcing`, `critical_albedo` over arrays of (tauStar_aer, alb_aer); every
  bisection step is one batched solve.

The radiance field never leaves the device: the solve keeps it resident and the flux epilogue
(csrc/epilogue.hip, crit:377-382) returns B numbers.
"""
from __future__ import annotations

import numpy as np

from .inputs import direction_grid, gas_row_weights, phase_function, slab_indices, tau_profile
from .main import (EARTH_RADIUS_KM, _beam_args, _brdf_args, _delta_m_aerosol, _delta_m_args, _gas_args, _raise_unconverged,
                   device_phase, get_solver, solve_brdf, solve_profile, solve_spherical)


def _net_flux_columns(tau, idx_up, idx_down, mu, mu0, grd_alb, alb_atm, alb_aer, dtau_atm, dtau_aer, tauStar_tot, P_atm, P_aer,
                      P0_atm, P0_aer, max_orders=256, device=0, beam="plane", earth_radius=EARTH_RADIUS_KM, z0=120,
                      surface="specular", brdf=None, gas=None):
    """TOA net flux (crit:382) of B columns on their grids tau [B, L]; per-column arrays or scalars otherwise.
    gas (the namespace of main._gas_args): the absorbing gas of main.SOS_Aer_batch -- tau and tauStar_tot are the scattering
    column's on the way in and get the gas here (main.solve_profile, the flux epilogue on the total tau).
    beam='spherical': the pseudo-spherical direct beam (main.solve_spherical) on the altitudes np.linspace(z0, 0, L), and the
    flux's beam terms on the same slant path (the beam epilogue).  surface='brdf' with `brdf`: the BRDF ground of
    main.SOS_Aer_batch (main.solve_brdf), grd_alb its per-column scale; the flux of the summed field."""
    spherical = _beam_args(beam, earth_radius)
    tau = np.atleast_2d(np.asarray(tau, dtype=np.float64))
    B, L = tau.shape
    N = len(mu) // 2
    ground = _brdf_args(surface, brdf, grd_alb, N, B, beam=beam)
    if ground:
        grd_alb = 0.0                                        # the series' solves run over a black ground
    s = get_solver(L, N, B, max_orders, device)
    if not s.same_grid(mu):
        s.set_grid(mu)
    if not s.same_phase(P_atm, P_aer):
        s.set_phase(P_atm, P_aer)
    if gas is not None:
        gas.tau0 = tau
        tau, gas.w = gas_row_weights(tau, gas.gas_tau)
        tauStar_tot = np.broadcast_to(np.asarray(tauStar_tot, dtype=np.float64), (B,)) + gas.gas_tau[:, -1]
    s.set_columns(np.full(B, idx_up), np.full(B, idx_down), mu0, grd_alb, alb_atm, alb_aer, dtau_atm, dtau_aer, tauStar_tot)
    P0a = np.ascontiguousarray(np.broadcast_to(np.asarray(P0_atm, dtype=np.float64), (B, 2 * N)))
    P0r = np.ascontiguousarray(np.broadcast_to(np.asarray(P0_aer, dtype=np.float64), (B, 2 * N)))
    if gas is not None:
        r, _, epi = solve_profile(s, tau, P0a, P0r, gas.w, np.broadcast_to(np.asarray(mu0, dtype=np.float64), (B,)),
                                  np.linspace(z0, 0, L) if spherical else None, earth_radius, device=device, fetch_field=False,
                                  want=("net_toa",))
    elif spherical:
        r, _, epi = solve_spherical(s, tau, P0a, P0r, np.linspace(z0, 0, L), earth_radius, device=device, fetch_field=False,
                                    want=("net_toa",))
    elif ground:
        r, _, epi = solve_brdf(s, tau, P0a, P0r, ground, mu0, device=device, fetch_field=False, want=("net_toa",))
    else:
        r = s.solve(tau, P0a, P0r, fetch_field=False)
    _raise_unconverged(r.status, N, max_orders)
    return epi["net_toa"] if spherical or ground or gas is not None else s.epilogue(want=("net_toa",))["net_toa"]


# ---------------------------------------------------------------------------------------------
# drop-in surface (crit:20, crit:394)
# ---------------------------------------------------------------------------------------------
def SOS_Aer_radiative_forcing(tauStar_aer, dtau_aer, tauStar_atm, dtau_atm, P_aer, P0_aer, alb_aer, P_atm, P0_atm, alb_atm,
                              grd_alb, F0, mu, mu0, nb_angles, tau, nb_layers, idx_up, idx_down, *, baseline="no_aerosol",
                              tauStar_tot=None, max_orders=256, device=0):
    """crit:20-389.  `tauStar_aer == 0` returns the net flux at the top of the atmosphere of the column described by
    the other arguments (crit:384-385); otherwise the forcing (crit:387-389).  `tauStar_tot` stands for the module
    global the reference's function reads (crit:39); default tauStar_atm + tauStar_aer.  `F0` must be pi/mu0
    (crit:469), as everywhere in the reference."""
    if baseline not in ("coded", "no_aerosol"):
        raise ValueError("baseline must be 'coded' or 'no_aerosol'")
    if abs(F0 - np.pi / mu0) > 1e-12 * F0:
        raise ValueError("F0 must be pi/mu0 (crit:469)")
    tot = tauStar_atm + tauStar_aer if tauStar_tot is None else tauStar_tot
    args = dict(P_atm=P_atm, P_aer=P_aer, P0_atm=P0_atm, P0_aer=P0_aer, max_orders=max_orders, device=device)
    f = float(_net_flux_columns(tau, idx_up, idx_down, mu, mu0, grd_alb, alb_atm, alb_aer, dtau_atm, dtau_aer, tot, **args)[0])
    if tauStar_aer == 0:
        return f
    if baseline == "coded":
        return f - f                                  # crit:388 solves the same column again: exactly 0.0
    tau0 = np.arange(0, nb_layers) * tauStar_atm / (nb_layers - 1)          # taup:21 with no aerosol
    f0 = float(_net_flux_columns(tau0, idx_up, idx_down, mu, mu0, grd_alb, alb_atm, alb_aer, dtau_atm, 0.0, tauStar_atm, **args)[0])
    return f - f0


def SOS_Aer_critical_albedo(tauStar_aer, dtau_aer, tauStar_atm, dtau_atm, P_aer, P0_aer, P_atm, P0_atm, alb_atm, grd_alb, F0, mu,
                            mu0, nb_angles, tau, nb_layers, idx_up, idx_down, *, baseline="no_aerosol", **kw):
    """crit:394-410: bisection on the aerosol single-scattering albedo until the bracket is narrower than 0.1 or
    |forcing| < 0.001."""
    alb_max, alb_min = 1, 0
    while (alb_max - alb_min) > 0.1:
        test = (alb_max + alb_min) / 2
        f = SOS_Aer_radiative_forcing(tauStar_aer, dtau_aer, tauStar_atm, dtau_atm, P_aer, P0_aer, test, P_atm, P0_atm, alb_atm,
                                      grd_alb, F0, mu, mu0, nb_angles, tau, nb_layers, idx_up, idx_down, baseline=baseline, **kw)
        if np.abs(f) < 0.001:
            return test
        if f > 0:
            alb_min = test
        else:
            alb_max = test
    return (alb_max + alb_min) / 2


# ---------------------------------------------------------------------------------------------
# batched over (tauStar_aer, alb_aer)
# ---------------------------------------------------------------------------------------------
def _solve_fluxes(mu0, tauStar_atm, tauStar_aer, grd_alb, alb_atm, alb_aer, geom, phases, max_orders, device, beam="plane",
                  earth_radius=EARTH_RADIUS_KM, surface="specular", brdf=None, gas=None):
    """TOA net flux (crit:382) of B columns; arrays of length B for tauStar_aer and alb_aer."""
    z0, z_up, z_down, L, N = geom
    P0_atm, P_atm, P0_aer, P_aer = phases
    iu, idn = slab_indices(z0, z_up, z_down, L)
    tau = np.stack([tau_profile(tauStar_atm, t, z0, z_up, z_down, L) for t in tauStar_aer])
    ta = np.asarray(tauStar_aer, dtype=np.float64)
    return _net_flux_columns(tau, iu, idn, direction_grid(N), mu0, grd_alb, alb_atm, alb_aer, tauStar_atm / L,
                             ta / (idn + 1 - iu), tauStar_atm + ta, P_atm, P_aer, P0_atm, P0_aer, max_orders, device, beam, earth_radius,
                             z0, surface, brdf, gas)


def toa_net_flux(mu0, tauStar_atm, tauStar_aer, grd_alb, alb_atm, alb_aer, *, z0=120, z_up=25, z_down=17, nb_layers=200,
                 nb_angles=128, atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7, phases=None,
                 max_orders=256, device=0, beam="plane", earth_radius=EARTH_RADIUS_KM, surface="specular", brdf=None, delta_m=None,
                 mie_aer=None, gas_tau=None):
    """Net flux at the top of the atmosphere, -F_down[0] - F_up[0] (crit:377-382), for arrays of
    (tauStar_aer, alb_aer).  beam='spherical' (with `earth_radius`, km): the direct beam on its slant path through spherical
    shells, in the solve and in the flux's beam terms (main.SOS_Aer_batch); `radiative_forcing` and `critical_albedo` pass
    both keywords on.  surface='brdf' with `brdf` ('lambertian', ('rpv', rho0, k, theta), ('ross_li', f_iso, f_vol, f_geo[,
    mu_floor]), ('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]]) or arrays (R, r0)): the BRDF ground of main.SOS_Aer_batch, grd_alb its scale; `radiative_forcing` and
    `critical_albedo` pass these on too.  `delta_m=Lambda` (2 .. 128; `mie_aer` as in main.SOS_Aer_batch): the aerosol
    delta-M-scaled -- its phase arrays from the truncated table, built on the device, and tauStar_aer and
    alb_aer scaled per column; the flux is the epilogue's on the scaled column, whose direct beam contains the forward-scattered
    light.  Not with `phases`, beam='spherical' or surface='brdf'.  `radiative_forcing` and `critical_albedo` pass it on: the
    bisection runs on the unscaled albedo.  `gas_tau` ([L] or [B, L]): the absorbing gas of main.SOS_Aer_batch, its cumulative
    absorption optical depth at the levels; with beam='spherical' on the slant path of the total tau; not with surface='brdf' or
    delta_m.  `radiative_forcing` passes it on: the baseline column keeps the gas."""
    gas = _gas_args(gas_tau, lambda: int(np.broadcast(np.atleast_1d(tauStar_aer), np.atleast_1d(alb_aer)).size), nb_layers,
                    surface=surface, delta_m=delta_m)
    dm = _delta_m_args(delta_m, aer_phase_fun, P_aer=None if phases is None else phases[3], surface=surface, beam=beam)
    _beam_args(beam, earth_radius)
    if surface not in ("specular", "brdf"):
        raise ValueError("surface must be 'specular' or 'brdf' (got %r)" % (surface,))
    _brdf_args(surface, brdf, grd_alb, nb_angles, int(np.broadcast(np.atleast_1d(tauStar_aer), np.atleast_1d(alb_aer)).size), beam=beam)
    ta, wa = np.broadcast_arrays(np.atleast_1d(np.asarray(tauStar_aer, dtype=float)), np.atleast_1d(np.asarray(alb_aer, dtype=float)))
    if dm is not None:
        mu = direction_grid(nb_angles)
        s = get_solver(int(nb_layers), int(nb_angles), ta.size, max_orders, device)
        if not s.same_grid(mu):
            s.set_grid(mu)
        P0a, Pa = device_phase(s, atm_phase_fun, [mu0], g_atm)
        phase, ta, wa = _delta_m_aerosol(s, dm, aer_phase_fun, g_aer, mie_aer, ta, wa, device)
        P0r, Pr = device_phase(s, phase[0], [mu0], phase[1], phase[2])
        phases = (P0a[0], Pa, P0r[0], Pr)
    if phases is None:
        mu = direction_grid(nb_angles)
        P0a, Pa = phase_function(atm_phase_fun, nb_angles, mu, mu0, g_atm)
        P0r, Pr = phase_function(aer_phase_fun, nb_angles, mu, mu0, g_aer)
        phases = (P0a, Pa, P0r, Pr)
    return _solve_fluxes(mu0, tauStar_atm, ta, grd_alb, alb_atm, wa, (z0, z_up, z_down, nb_layers, nb_angles), phases, max_orders, device,
                         beam, earth_radius, surface, brdf, gas)


def radiative_forcing(mu0, tauStar_atm, tauStar_aer, grd_alb, alb_atm, alb_aer, *, baseline="no_aerosol", **kw):
    """TOA net flux with the aerosol layer minus the baseline (crit:384-389): the same column without the aerosol
    ('no_aerosol', default) or, as the reference is coded, the same column again ('coded': identically zero)."""
    ta = np.atleast_1d(np.asarray(tauStar_aer, dtype=float))
    with_aer = toa_net_flux(mu0, tauStar_atm, ta, grd_alb, alb_atm, alb_aer, **kw)
    if baseline == "coded":
        return with_aer - with_aer
    if kw.get("gas_tau") is not None and np.ndim(kw["gas_tau"]) == 2:
        # every column its own gas: every column its own baseline
        return with_aer - toa_net_flux(mu0, tauStar_atm, np.zeros_like(with_aer), grd_alb, alb_atm, np.ones_like(with_aer), **kw)
    base = toa_net_flux(mu0, tauStar_atm, [0.0], grd_alb, alb_atm, [1.0], **kw)[0]
    return with_aer - base


def critical_albedo(mu0, tauStar_atm, tauStar_aer, grd_alb, alb_atm, *, width=0.1, tol=1e-3, baseline="no_aerosol", **kw):
    """Aerosol single-scattering albedo at which the forcing changes sign, by the bisection of crit:394-410
    (stop when the bracket is narrower than `width` or |forcing| < `tol`), for an array of tauStar_aer."""
    ta = np.atleast_1d(np.asarray(tauStar_aer, dtype=float))
    lo, hi = np.zeros_like(ta), np.ones_like(ta)
    result = np.full_like(ta, np.nan)
    base = None if baseline == "coded" else toa_net_flux(mu0, tauStar_atm, [0.0], grd_alb, alb_atm, [1.0], **kw)[0]
    live = np.ones(len(ta), dtype=bool)
    while live.any() and np.any((hi - lo)[live] > width):
        test = (hi + lo) / 2
        f = np.zeros_like(ta)
        fl = toa_net_flux(mu0, tauStar_atm, ta[live], grd_alb, alb_atm, test[live], **kw)
        f[live] = fl - (fl if base is None else base)
        done = live & (np.abs(f) < tol)
        result[done] = test[done]
        live &= ~done
        up = live & (f > 0)
        lo[up] = test[up]
        hi[live & ~up] = test[live & ~up]
        narrow = live & ((hi - lo) <= width)
        result[narrow] = ((hi + lo) / 2)[narrow]
        live &= ~narrow
    result[np.isnan(result)] = ((hi + lo) / 2)[np.isnan(result)]
    return result
