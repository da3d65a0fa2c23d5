"""Column-level drivers: the call surface of SOS_Aer_main_specular.py / SOS_Aer_main_lambertian.py.

`SOS_Aer(**overrides)` takes the reference's local names as keywords (spec:23-96); called
with no arguments it uses the literals the reference ships.  Unlike the reference (which
returns None and plots) it returns the radiance fields.  `SOS_Aer_batch` solves many
independent columns that share (nb_layers, nb_angles, phase matrices) in one launch sequence.
"""
from __future__ import annotations

from contextlib import contextmanager, nullcontext
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _lib
from .inputs import direction_grid, gas_row_weights, slab_indices, tau_profile
from .ocean import slope_variance
from .solver import DevicePhaseSets, Solver

# the literals of SOS_Aer_main_specular.py:23-96
DEFAULTS = dict(
    mu0=0.5, z0=120, z_up=25, z_down=17, nb_layers=800, tauStar_atm=0.104, tauStar_aer=0.120,
    grd_alb=1, alb_atm=1.0, alb_aer=1.0, nb_angles=501,
    atm_phase_fun="rayleigh", g_atm=0.5, r_atm=0, lambda0_atm=0, indx_atm=0, N0_atm=None, r_m_atm=None, sig_atm=None,
    aer_phase_fun="eva", g_aer=0.5, r_aer=0, lambda0_aer=0.550, indx_aer=1.44 + 0.0j, N0_aer=501187, r_m_aer=0.506,
    sig_aer=1.2,
)


@dataclass
class ColumnResult:
    I: np.ndarray            # [L, 2N] total radiance (spec:303,456)
    I_saved: np.ndarray      # [n, L, 2N] per-order fields (spec:304-305,458)
    n: int                   # final order (spec:307-310)
    tau: np.ndarray
    mu: np.ndarray
    idx_up: int
    idx_down: int
    status: int
    beam_slant: Optional[np.ndarray] = None   # [L] (beam='spherical'): slant optical depth of the direct beam at every level
    bounces: Optional[int] = None             # (surface='brdf'): ground reflections summed until the series' term fell below tol
    bounce_ratio: Optional[float] = None      # ... and the last term's share of the sum
    black_sky_albedo: Optional[float] = None  # (brdf=('ross_li', ...) or ('cox_munk', ...)): the ground's directional-hemispherical reflectance at mu0
    white_sky_albedo: Optional[float] = None  # ... and its bihemispherical reflectance, both on the grid's trapezoid
    delta_m_f: Optional[float] = None           # (delta_m=...): the truncated fraction f = chi_Lambda of the aerosol's scattering
    tauStar_aer_scaled: Optional[float] = None  # ... the aerosol optical depth the column was solved with
    alb_aer_scaled: Optional[float] = None      # ... and its single-scattering albedo
    gas_tau: Optional[np.ndarray] = None        # [L] (gas_tau=...): the gas absorption optical depth the column was solved with
    row_weight: Optional[np.ndarray] = None     # [L] ... and the weight on the source function of every row


@dataclass
class BatchResult:
    I: np.ndarray            # [B, L, 2N]
    n: np.ndarray            # [B]
    status: np.ndarray       # [B]
    tau: np.ndarray          # [B, L]
    mu: np.ndarray
    idx_up: int
    idx_down: int
    I_saved: Optional[np.ndarray] = None
    I_azimuth: Optional[np.ndarray] = None   # [B, nlev, 2N, len(azimuths)] (azimuths=...): radiance at the requested levels
    mode_status: Optional[np.ndarray] = None  # [M + 1, B] status of the solve of every Fourier mode (row 0 is `status`)
    view_mu_signed: Optional[np.ndarray] = None    # [2V] (view_mu=...): the signed view lanes (-view_mu, +view_mu)
    I_view: Optional[np.ndarray] = None            # [B, nlev, 2V] radiance at the view lanes = I_view_first + I_view_scattered
    I_view_first: Optional[np.ndarray] = None      # [B, nlev, 2V] its closed-form first order
    I_view_scattered: Optional[np.ndarray] = None  # [B, nlev, 2V] the transport of the field's source (orders n >= 2)
    I_view_azimuth: Optional[np.ndarray] = None            # [B, nlev, 2V, len(view_azimuths)] (view_azimuths=...) = _first + _scattered
    I_view_azimuth_first: Optional[np.ndarray] = None      # its first order: exact at (lane, azimuth), or the sum of the modes'
    I_view_azimuth_scattered: Optional[np.ndarray] = None  # the synthesis of the per-mode transports of the fields' sources
    view_mode_status: Optional[np.ndarray] = None          # [M + 1, B] status of the solve of every Fourier mode (row 0 is `status`)
    beam_slant: Optional[np.ndarray] = None   # [B, L] (beam='spherical'): slant optical depth of the direct beam at every level
    bounces: Optional[np.ndarray] = None      # [B] (surface='brdf'): the ground reflection at which the column's term fell below tol
    bounce_ratio: Optional[np.ndarray] = None  # [B] ... and the last term's share of the sum on the TOA-up and surface-down lanes
    bounce_orders: Optional[np.ndarray] = None  # [K, B] (surface='brdf'): the orders the solve of every ground reflection ran
    I_view_ground: Optional[np.ndarray] = None          # [B, nlev, 2V] (brdf_view=True): the ground's unscattered radiance at the view lanes, a term of I_view
    I_view_azimuth_ground: Optional[np.ndarray] = None  # [B, nlev, 2V, len(view_azimuths)] the same at (lane, azimuth), a term of I_view_azimuth
    black_sky_albedo: Optional[np.ndarray] = None  # [B] (brdf=('ross_li', ...) or ('cox_munk', ...)): the ground's directional-hemispherical reflectance at mu0
    white_sky_albedo: Optional[np.ndarray] = None  # [B] ... and its bihemispherical reflectance, both on the grid's trapezoid
    delta_m_f: Optional[float] = None                  # (delta_m=...): the truncated fraction f = chi_Lambda of the aerosol's scattering
    tauStar_aer_scaled: Optional[np.ndarray] = None    # [B] ... the aerosol optical depth the columns were solved with
    alb_aer_scaled: Optional[np.ndarray] = None        # [B] ... and its single-scattering albedo
    gas_tau: Optional[np.ndarray] = None               # [B, L] (gas_tau=...): the gas absorption optical depth of every column (tau includes it)
    row_weight: Optional[np.ndarray] = None            # [B, L] ... and the weight on the source function of every row


_solvers = {}


def get_solver(nb_layers, nb_angles, batch, max_orders, device=0) -> Solver:
    import os
    key = (nb_layers, nb_angles, device, os.environ.get("SOSRT_TRANSPORT", ""))
    s = _solvers.get(key)
    if s is None or s.max_batch < batch or s.max_orders < max_orders:
        if s is not None:
            s.close()
        s = _solvers[key] = Solver(nb_layers, nb_angles, max_batch=batch, max_orders=max_orders, device=device)
    if s.order_budget != max_orders:                 # (a cached handle made for a larger budget serves this call with its own)
        s.set_order_budget(max_orders)
    return s


def _raise_status(status, nb_angles):
    st = np.atleast_1d(status)
    if np.any(st == _lib.COL_INDEXERROR):
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (2 * nb_angles, 2 * nb_angles))
    if np.any(st == _lib.COL_INTERNAL):
        raise RuntimeError("sosrt: internal error in the transport kernel (SOSRT_COL_INTERNAL)")


@contextmanager
def _on_torch_stream(s: Solver, device):
    """The cached handle `s` on torch's current stream of cuda:`device`, that device made current: yields the torch device.  On
    exit the stream is drained and the handle goes back to its own stream -- also when the body raises, and when the drain
    itself raises (that error propagates).  What a driver has to put back on the handle besides comes after the scope, in a
    `finally` of its own."""
    import torch
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        s.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        try:
            yield dev
        finally:
            # the solver is cached and goes back to its own stream: drain this one first, so that the handle's internal
            # buffers are not reused under the last launches (the order loop has already waited for all but the last two)
            try:
                s.synchronize()
            finally:
                s.set_stream(None)


def _phase_kind(s: Solver, name, g=0.0, mie=None):
    """(kind, g) of a named phase function as the device builders of handle `s` take it; a Mie-derived one ('mie' / 'eva' /
    'wildfire' / 'fwc') becomes the handle's table on the scattering cosine.  `device=True` in the `mie` dict: the table from
    the Mie kernels of this handle."""
    from .inputs import _scalar_phase
    kw = dict(mie or {})
    if kw.get("device") is True:
        kw["device"] = s
    kind, tab = ("iso", None) if name == "iso" else _scalar_phase(name, g, **kw)[1]
    if tab is not None:
        s.set_phase_table(*tab)
    return kind, g


def _raise_unconverged(status, nb_angles, max_orders):
    """The flux drivers (forcing, thermal, bands) sum or difference their columns, so any non-zero status raises: IndexError as
    the reference does where its mu -> 0 search leaves the grid (spec:404), RuntimeError for anything else."""
    if np.any(status == _lib.COL_INDEXERROR):
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (2 * nb_angles, 2 * nb_angles))
    if np.any(status != 0):
        raise RuntimeError("columns did not converge within %d orders: status %s" % (max_orders, status))


def device_phase(s: Solver, name, mu0, g=0.0, mie=None, matrix=True):
    """(P0 rows [len(mu0), 2N], P [2N, 2N] or None) of a named phase function, azimuth-averaged by the HIP kernels of solver
    `s` (phase:79-133 and its siblings; the grid must be set).  `mie` = dict(r=, lambda0=, indx=, r_m=, sig=) for 'mie' /
    'eva' / 'wildfire', whose phase function goes to the device as a table on the scattering cosine; `device=True` in that dict
    builds the table with the device's Mie kernels instead of the host series."""
    kind, g = _phase_kind(s, name, g, mie)
    P0 = s.phase_p0(kind, mu0, g)
    return P0, (s.phase_matrix(kind, g) if matrix else None)


EARTH_RADIUS_KM = 6371.0


def _beam_args(beam, earth_radius, azimuths=None, view_mu=None, view_azimuths=None, mode_batch=False, mode_chunk=None,
               first_order="coded", devices=None, beam_stages=False):
    """Checks of the `beam` keyword, made before any handle exists: True for the pseudo-spherical beam.  Without
    `beam_stages=True` the stages that compute first orders of their own are refused: those are plane closed forms.  With it
     `azimuths`, `view_mu` and `view_azimuths` take their first orders on the slant path; the mode batch stays
    refused."""
    if not isinstance(beam, str) or beam not in ("plane", "spherical"):
        raise ValueError("beam must be 'plane' or 'spherical' (got %r)" % (beam,))
    if not isinstance(beam_stages, (bool, np.bool_)):
        raise ValueError("beam_stages must be True or False (got %r)" % (beam_stages,))
    if beam == "plane":
        if beam_stages:
            raise ValueError("beam_stages=True belongs to beam='spherical': the plane beam's stages need no keyword")
        return False
    try:
        er = float(earth_radius)
    except (TypeError, ValueError):
        raise ValueError("earth_radius must be a number of kilometres (got %r)" % (earth_radius,)) from None
    if not (np.isfinite(er) and er > 0):
        raise ValueError("earth_radius must be finite and > 0 km (got %r)" % (earth_radius,))
    if beam_stages and (mode_batch or mode_chunk is not None):
        raise ValueError("beam='spherical' is not available with mode_batch / mode_chunk, also with beam_stages=True: the batched "
                         "modes take their first orders from the order loop's plane closed form")
    if not beam_stages and (azimuths is not None or mode_batch or mode_chunk is not None):
        raise ValueError("beam='spherical' is not available with azimuths / mode_batch: the first order of a Fourier mode m >= 1 is "
                         "the plane closed form")
    if not beam_stages and (view_mu is not None or view_azimuths is not None):
        raise ValueError("beam='spherical' is not available with view_mu / view_azimuths: the first order at a view cosine is the "
                         "plane closed form")
    if first_order != "coded":
        raise ValueError("beam='spherical' is not available with first_order='readme': the isotropically reflected beam of the "
                         "README's first order has no slant form")
    if devices is not None and len(devices) > 1:
        raise ValueError("beam='spherical' is not available with devices=[...]: solve each shard with SOS_Aer_batch(device=...)")
    return True


def _delta_m_args(delta_m, aer_phase_fun="hg", azimuths=None, aer_set=None, P_aer=None, P0_aer=None, mode_batch=False,
                  mode_chunk=None, surface="specular", beam="plane", source="solar", first_order="coded", devices=None):
    """Checks of the `delta_m` keyword, made before any handle exists: None, or a namespace with the order Lambda that
    `_prepare_batch` fills (f, the truncated table, the scaled optics).  What has no delta-M form yet is refused."""
    if delta_m is None:
        return None
    from .deltam import check_order
    order = check_order(delta_m)
    no = lambda what, why: ValueError("delta_m is not available with %s: %s" % (what, why))
    if aer_set is not None or isinstance(aer_phase_fun, (list, tuple)):
        raise no("aer_set / a list of aerosols", "one aerosol is truncated per call")
    if P_aer is not None or P0_aer is not None:
        raise no("P_aer / P0_aer arrays", "the moments are taken of a named phase function")
    if aer_phase_fun in ("iso", "rayleigh"):
        raise ValueError("delta_m is for a forward-peaked aerosol: %r has no peak to truncate" % (aer_phase_fun,))
    if azimuths is not None:
        raise no("azimuths", "the grid's synthesis has no exact first order; view_mu with view_azimuths has the TMS one")
    if mode_batch or mode_chunk is not None:
        raise no("mode_batch / mode_chunk", "they belong to azimuths")
    if surface == "brdf":
        raise no("surface='brdf'", "the ground's series reflects the unscaled beam")
    if beam != "plane":
        raise no("beam='spherical'", "the slant path is not scaled")
    if source != "solar":
        raise no("source='thermal'", "emission has no beam to move the forward peak into")
    if first_order != "coded":
        raise no("first_order='readme'", "the README's first order is not scaled")
    if devices is not None and len(devices) > 1:
        raise no("devices=[...]", "solve each shard with SOS_Aer_batch(device=...)")
    return SimpleNamespace(order=order)


def _delta_m_aerosol(s: Solver, dm, aer_phase_fun, g_aer, mie_aer, tauStar_aer, alb_aer, device):
    """Delta-M of the aerosol on handle `s` (whose grid is set), into the namespace `dm` of `_delta_m_args`: f, the exact
    function as `_phase_kind` takes it, the truncated one as the named table ('table', 0, dict(table=...)) every later builder
    of the call resolves, and the scaled optics.  Returns (the truncated function's (name, g, mie), tauStar_aer', alb_aer')."""
    from .deltam import delta_m, scale_optics
    with _on_torch_stream(s, device):
        dm.f, _, keep = delta_m(s, aer_phase_fun, dm.order, g_aer, mie_aer)
        table = (keep["tab_mu"].cpu().numpy(), keep["truncated"].cpu().numpy())
        exact = None if keep["exact"] is None else keep["exact"].cpu().numpy()
    # (the exact function with mean 1 over [-1, 1], as the truncated one has: HG is, a table is divided by its norm)
    dm.exact = (aer_phase_fun, g_aer, mie_aer) if exact is None else ("table", 0.0, dict(table=(table[0], exact)))
    dm.phase = ("table", 0.0, dict(table=table))
    dm.tauStar_aer, dm.alb_aer = scale_optics(tauStar_aer, alb_aer, dm.f)
    return dm.phase, dm.tauStar_aer, dm.alb_aer


def _solve_resident(s: Solver, tau, P0a, P0r, seed, epilogue, tol=1e-4, save_orders=False, device=0, fetch_field=True, want=(),
                    z_profile=None, keep_device=False, post=None):
    """A solve of handle `s` (grid, phase matrices and columns set) that stays on the device, on torch's current stream: the
    uploads, `seed(up, dev, d_tau, B, p0a, p0r)` -> (d_I1 [B, L, 2N] the field the order loop starts from, dict of further
    tensors to return) or None for the handle's own first order, `solve_device` (with save_orders twice: the first pass gives
    n, the second stores exactly max(n) orders per column, as Solver.solve), and for the names `want` of `Solver.epilogue`
    (`z_profile` for the heating rate) `epilogue(d_tau, d_I, d_z, the seed's tensors, the five output addresses, B)`.  `P0a`, `P0r` may be None
    (address 0).  `post(up, dev, d_tau, d_I, d_n, d_st, B, p0a, p0r)` -> dict of further tensors runs between the solve and the
    epilogue and may add to the field in place (the BRDF ground's bounce loop).  Returns (SolveResult, the seed's tensors on the host, dict of the wanted epilogue arrays); keep_device=True:
    the torch tensors {"I", "n", "status", "tau"} and the seed's instead, left on the device.  The handle goes back to its own
    stream and to its default per-order storage, also on error."""
    import torch
    from .solver import SolveResult
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    B, L = tau.shape
    D = s.D
    try:
        with _on_torch_stream(s, device) as dev:
            def up(a):
                # (a host copy only where torch could not take the array as it is: broadcast inputs are read-only)
                a = np.ascontiguousarray(a, dtype=np.float64)
                return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
            d_tau, d_P0a, d_P0r = up(tau), None if P0a is None else up(P0a), None if P0r is None else up(P0r)
            p0a, p0r = 0 if d_P0a is None else d_P0a.data_ptr(), 0 if d_P0r is None else d_P0r.data_ptr()
            d_I1, extra = (None, {}) if seed is None else seed(up, dev, d_tau, B, p0a, p0r)
            d_I = torch.empty((B, L, D), dtype=torch.float64, device=dev)
            d_n = torch.zeros(B, dtype=torch.int32, device=dev)
            d_st = torch.zeros(B, dtype=torch.int32, device=dev)
            solve = lambda d_sv: s.solve_device(d_tau.data_ptr(), p0a, p0r, d_I.data_ptr(), tol=tol,
                                                d_I1=0 if d_I1 is None else d_I1.data_ptr(), d_I_saved=0 if d_sv is None else d_sv.data_ptr(),
                                                d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            solve(None)
            d_sv = None
            if save_orders:
                s.synchronize()
                slots = int(max(1, d_n.max().item()))
                s.set_saved_orders(slots)
                d_sv = torch.zeros((B, slots, L, D), dtype=torch.float64, device=dev)
                solve(d_sv)
            if post is not None:
                extra = dict(extra, **post(up, dev, d_tau, d_I, d_n, d_st, B, p0a, p0r))
            epi = {}
            want = [k for k in ("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")
                    if k in set(want) and not (k == "heating_rate" and z_profile is None)]
            if want:
                d_zp = None if z_profile is None else up(z_profile)
                d_out = {k: torch.empty((B,) if k == "net_toa" else (B, L), dtype=torch.float64, device=dev) for k in want}
                ptr = lambda k: d_out[k].data_ptr() if k in d_out else 0
                epilogue(d_tau.data_ptr(), d_I.data_ptr(), 0 if d_zp is None else d_zp.data_ptr(), extra,
                         (ptr("flux_down"), ptr("flux_up"), ptr("diffusivity"), ptr("heating_rate"), ptr("net_toa")), B)
                s.synchronize()
                epi = {k: v.cpu().numpy() for k, v in d_out.items()}
            s.synchronize()
            if keep_device:
                return dict({"I": d_I, "n": d_n, "status": d_st, "tau": d_tau}, **extra)
            r = SolveResult(I=d_I.cpu().numpy() if fetch_field else None, n=d_n.cpu().numpy(), status=d_st.cpu().numpy(),
                            I_saved=None if d_sv is None else d_sv.cpu().numpy())
            return r, {k: v.cpu().numpy() for k, v in extra.items()}, epi
    finally:
        if save_orders:
            s.set_saved_orders(None)


def solve_spherical(s: Solver, tau, P0a, P0r, z, earth_radius=EARTH_RADIUS_KM, tol=1e-4, save_orders=False, device=0,
                    fetch_field=True, want=(), z_profile=None, keep_device=False):
    """The solve of handle `s` (grid, phase matrices and columns set) with the PSEUDO-SPHERICAL DIRECT BEAM:
    the beam's slant optical depth through spherical shells at the altitudes `z` [L] (km, descending), the first order layer
    by layer on that path, then the order loop as it is, fed that first order (`Solver.beam_slant_device`,
    `first_order_beam_device`, `solve_device(d_I1=...)`).  `want`: names of `Solver.epilogue` to compute from the resident
    field with the beam terms on the slant path (`z_profile` for the heating rate).  Returns (SolveResult, sigma [B, L],
    dict of the wanted epilogue arrays); keep_device=True: the torch tensors {"I", "n", "status", "tau", "beam_slant"}
    instead, left on the device.  The handle goes back to its own stream and to its default per-order storage, also on error."""
    import torch

    def seed(up, dev, d_tau, B, p0a, p0r):
        d_z = up(z)
        d_sig = torch.empty((B, d_tau.shape[1]), dtype=torch.float64, device=dev)
        d_I1 = torch.empty((B, d_tau.shape[1], s.D), dtype=torch.float64, device=dev)
        s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), earth_radius, B=B)
        s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), p0a, p0r, d_I1.data_ptr(), B=B)
        return d_I1, {"beam_slant": d_sig}

    def epilogue(d_tau, d_I, d_zp, extra, out, B):
        s.epilogue_beam_device(d_tau, d_I, extra["beam_slant"].data_ptr(), d_zp, "crit", *out, B=B)

    r = _solve_resident(s, tau, P0a, P0r, seed, epilogue, tol, save_orders, device, fetch_field, want, z_profile, keep_device)
    return r if keep_device else (r[0], r[1]["beam_slant"], r[2])


def _thermal_args(source, planck, planck_surface, surface_emissivity, B, nb_layers, azimuths=None, view_azimuths=None,
                  mode_batch=False, mode_chunk=None, beam="plane", first_order="coded", devices=None):
    """Checks of the `source` keyword, made before any handle exists: None for the solar source, else (planck [B, L],
    planck_surface [B], emissivity [B] or None) of the thermal one."""
    if not isinstance(source, str) or source not in ("solar", "thermal"):
        raise ValueError("source must be 'solar' or 'thermal' (got %r)" % (source,))
    if source == "solar":
        if planck is not None or planck_surface is not None or surface_emissivity is not None:
            raise ValueError("planck, planck_surface and surface_emissivity belong to source='thermal': the solar source has no "
                             "emission term")
        return None
    if planck is None or planck_surface is None:
        raise ValueError("source='thermal' needs planck (the Planck radiance at every level, [L] or [B, L]) and planck_surface "
                         "(the ground's, a scalar or [B])")
    if azimuths is not None or mode_batch or mode_chunk is not None or view_azimuths is not None:
        raise ValueError("source='thermal' is not available with azimuths / mode_batch / view_azimuths: emission is isotropic in "
                         "azimuth and has only the m = 0 mode")
    if beam != "plane":
        raise ValueError("source='thermal' is not available with beam='spherical': the thermal field has no direct beam to bend")
    if first_order != "coded":
        raise ValueError("source='thermal' is not available with first_order='readme': the emitted field replaces the first order")
    if devices is not None and len(devices) > 1:
        raise ValueError("source='thermal' is not available with devices=[...]: solve each shard with SOS_Aer_batch(device=...)")
    L = int(nb_layers)
    try:
        pl = np.asarray(planck, dtype=np.float64)
        bs = np.asarray(planck_surface, dtype=np.float64)
        es = None if surface_emissivity is None else np.asarray(surface_emissivity, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("planck, planck_surface and surface_emissivity must be numbers") from None
    if pl.shape not in ((L,), (B, L)):
        raise ValueError("planck must have the shape [L] = (%d,) or [B, L] = (%d, %d): one Planck radiance per level (got %s)"
                         % (L, B, L, pl.shape))
    if bs.shape not in ((), (B,)):
        raise ValueError("planck_surface must be a scalar or [B] = (%d,) (got %s)" % (B, bs.shape))
    if es is not None and es.shape not in ((), (B,)):
        raise ValueError("surface_emissivity must be a scalar or [B] = (%d,) (got %s)" % (B, es.shape))
    full = lambda a, shape: np.ascontiguousarray(np.broadcast_to(a, shape))
    return full(pl, (B, L)), full(bs, (B,)), None if es is None else full(es, (B,))


def _broadcast_columns(*cols):
    """The per-column arguments of a batch (scalars or arrays) as float64 arrays of their common length (views: nothing is
    copied)."""
    cols = [np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in cols]
    try:
        return np.broadcast_arrays(*cols)
    except ValueError:
        raise ValueError("the per-column arguments do not broadcast to a common length") from None


def _batch_width(*cols):
    """Columns of a batch whose per-column arguments broadcast to a common length."""
    return int(_broadcast_columns(*cols)[0].shape[0])


def solve_thermal(s: Solver, tau, planck, planck_surface, emissivity=None, tol=1e-4, save_orders=False, want=(), z_profile=None,
                  keep_device=False, device=0, fetch_field=True):
    """The solve of handle `s` (grid, phase matrices and columns set) with the THERMAL SOURCE: the field the
    layers and the ground emit (`planck` [B, L] the Planck radiance at every level, `planck_surface` [B], `emissivity` [B] or
    None for 1 - grd_alb), then the order loop as it is, fed that field (`Solver.emission_device`, `solve_device(d_I1=...)`);
    mu0 does not enter.  The three sources may be float64 torch tensors of those shapes on cuda:`device`: nothing is uploaded
    for them.  `want`: names of `Solver.epilogue` to compute from the field without beam terms (`epilogue_emission_device`;
    `z_profile` for the heating rate).  Returns (SolveResult, dict of the wanted epilogue arrays); keep_device=True: the torch
    tensors {"I", "n", "status", "tau"} instead, left on the device.  The handle goes back to its own stream and to its default
    per-order storage, also on error."""
    import torch

    def seed(up, dev, d_tau, B, p0a, p0r):
        def src(a, shape, name):
            # a torch tensor on the device is used where it lies (sosrt.bands builds the sources there); NumPy is uploaded
            if not isinstance(a, torch.Tensor):
                return up(np.broadcast_to(a, shape))
            if a.device != dev or a.dtype != torch.float64 or tuple(a.shape) != shape:
                raise ValueError("%s as a torch tensor must be float64 %s on %s (got %s %s on %s)"
                                 % (name, shape, dev, a.dtype, tuple(a.shape), a.device))
            return a.contiguous()
        L = d_tau.shape[1]
        d_pl, d_bs = src(planck, (B, L), "planck"), src(planck_surface, (B,), "planck_surface")
        d_es = None if emissivity is None else src(emissivity, (B,), "surface_emissivity")
        d_I0 = torch.empty((B, L, s.D), dtype=torch.float64, device=dev)
        s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr(), 0 if d_es is None else d_es.data_ptr(), B=B)
        return d_I0, {}

    def epilogue(d_tau, d_I, d_zp, extra, out, B):
        s.epilogue_emission_device(d_tau, d_I, d_zp, *out, B=B)

    r = _solve_resident(s, tau, None, None, seed, epilogue, tol, save_orders, device, fetch_field, want, z_profile, keep_device)
    return r if keep_device else (r[0], r[2])


def _gas_args(gas_tau, B, nb_layers, azimuths=None, view_mu=None, view_azimuths=None, mode_batch=False, mode_chunk=None,
              surface="specular", delta_m=None, first_order="coded", save_orders=False, devices=None, gas_view=False):
    """Checks of the `gas_tau` keyword, made before any handle exists: None, or a namespace with gas_tau [B, L] that
    `_prepare_batch` fills (tau0, the row weights).  B is a number or a callable that gives it.  The stages that evaluate one
    constant per zone are refused (open items); `gas_view=True` opens `view_mu`, whose stage then runs on
    the weighted entries."""
    if not isinstance(gas_view, (bool, np.bool_)):
        raise ValueError("gas_view must be True or False (got %r)" % (gas_view,))
    if gas_tau is None:
        if gas_view:
            raise ValueError("gas_view=True belongs to gas_tau: without a gas profile the view stage needs no keyword")
        return None
    no = lambda what, why: ValueError("gas_tau is not available with %s: %s" % (what, why))
    if azimuths is not None:
        raise no("azimuths", "the first order of a Fourier mode evaluates one scattering coefficient per zone")
    if gas_view:
        if view_mu is None:
            raise ValueError("gas_view=True is the view stage under gas_tau: give view_mu")
        if view_azimuths is not None:
            raise no("view_azimuths, also with gas_view=True", "the modes m >= 1 are not solved under per-level weights yet")
    elif view_mu is not None or view_azimuths is not None:
        raise no("view_mu / view_azimuths", "the view stage evaluates one scattering coefficient per zone")
    if mode_batch or mode_chunk is not None:
        raise no("mode_batch / mode_chunk", "they belong to azimuths")
    if surface == "brdf":
        raise no("surface='brdf'", "the ground's series takes its first orders from the order loop's closed form")
    if delta_m is not None:
        raise no("delta_m", "the scaled column's first order is the closed form")
    if first_order != "coded":
        raise no("first_order='readme'", "the README's first order has no layer-by-layer form")
    if save_orders:
        raise no("save_orders", "the per-order history starts from the handle's own first order")
    if devices is not None and len(devices) > 1:
        raise no("devices=[...]", "solve each shard with SOS_Aer_batch(device=...)")
    B, L = int(B() if callable(B) else B), int(nb_layers)
    try:
        g = np.asarray(gas_tau, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("gas_tau must be numbers") from None
    if g.shape not in ((L,), (B, L)):
        raise ValueError("gas_tau must have the shape [L] = (%d,) or [B, L] = (%d, %d): the cumulative absorption optical depth of "
                         "the gases at every level (got %s)" % (L, B, L, g.shape))
    if not np.all(np.isfinite(g)):
        raise ValueError("gas_tau must be finite")
    if np.any(g[..., 0] != 0):
        raise ValueError("gas_tau is cumulative from the top: it must be 0 at level 0")
    if np.any(np.diff(g, axis=-1) < 0):
        raise ValueError("gas_tau is cumulative from the top: it must not decrease with the level")
    return SimpleNamespace(gas_tau=np.ascontiguousarray(np.broadcast_to(g, (B, L))), tau0=None, w=None)


def solve_profile(s: Solver, tau, P0a, P0r, w, mu0=None, z=None, earth_radius=EARTH_RADIUS_KM, thermal=None, tol=1e-4, device=0,
                  fetch_field=True, want=(), z_profile=None, keep_device=False, w_aer=None, post=None):
    """The solve of handle `s` (grid, phase matrices and columns set) with PER-LEVEL WEIGHTS ON THE SOURCE FUNCTION (DESIGN section
    29): `w` [B, L] multiplies the atmosphere's row coefficient, `w_aer` (default `w`: an absorbing gas weighs both alike) the
    aerosol's (`Solver.set_row_weights_device`); `tau` [B, L] is the total optical depth, gas included.  Solar (`mu0` [B]): the
    first order layer by layer with the weights in its scattering coefficient (`first_order_profile_device`) on the plane beam
    sigma = tau / mu0, or with `z` [L] (km, descending) on the slant path of `beam_slant_device`; `thermal` = (planck [B, L],
    planck_surface [B], emissivity [B] or None): the emitted field with the weights in its emission coefficient
    (`emission_profile_device`).  Then the order loop from that field, and for the names `want` the epilogue that goes with the
    source.  Returns (SolveResult, sigma [B, L] or None, dict of the wanted epilogue arrays); keep_device=True: the torch tensors
    {"I", "n", "status", "tau"[, "beam_slant"]} instead.  `post(dev, d_tau, d_I, d_sigma, B)` runs behind the solve, on the
    resident field and inside the stream scope, WHILE THE WEIGHTS ARE SET (the view stage of DESIGN section 30): torch tensors
    d_tau [B, L], d_I [B, L, 2N] and d_sigma [B, L] (the beam path of the first order; None with `thermal`); what it returns is
    dropped.  The weights are cleared when the call returns, also on error."""
    import torch
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), tau.shape))
    wr = w if w_aer is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w_aer, dtype=np.float64), tau.shape))
    if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(np.isfinite(wr)) and np.all(wr >= 0)):
        raise ValueError("the row weights must be finite and >= 0")
    if thermal is None and mu0 is None:
        raise ValueError("solve_profile needs mu0 (the solar source) or thermal")

    kept = {}

    def seed(up, dev, d_tau, B, p0a, p0r):
        L = d_tau.shape[1]
        d_w = up(w)
        d_wr = d_w if wr is w else up(wr)
        s.set_row_weights_device(d_w.data_ptr(), d_wr.data_ptr(), B=B)
        d_I1 = torch.empty((B, L, s.D), dtype=torch.float64, device=dev)
        if thermal is not None:
            def src(a, shape):
                return a.contiguous() if isinstance(a, torch.Tensor) else up(np.broadcast_to(a, shape))
            d_pl, d_bs = src(thermal[0], (B, L)), src(thermal[1], (B,))
            d_es = None if thermal[2] is None else src(thermal[2], (B,))
            s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I1.data_ptr(),
                                      0 if d_es is None else d_es.data_ptr(), B=B)
            return d_I1, {}
        if z is None:
            d_sig = up(tau / np.broadcast_to(np.asarray(mu0, dtype=np.float64), (B,))[:, None])
        else:
            d_z = up(z)
            d_sig = torch.empty((B, L), dtype=torch.float64, device=dev)
            s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), earth_radius, B=B)
        s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), p0a, p0r, d_I1.data_ptr(), B=B)
        kept["sigma"] = d_sig
        return d_I1, {"beam_slant": d_sig}

    def epilogue(d_tau, d_I, d_zp, extra, out, B):
        if thermal is not None:
            s.epilogue_emission_device(d_tau, d_I, d_zp, *out, B=B)
        elif z is None:
            s.epilogue_device(d_tau, d_I, d_zp, "crit", *out)
        else:
            s.epilogue_beam_device(d_tau, d_I, extra["beam_slant"].data_ptr(), d_zp, "crit", *out, B=B)

    def after(up, dev, d_tau, d_I, d_n, d_st, B, p0a, p0r):
        post(dev, d_tau, d_I, kept.get("sigma"), B)
        return {}

    try:
        r = _solve_resident(s, tau, None if thermal is not None else P0a, None if thermal is not None else P0r, seed, epilogue, tol,
                            False, device, fetch_field, want, z_profile, keep_device, None if post is None else after)
    finally:
        s.set_row_weights_device(0, 0)
    if keep_device:
        if z is None:
            r.pop("beam_slant", None)
        return r
    return r[0], (r[1].get("beam_slant") if z is not None else None), r[2]


MAX_BOUNCES = 32
BRDF_NPHI = 65
ROSS_LI_MU_FLOOR = 0.17364817766693033    # cos 80 deg: the Ross-Li kernels carry sec theta and are not meant for grazing angles
COX_MUNK_INDEX = 1.34                     # sea water in the visible
COX_MUNK_MAX_WINDS = _lib.BRDF_MAX_TERMS - 1   # every distinct wind is one glint term beside the isotropic one


def _cox_munk_args(spec, brdf, B):
    """The ocean ground ('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]]) of `_brdf_args` (DESIGN section
    26), rho = f_iso + f_glint rho_glint: spec.terms = the isotropic term, then one glint term (sigma2, n, shadow) per distinct
    wind speed, ascending; spec.weight [B, 1 + winds] = f_iso, then f_glint on the column's own wind and 0 on the others."""
    if not 2 <= len(brdf) <= 6:
        raise ValueError("the Cox-Munk brdf is ('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]]) (got %r)" % (brdf,))
    shadow = brdf[5] if len(brdf) > 5 else True
    if not (isinstance(shadow, (bool, np.bool_)) or (isinstance(shadow, (int, float, np.integer, np.floating)) and shadow in (0, 1))):
        raise ValueError("the Cox-Munk shadow must be True or False (got %r)" % (shadow,))
    try:
        wind = np.asarray(brdf[1], dtype=np.float64)
        n = float(brdf[2]) if len(brdf) > 2 else COX_MUNK_INDEX
        f = [np.asarray(brdf[i] if len(brdf) > i else d, dtype=np.float64) for i, d in ((3, 0.0), (4, 1.0))]
    except (TypeError, ValueError):
        raise ValueError("the Cox-Munk wind_speed, refractive_index, f_iso and f_glint must be numbers (got %r)" % (brdf[1:],)) from None
    if wind.shape not in ((), (1,), (B,)) or not np.all(np.isfinite(wind)) or np.any(wind < 0):
        raise ValueError("the Cox-Munk wind_speed (m/s at 10 m) must be finite, >= 0 and a scalar or [B] = (%d,)" % B)
    if not (np.isfinite(n) and n > 1):
        raise ValueError("the Cox-Munk refractive_index=%g: need a finite real index > 1" % n)
    if any(x.shape not in ((), (1,), (B,)) or not np.all(np.isfinite(x)) or np.any(x < 0) for x in f):
        raise ValueError("the Cox-Munk weights f_iso, f_glint must each be finite, >= 0 and a scalar or [B] = (%d,)" % B)
    if all(np.all(x == 0) for x in f):
        raise ValueError("the Cox-Munk weights f_iso, f_glint are both zero: a black ground is surface='specular' with grd_alb=0")
    if np.any(spec.scale != 1):
        raise ValueError("brdf=('cox_munk', ...) carries its amplitude in its weights: grd_alb must be omitted or 1")
    column = lambda x: np.broadcast_to(x.reshape(-1) if x.ndim else x, (B,))
    winds, own = np.unique(column(wind), return_inverse=True)
    if len(winds) > COX_MUNK_MAX_WINDS:
        raise ValueError("brdf=('cox_munk', ...) takes at most %d distinct wind speeds in one batch (got %d): every wind is an "
                         "operator term of its own; make one call per wind" % (COX_MUNK_MAX_WINDS, len(winds)))
    spec.kind, spec.params = "cox_munk", (n, float(shadow))
    spec.terms = (("lambertian", ()),) + tuple(("cox_munk", (float(slope_variance(u)), n, float(shadow))) for u in winds)
    spec.weight = np.zeros((B, 1 + len(winds)))
    spec.weight[:, 0] = column(f[0])
    spec.weight[np.arange(B), 1 + own.reshape(-1)] = column(f[1])
    return spec


def _brdf_args(surface, brdf, grd_alb, nb_angles, B, azimuths=None, view_mu=None, view_azimuths=None, mode_batch=False,
               mode_chunk=None, beam="plane", source="solar", first_order="coded", devices=None, save_orders=False,
               brdf_modes=False, brdf_view=False):
    """Checks of surface='brdf', made before any handle exists: None for every other surface, else a namespace (kind, params,
    R [N-1, N-1] or None, r0 [B, N-1] or None, scale [B], modes; terms, weight) of the ground `brdf` with `grd_alb` as its
    per-column scale; terms: None, or for ('ross_li', ...) and ('cox_munk', ...) the (kind, params) of its operator terms, with weight [B, K] their
    per-column weights;
    modes: the call is the azimuth-resolved one over the ground's Fourier modes (`brdf_modes=True` with `azimuths`); view: the
    call adds the ground's term at the view lanes (`brdf_view=True` with `view_mu`)."""
    if not isinstance(brdf_modes, (bool, np.bool_)):
        raise ValueError("brdf_modes must be True or False (got %r)" % (brdf_modes,))
    if not isinstance(brdf_view, (bool, np.bool_)):
        raise ValueError("brdf_view must be True or False (got %r)" % (brdf_view,))
    if not (isinstance(surface, str) and surface == "brdf"):
        if brdf is not None:
            raise ValueError("brdf belongs to surface='brdf'")
        if brdf_modes:
            raise ValueError("brdf_modes belongs to surface='brdf' (with brdf= and azimuths=)")
        if brdf_view:
            raise ValueError("brdf_view belongs to surface='brdf' (with brdf= and view_mu=)")
        return None
    if brdf is None:
        raise ValueError("surface='brdf' needs brdf: 'lambertian', ('rpv', rho0, k, theta), ('ross_li', f_iso, f_vol, f_geo[, "
                         "mu_floor]), ('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]]) or the arrays (R, r0)")
    if brdf_view:
        if view_mu is None:
            raise ValueError("brdf_view=True is the view stage over the BRDF ground: give view_mu")
        if azimuths is not None or brdf_modes:
            raise ValueError("surface='brdf' with brdf_view=True is not available with azimuths / brdf_modes: view_mu and the "
                             "grid's azimuth synthesis do not go together (the radiance at a view cosine and an azimuth is "
                             "view_azimuths=[...])")
        if mode_batch or mode_chunk is not None:
            raise ValueError("surface='brdf' with brdf_view=True is not available with mode_batch / mode_chunk: the series in "
                             "ground reflections runs inside the loop over the modes, on one mode's resident field")
    elif brdf_modes:
        if azimuths is None:
            raise ValueError("brdf_modes=True is the azimuth-resolved call over the BRDF ground: give azimuths")
        if mode_batch or mode_chunk is not None or view_azimuths is not None:
            raise ValueError("surface='brdf' with brdf_modes=True is not available with mode_batch / mode_chunk / view_azimuths: "
                             "the series in ground reflections runs inside the loop over the modes, on one mode's resident field")
    elif azimuths is not None or mode_batch or mode_chunk is not None or view_azimuths is not None:
        raise ValueError("surface='brdf' is not available with azimuths / mode_batch / view_azimuths: only the azimuth mean "
                         "(mode m = 0) of the BRDF is built (azimuths over the ground's modes m >= 1: brdf_modes=True)")
    if view_mu is not None and not brdf_view:
        raise ValueError("surface='brdf' is not available with view_mu: the view stage has no ground-reflection term "
                         "(the ground's term at the view lanes: brdf_view=True)")
    if beam != "plane":
        raise ValueError("surface='brdf' is not available with beam='spherical': the reflected beam is the plane one")
    if source != "solar":
        raise ValueError("surface='brdf' is not available with source='thermal': the ground's emission over a BRDF is not built")
    if first_order != "coded":
        raise ValueError("surface='brdf' is not available with first_order='readme': the series starts from the black-ground solve")
    if devices is not None and len(devices) > 1:
        raise ValueError("surface='brdf' is not available with devices=[...]: solve each shard with SOS_Aer_batch(device=...)")
    if save_orders:
        raise ValueError("surface='brdf' is not available with save_orders: the field is a sum over ground reflections, each "
                         "with orders of its own")
    N = int(nb_angles)
    if N < 4:
        raise ValueError("surface='brdf' needs nb_angles >= 4 (got %d)" % N)
    try:
        scale = np.asarray(grd_alb, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("grd_alb must be numbers") from None
    if scale.shape not in ((), (1,), (B,)) or not np.all(np.isfinite(scale)) or np.any(scale < 0):
        raise ValueError("grd_alb (the ground's per-column scale under surface='brdf') must be finite, >= 0 and a scalar or [B] = (%d,)" % B)
    scale = np.ascontiguousarray(np.broadcast_to(scale.reshape(-1) if scale.ndim else scale, (B,)))
    spec = SimpleNamespace(kind=None, params=(), R=None, r0=None, scale=scale, modes=bool(brdf_modes), view=bool(brdf_view),
                           terms=None, weight=None)
    if isinstance(brdf, str):
        if brdf != "lambertian":
            raise ValueError("brdf must be 'lambertian', ('rpv', rho0, k, theta), ('ross_li', ...), ('cox_munk', ...) or the arrays (R, r0) "
                             "(got %r)" % (brdf,))
        spec.kind = "lambertian"
        return spec
    if not isinstance(brdf, (tuple, list)) or len(brdf) < 2:
        raise ValueError("brdf must be 'lambertian', ('rpv', rho0, k, theta), ('ross_li', ...), ('cox_munk', ...) or the arrays (R, r0) "
                         "(got %r)" % (brdf,))
    if isinstance(brdf[0], str) and brdf[0] == "ross_li":
        if len(brdf) not in (4, 5):
            raise ValueError("the Ross-Li brdf is ('ross_li', f_iso, f_vol, f_geo) or ('ross_li', f_iso, f_vol, f_geo, mu_floor) "
                             "(got %r)" % (brdf,))
        try:
            f = [np.asarray(x, dtype=np.float64) for x in brdf[1:4]]
            floor = float(brdf[4]) if len(brdf) == 5 else ROSS_LI_MU_FLOOR
        except (TypeError, ValueError):
            raise ValueError("the Ross-Li weights f_iso, f_vol, f_geo and mu_floor must be numbers (got %r)" % (brdf[1:],)) from None
        if any(x.shape not in ((), (1,), (B,)) or not np.all(np.isfinite(x)) or np.any(x < 0) for x in f):
            raise ValueError("the Ross-Li weights f_iso, f_vol, f_geo must each be finite, >= 0 and a scalar or [B] = (%d,)" % B)
        if all(np.all(x == 0) for x in f):
            raise ValueError("the Ross-Li weights f_iso, f_vol, f_geo are all zero: a black ground is surface='specular' with "
                             "grd_alb=0")
        if not (np.isfinite(floor) and 0 <= floor < 1):
            raise ValueError("the Ross-Li mu_floor=%g: need 0 <= mu_floor < 1" % floor)
        if np.any(scale != 1):
            raise ValueError("brdf=('ross_li', ...) carries its amplitude in its weights: grd_alb must be omitted or 1")
        spec.kind, spec.params = "ross_li", (floor,)
        spec.terms = (("lambertian", ()), ("ross_thick", (floor,)), ("li_sparse_r", (floor,)))
        spec.weight = np.ascontiguousarray(np.stack([np.broadcast_to(x.reshape(-1) if x.ndim else x, (B,)) for x in f], axis=1))
        return spec
    if isinstance(brdf[0], str) and brdf[0] == "cox_munk":
        return _cox_munk_args(spec, brdf, B)
    if isinstance(brdf[0], str):
        if brdf[0] != "rpv" or len(brdf) != 4:
            raise ValueError("a named brdf is 'lambertian', ('rpv', rho0, k, theta), ('ross_li', f_iso, f_vol, f_geo[, mu_floor]) or "
                             "('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]]) (got %r)" % (brdf,))
        try:
            rho0, k, theta = (float(x) for x in brdf[1:])
        except (TypeError, ValueError):
            raise ValueError("the RPV parameters rho0, k, theta must be numbers (got %r)" % (brdf[1:],)) from None
        if not (np.isfinite(rho0) and rho0 > 0 and np.isfinite(k) and k > 0 and abs(theta) < 1):
            raise ValueError("RPV parameters rho0=%g, k=%g, theta=%g: need rho0 > 0, k > 0, |theta| < 1" % (rho0, k, theta))
        if np.any(scale != 1):
            raise ValueError("brdf=('rpv', ...) carries its amplitude in rho0: grd_alb must be omitted or 1")
        spec.kind, spec.params = "rpv", (rho0, k, theta)
        return spec
    if len(brdf) != 2:
        raise ValueError("brdf as arrays is the pair (R [N-1, N-1], r0 [N-1] or [B, N-1])")
    if brdf_modes:
        raise ValueError("brdf as arrays (R, r0) carries no azimuth information: brdf_modes=True needs a named brdf")
    if brdf_view:
        raise ValueError("brdf as arrays (R, r0) carries no rows off the grid: brdf_view=True needs a named brdf")
    try:
        R, r0 = np.asarray(brdf[0], dtype=np.float64), np.asarray(brdf[1], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("brdf as arrays is the pair (R [N-1, N-1], r0 [N-1] or [B, N-1]) of numbers") from None
    if R.shape != (N - 1, N - 1) or r0.shape not in ((N - 1,), (B, N - 1)):
        raise ValueError("brdf as arrays: R must be [N-1, N-1] = (%d, %d) and r0 [N-1] or [B, N-1] (got %s and %s)"
                         % (N - 1, N - 1, R.shape, r0.shape))
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(r0))):
        raise ValueError("brdf as arrays: R and r0 must be finite")
    spec.R, spec.r0 = R, np.ascontiguousarray(np.broadcast_to(r0, (B, N - 1)))
    return spec


def _reflection_scratch(s: Solver, dev, B, L):
    """The buffers of `_reflect`: d_S [B, N-1], d_G, d_Ik [B, L, 2N], d_ratio [B] and the int32 d_nk, d_stk, d_gst [B]."""
    import torch
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in ("d_nk", "d_stk", "d_gst")}
    return SimpleNamespace(d_S=f64(B, s.N - 1), d_G=f64(B, L, s.D), d_Ik=f64(B, L, s.D), d_ratio=f64(B), **i32)


def _per_term(ground, dev, shape, build, axis=0, skip_iso=False):
    """What a builder of the named BRDF `ground` fills, `build(kind, params, address)` writing a tensor of `shape`: that tensor,
    or for a ground of operator terms (ground.terms) the terms' tensors stacked along `axis`.  skip_iso: the isotropic term is
    not built and stays +0 (its modes m >= 1)."""
    import torch
    if not ground.terms:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
        build(ground.kind, ground.params, out.data_ptr())
        return out
    parts = []
    for kind, params in ground.terms:
        if skip_iso and kind == "lambertian":
            parts.append(torch.zeros(shape, dtype=torch.float64, device=dev))
            continue
        parts.append(torch.empty(shape, dtype=torch.float64, device=dev))
        build(kind, params, parts[-1].data_ptr())
    return torch.stack(parts, dim=axis).contiguous()


def _ground_scale(ground, dev):
    """The per-column factor of the ground source on the device: the scale [B], or the weights [B, K] of a ground of terms."""
    import torch
    return torch.from_numpy(np.array(ground.scale if ground.terms is None else ground.weight, dtype=np.float64)).to(dev)


def _view_ground(s: Solver, ground, mu_view, d_tau, levels, d_out, d_scale, **kw):
    """`Solver.view_ground_device` for the ground `ground`, `d_scale` of `_ground_scale` (a ground of terms: the terms kernel)."""
    if ground.terms:
        s.view_ground_terms_device(len(ground.terms), mu_view, d_tau, levels, d_scale, d_out, **kw)
    else:
        s.view_ground_device(mu_view, d_tau, levels, d_out, d_scale=d_scale, **kw)


def _reflect(s: Solver, B, k, d_tau, d_total, R, r0, d_scale, buf, status, hook=None, terms=0, **solve_kw):
    """Ground reflection k >= 1, enqueued: the ground source (`R`, `d_scale`; terms = K > 0: the stacks `R` [K, N-1, N-1], `r0`
    [K, B, N-1] and the weights `d_scale` [B, K], `Solver.ground_source_terms_device`) of the downward surface row of `src`, the last term
    buf.d_Ik (reflection 1: `d_total`, which holds the black solve, with the beam rows `r0`) -> `hook(k, src)`, for what reads the
    same source -> its unscattered field -> the order loop from it (`solve_kw`: what else `Solver.solve_device` takes) into buf.d_Ik,
    its orders into buf.d_nk -> d_total += buf.d_Ik, buf.d_ratio.  `status` [B] takes the ground field's, else the solve's, where 0."""
    import torch
    src = d_total if k == 1 else buf.d_Ik
    if terms:
        s.ground_source_terms_device(terms, src.data_ptr(), d_tau.data_ptr(), R.data_ptr(), d_scale.data_ptr(), buf.d_S.data_ptr(),
                                     r0.data_ptr() if k == 1 else 0, B=B)
    else:
        s.ground_source_device(src.data_ptr(), d_tau.data_ptr(), R.data_ptr(), buf.d_S.data_ptr(), r0.data_ptr() if k == 1 else 0,
                               d_scale.data_ptr(), B=B)
    if hook is not None:
        hook(k, src)
    s.ground_first_order_device(d_tau.data_ptr(), buf.d_S.data_ptr(), buf.d_G.data_ptr(), buf.d_gst.data_ptr(), B=B)
    s.solve_device(d_tau.data_ptr(), d_I_out=buf.d_Ik.data_ptr(), d_I1=buf.d_G.data_ptr(), d_n_orders=buf.d_nk.data_ptr(),
                   d_status=buf.d_stk.data_ptr(), **solve_kw)
    s.bounce_accumulate_device(buf.d_Ik.data_ptr(), d_total.data_ptr(), buf.d_ratio.data_ptr(), B=B)
    status.copy_(torch.where(status != 0, status, torch.where(buf.d_gst != 0, buf.d_gst, buf.d_stk)))


def solve_brdf(s: Solver, tau, P0a, P0r, spec, mu0, tol=1e-4, max_bounces=MAX_BOUNCES, nphi=BRDF_NPHI, device=0, fetch_field=True,
               want=(), z_profile=None, keep_device=False, view=None):
    """The solve of handle `s` (grid, phase matrices set; columns set over a BLACK ground: the specular surface with albedo 0)
    over the BRDF GROUND `spec` of `_brdf_args`: the plain solve, then on the device the series in ground
    reflections (`_reflect`, of the last term's downward surface row and, in the first bounce, of the direct beam) until every
    column's term is below `tol` of the sum on the TOA-up and surface-down lanes, or `max_bounces`; B ratios come back per
    bounce, nothing else.  Every column runs every bounce of the batch.  `want`: names of `Solver.epilogue` from the summed field
    (`epilogue_device`: over the black ground its reflected-beam term is zero; the reflected beam is in the field).  Returns
    (SolveResult, {"bounces" [B]: the bounce at which the column fell below tol, "bounce_ratio" [B]: its last ratio,
    "bounce_orders" [K, B]: the orders the solve of every bounce ran}, dict of the wanted epilogue arrays); keep_device=True: the
    torch tensors {"I", "n", "status", "tau", "bounces", "bounce_ratio", "bounce_orders"} instead.  n is the black solve's; a column
    still above tol at the cap has status COL_MAXORDERS, one whose ground rows fail the mu -> 0 search COL_INDEXERROR.

    A ground of operator terms (spec.terms, the Ross-Li ground): the K operators and beam-row stacks are built
    once (`_per_term`), every reflection's ground source sums them with the column's weights (`Solver.ground_source_terms_device`),
    and "black_sky_albedo" / "white_sky_albedo" [B], sum_i 2 w_i mu_i sum_k f_k r0_k[b][i] and sum_i 2 w_i mu_i sum_j sum_k f_k
    R_k[j][i] on the upward nodes' trapezoid, join the second value.

    `view` = (view_mu [V], levels) (a named BRDF only): also THE GROUND'S UNSCATTERED RADIANCE AT THE VIEW LANES,
    summed over the reflections on the same sources the ground source reads -- the beam's single reflection written once, every
    reflection's diffuse part accumulated (`Solver.view_ground_device`): "I_view_ground_beam", "I_view_ground_diffuse"
    [B, nlev, 2V] and their sum "I_view_ground" join the second value.  The field and the counts do not change by a bit."""
    import torch
    if s.single_slab:
        raise ValueError("surface='brdf' is not available for the single slab: it has no ground")
    max_bounces = int(max_bounces)
    if max_bounces < 1:
        raise ValueError("max_bounces must be >= 1 (got %d)" % max_bounces)

    def post(up, dev, d_tau, d_I, d_n, d_st, B, p0a, p0r):
        L, M = d_tau.shape[1], s.N - 1
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        d_scale, K = _ground_scale(spec, dev), len(spec.terms or ())
        if spec.R is None:
            d_mu0 = up(np.broadcast_to(np.asarray(mu0, dtype=np.float64), (B,)))
            d_R = _per_term(spec, dev, (M, M), lambda kind, par, out: s.brdf_operator_device(kind, out, par, nphi))
            d_r0 = _per_term(spec, dev, (B, M), lambda kind, par, out: s.brdf_beam_device(kind, d_mu0.data_ptr(), out, par, nphi, B=B))
        else:
            d_R, d_r0 = up(spec.R.T), up(spec.r0)            # (the device reads the lanes i of one j contiguously)
        buf = _reflection_scratch(s, dev, B, L)
        bounces, orders, view_hook = np.zeros(B, dtype=np.int32), [], None
        if view is not None:
            vmu, vlev = view
            V = len(vmu)
            d_Rv = _per_term(spec, dev, (M, V), lambda kind, par, out: s.brdf_view_rows_modes_device(kind, vmu, out, 0, 1, par, nphi))
            d_r0v = _per_term(spec, dev, (B, V), lambda kind, par, out: s.brdf_view_beam_modes_device(kind, d_mu0.data_ptr(), vmu, out,
                                                                                                     0, 1, par, nphi, B=B))
            d_vb, d_vd = f64(B, len(vlev), 2 * V), f64(B, len(vlev), 2 * V)
            _view_ground(s, spec, vmu, d_tau.data_ptr(), vlev, d_vb.data_ptr(), d_scale.data_ptr(), d_r0v=d_r0v.data_ptr(), B=B)
            def view_hook(k, src):                          # reflection k's diffuse part, from the source the ground source has just read
                _view_ground(s, spec, vmu, d_tau.data_ptr(), vlev, d_vd.data_ptr(), d_scale.data_ptr(), d_I=src.data_ptr(),
                             d_Rv=d_Rv.data_ptr(), accumulate=k > 1, B=B)
        for k in range(1, max_bounces + 1):
            _reflect(s, B, k, d_tau, d_I, d_R, d_r0, d_scale, buf, d_st, view_hook, K, d_P0_atm=p0a, d_P0_aer=p0r, tol=tol)
            orders.append(buf.d_nk.clone())
            s.synchronize()
            ratio = buf.d_ratio.cpu().numpy()
            bounces[(bounces == 0) & (ratio < tol)] = k
            if np.all(ratio < tol):
                break
        late = torch.from_numpy(bounces == 0).to(dev) & (d_st == 0)
        d_st.copy_(torch.where(late, torch.full_like(d_st, _lib.COL_MAXORDERS), d_st))
        bounces[bounces == 0] = k
        out = {"bounces": torch.from_numpy(bounces).to(dev), "bounce_ratio": buf.d_ratio, "bounce_orders": torch.stack(orders)}
        if view is not None:
            out.update(I_view_ground_beam=d_vb, I_view_ground_diffuse=d_vd, I_view_ground=d_vb + d_vd)
        if K:
            # the albedos of the weighted ground on the grid's own quadrature, from the rows already built: 2 w_i mu_i over the
            # upward nodes, w their trapezoid weights
            u = s.mu[s.N + 1:]
            w = np.empty(M)
            w[0], w[-1], w[1:-1] = (u[1] - u[0]) / 2, (u[-1] - u[-2]) / 2, (u[2:] - u[:-2]) / 2
            d_wmu = up(2 * w * u)
            out.update(black_sky_albedo=torch.einsum("bk,kbi,i->b", d_scale, d_r0, d_wmu),
                       white_sky_albedo=torch.einsum("bk,k->b", d_scale, torch.einsum("kji,i->k", d_R, d_wmu)))
        return out

    def epilogue(d_tau, d_I, d_zp, extra, out, B):
        s.epilogue_device(d_tau, d_I, d_zp, "crit", *out)

    r = _solve_resident(s, tau, P0a, P0r, None, epilogue, tol, False, device, fetch_field, want, z_profile, keep_device, post=post)
    return r if keep_device else (r[0], r[1], r[2])


def SOS_Aer_batch(mu0, tauStar_aer, grd_alb, *, tauStar_atm=0.124, alb_atm=1.0, alb_aer=1.0, z0=120, z_up=25, z_down=17,
                  nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7,
                  mie_atm=None, mie_aer=None,
                  P_atm=None, P_aer=None, P0_atm=None, P0_aer=None, surface="specular", tol=1e-4, max_orders=256,
                  save_orders=False, device=0, devices=None, raise_on_error=True, first_order="coded", azimuths=None,
                  n_modes=None, nphi_modes=None, levels=(0, -1), aer_set=None, mode_batch=False, mode_chunk=None,
                  view_mu=None, view_levels=(0, -1), view_quadrature="grid", view_azimuths=None,
                  view_first_order="exact", beam="plane", earth_radius=EARTH_RADIUS_KM, source="solar", planck=None,
                  planck_surface=None, surface_emissivity=None, brdf=None, max_bounces=MAX_BOUNCES,
                  brdf_modes=False, brdf_view=False, beam_stages=False, delta_m=None, gas_tau=None, gas_view=False) -> BatchResult:
    """Solve B independent columns (arrays mu0, tauStar_aer, grd_alb broadcast to a common length;
    tauStar_atm, alb_atm, alb_aer may be arrays too).  Phase functions that are not handed in as arrays are built on the
    device (`device_phase`): any name of `inputs.phase_function`, `mie_atm` / `mie_aer` = dict(r=, lambda0=, indx=, r_m=,
    sig=[, device=True: the Mie table from the device builder]) for the Mie-derived ones ('eva' and 'wildfire' default to the
    README's scenarios).
    `first_order='readme'`: the README's Lambertian first order
    (Solver.set_first_order; parity unpinned, single device).  `devices=[0, 1, ...]` shards the columns over several
    GPUs of the node, one worker process each, and gathers the fields (sosrt.dist.solve_on_devices; per-order
    fields are not gathered).

    `aer_set` [B] (integers): SEVERAL AEROSOLS IN ONE BATCH, column b takes aerosol aer_set[b].  Either `P_aer` is a stack
    [S, 2N, 2N] with `P0_aer` [B, 2N] (each column the P0 of its own aerosol), or `aer_phase_fun` (and, where they differ,
    `g_aer` / `mie_aer`) is a list of S names (numbers / dicts) and the matrices and every column's P0 are built on the device.
    (A `solver.DevicePhaseSets` in `P_aer` names a stack that is already on the device.)
    Column b has the bits it has in a batch of its own aerosol alone (Solver.set_phase_sets / set_aerosol_sets).  Not with
    `azimuths`, `first_order='readme'` or several `devices`.

    `azimuths` (radians, array): also the azimuth-resolved radiance I(phi) at the rows `levels` (default TOA and surface),
    BatchResult.I_azimuth [B, len(levels), 2N, len(azimuths)], from the Fourier modes m = 0 .. `n_modes` (default 16) of the
    phase functions (`azimuth_modes`; modes m >= 1 built on `nphi_modes` azimuth nodes, default max(25, 2 n_modes + 1)).  phi
    follows the reference's ring: phi = 0 with an upward mu = mu0 is exact back-scatter.  I, n and status are those of the
    plain call, bit for bit.  Needs named phase functions (not arrays), the specular surface and a single device.
    `mode_batch=True` (opt-in; the default is the loop over the modes): the modes m >= 1 of all B columns are solved as ONE
    batch of c x B columns per chunk of c modes, the mode as the atmosphere and aerosol phase set of its columns
    (`azimuth_modes_batched`), and one launch sums all modes -- for a few columns, whose per-mode solves are bound by latency.
    Same bits as the loop.  c is the largest count that keeps c B columns within MODE_BATCH_FIELD_BYTES per field buffer,
    c x (distinct slab coefficient pairs) within the combined-matrix cache, and c <= 64; `mode_chunk=k` forces c = k.  The
    atmosphere's modes must be low-rank (iso, Rayleigh): otherwise ValueError, and `mode_batch=False` works.  Memory: the chunk
    bounds the handle's buffers only.  The fields of all modes wait for the one synthesis launch, n_modes x B x L x 2N doubles
    whatever c is (the loop keeps one mode's); beyond MODE_BATCH_MODES_BYTES the call is refused.  The cached handle is made
    c B columns wide and, like every widened handle of `get_solver`, stays that wide for later calls of this shape.

    `view_mu` (array of up to 64 cosines in [0.01, 1]): also the RADIANCE AT VIEW COSINES THAT ARE NOT NODES of the direction
    grid, at the rows `view_levels` (default TOA and surface): BatchResult.I_view [B, len(view_levels), 2V] on the signed
    lanes BatchResult.view_mu_signed = (-view_mu, +view_mu), the sum of I_view_first (the closed-form first order at the
    lanes) and I_view_scattered (the source function of the solved field I, integrated along the line of sight at the view
    cosine: `Solver.view_radiance_device`).  `view_quadrature='grid'` (default) is the reference's arithmetic per lane -- the
    trapezoid rule of its transport, without the mu -> 0 treatments of the grid: at a node it returns the grid's value (to
    the stopping rule's `tol`, because the source of I includes the last computed order, the series' next term); where the
    optical-depth step over the view cosine is >~ 1 it inherits the trapezoid rule's overshoot.  `'linear'` attenuates a
    piecewise-linear source exactly: the quadrature for limb-ward views.  I, n and status are those of the plain call, bit
    for bit.  Needs named phase functions (not arrays), the specular surface, the coded first order and a single device; not
    with `azimuths` or `aer_set`.

    `view_azimuths` (radians, array; needs `view_mu`): also the RADIANCE AT A VIEW COSINE AND A RELATIVE AZIMUTH,
    BatchResult.I_view_azimuth [B, len(view_levels), 2V, len(view_azimuths)] = I_view_azimuth_first + I_view_azimuth_scattered:
    the view stage run per Fourier mode m = 0 .. `n_modes` (default 16; `nphi_modes` as for `azimuths`) on the field of that
    mode, solved with the order counts of mode 0, and summed over the modes at the view lanes (`view_azimuth_modes`).  phi = 0
    with an upward view_mu = mu0 is back-scatter.  `view_first_order='exact'` (default): the first order from the phase
    function at (lane, azimuth) itself, without the truncation at n_modes, which rings for a forward-peaked aerosol;
    `'modes'`: the sum of the modes' first orders.  BatchResult.view_mode_status [n_modes + 1, B].  I, n, status and I_view*
    are those of the call without `view_azimuths`, bit for bit.  Not with `azimuths`, `mode_batch` or `mode_chunk`.

    `beam='spherical'`: the PSEUDO-SPHERICAL DIRECT BEAM.  The direct solar beam is attenuated along its slant path through
    spherical shells of radius `earth_radius` (km) + np.linspace(z0, 0, nb_layers) instead of exp(-tau / mu0); everything
    scattered is transported plane-parallel as before (`solve_spherical`; the reflected beam travels upward plane-parallel).
    At mu0 = 0.21 the converged field moves by about 7 % of its maximum, at mu0 = 0.6 by 0.3 %.  BatchResult.beam_slant [B, L]
    is the beam's slant optical depth at every level (None for 'plane').  `beam='plane'` (default) is the code path as it
    was.  Works with phase functions by name or as arrays, `aer_set` and `save_orders`; not with `azimuths`, `view_mu`,
    `view_azimuths`, `mode_batch`, `first_order='readme'` or several `devices` (their first orders are plane closed forms).

    `beam_stages=True` (opt-in, with `beam='spherical'`): THE SPHERE IN THE AZIMUTH AND VIEW STAGES.  `azimuths`,
    `view_mu` and `view_azimuths` are then accepted, and every first order they compute is taken on the slant path of the mode-0
    solve (`beam_slant`): on the grid the first order of every Fourier mode (`Solver.first_order_beam_device` fed the mode's P0
    vectors, then the solve from it), at the view lanes the layer-by-layer first order at the view cosine
    (`Solver.view_first_order_beam_device`; with `view_first_order='exact'` one call serves all azimuths).  The scattered terms
    are plane-parallel and inherit the sphere through the field.  At mu0 = 0.21 the TOA view radiance moves by a few per cent of
    its maximum.  I, n and beam_slant are those of the spherical call without the stages, bit for bit.  Still refused:
    `mode_batch` / `mode_chunk`, `surface='brdf'`, `source='thermal'`, `first_order='readme'`, several `devices`.  With
    `beam='plane'` the keyword is a ValueError.

    `source='thermal'`: THERMAL EMISSION instead of the solar beam (`solve_thermal`).  `planck` ([L] or [B, L]) is the Planck
    radiance at every level in any unit -- the field comes out in it (`thermal.planck_radiance` gives W m-2 sr-1 um-1) --
    `planck_surface` (scalar or [B]) the ground's, `surface_emissivity` (scalar or [B]) the ground's emissivity, default
    1 - grd_alb.  A layer emits (1 - its single-scattering albedo) times a Planck radiance linear in tau across it; the order
    loop scatters and transports the emitted field as it is.  I (and I_saved) are the thermal field; mu0 does not enter.  With
    `view_mu`, I_view_first is the emission at the view lanes and I_view_scattered the view stage on I.  The orders n >= 1
    inherit the reference's mu -> 0 treatments, so the lanes next to mu = 0 may overshoot max(planck).  Not with `azimuths`,
    `mode_batch`, `view_azimuths` (emission has only the m = 0 mode), `beam='spherical'`, `first_order='readme'` or several
    `devices`.  `source='solar'` (default) is the code path as it was.

    `surface='brdf'` with `brdf=`: a GROUND WHOSE REFLECTANCE DEPENDS ON THE DIRECTIONS (`solve_brdf`), as a
    series in ground reflections around the unchanged order loop: the columns are solved over a black ground, then per
    reflection the last term's downward surface row (and once the direct beam) is reflected through the BRDF's azimuth-mean
    operator and the order loop transports and scatters that ground source, until every column's term is below `tol` of the
    sum or `max_bounces` (32; a column still above has status COL_MAXORDERS).  `brdf='lambertian'`: grd_alb[b] is the albedo,
    so an albedo sweep is one batch; `brdf=('rpv', rho0, k, theta)`: Rahman-Pinty-Verstraete with its hot spot (grd_alb
    omitted or 1); `brdf=('ross_li', f_iso, f_vol, f_geo[, mu_floor])`: the kernel-driven Ross-Thick / Li-Sparse-Reciprocal model
    rho = f_iso + f_vol K_vol + f_geo K_geo, every weight a scalar or [B] -- finite, >= 0, not all zero; the
    three operators are built once and every column's ground source sums them with its own weights, so a batch of pixels each
    with its own BRDF is one batch; both kernels are evaluated at max(mu, mu_floor), default ROSS_LI_MU_FLOOR = cos 80 deg (0:
    the formulas as written); rho is not clamped and can go negative for a large f_geo; grd_alb omitted or 1; the result then
    also has black_sky_albedo and white_sky_albedo [B] on the grid's quadrature;
    `brdf=('cox_munk', wind_speed[, refractive_index[, f_iso[, f_glint[, shadow]]]])`: the OCEAN, rho = f_iso +
    f_glint rho_glint with the sun glint of Cox and Munk's isotropic Gaussian slopes, sigma^2 = 0.003 + 0.00512 wind_speed (m/s at
    10 m; `ocean.slope_variance`), the unpolarised Fresnel reflectance of refractive_index (default COX_MUNK_INDEX = 1.34) and,
    with shadow (default True), the bidirectional Smith shadowing; f_iso (default 0: the water-leaving and whitecap reflectance,
    `ocean.whitecap_fraction`) and f_glint (default 1) are scalars or [B], finite, >= 0, not both zero; wind_speed is a scalar
    or [B] with at most COX_MUNK_MAX_WINDS = 3 distinct values -- every wind is an operator term, a column weighs its own with
    f_glint and the others with 0, and has the bits it has in a batch at its wind alone; more winds: one call per wind.  The
    specular direction is phi = pi.  rho_glint is not clamped: toward grazing incidence its directional-hemispherical reflectance
    on the grid's trapezoid exceeds 1 (1.07 on the lowest node at N = 128, 2 m/s).  grd_alb omitted or 1; black_sky_albedo and
    white_sky_albedo as for 'ross_li'; `brdf=(R, r0)`: a caller's operator R [N-1, N-1] (upward lane N+1+i from downward lane j, the flux
    quadrature folded in) and beam row r0 [N-1] or [B, N-1], grd_alb a plain scale.  BatchResult.bounces / bounce_ratio [B]
    / bounce_orders [K, B] (the orders of every reflection's solve); n is the black solve's.  Not with `mode_batch`,
    `beam='spherical'`, `source='thermal'`, `first_order='readme'`, `save_orders` or several `devices`; `azimuths` only with
    `brdf_modes=True`, `view_mu` / `view_azimuths` only with `brdf_view=True`.

    `brdf_modes=True` (with `surface='brdf'`, a named `brdf` and `azimuths`): the AZIMUTH-RESOLVED RADIANCE OVER THE BRDF GROUND
    (DESIGN section 21).  The Fourier modes m = 1 .. `n_modes` of the BRDF are built on the device (on the BRDF_NPHI = 65 nodes of
    its azimuth mean, so n_modes <= 63), and per mode, after the black solve of that mode, the series in ground reflections runs
    on the mode's resident field with (-1)^m R^m: every mode runs the reflections mode 0 ran, reflection k with the order counts
    of mode 0's reflection k.  I_azimuth then carries the ground's own azimuth dependence, RPV's hot spot at back-scatter
    (phi = 0 at an upward mu = mu0) among it; the ground's modes fall off as 1 / m^2 only (the hot spot is a cusp), so what n_modes
    leaves out is larger than over the specular ground.  `brdf='lambertian'` has no modes m >= 1: its I_azimuth is mode 0 plus
    the atmosphere's modes over a black ground.  I, n, status, bounces and bounce_ratio are those of the call without
    `azimuths`, bit for bit; mode_status [n_modes + 1, B] includes the reflections' solves and ground rows.

    `brdf_view=True` (with `surface='brdf'`, a named `brdf` and `view_mu`): the VIEW RADIANCE OVER THE BRDF GROUND (DESIGN section
    22).  I_view = I_view_first + I_view_scattered + I_view_ground: the closed-form first order over the black ground, the view
    stage on the field summed over the ground reflections, and the ground's own unscattered radiance at the view lanes,
    BatchResult.I_view_ground [B, nlev, 2V] -- every reflection's ground source at the view cosines (rows of the BRDF's operator
    built at mu_view, not interpolated from the grid) attenuated to the level; downward lanes 0; no view lane is blended.  With
    `view_azimuths` (n_modes <= 63) the ground's Fourier modes are implied: per mode the reflections run on the mode's resident
    field as under `brdf_modes`, the ground's term is accumulated per reflection with (-1)^m R^m at the view cosines, and
    I_view_azimuth = _first + _scattered + I_view_azimuth_ground.  `view_first_order='exact'` (default) also takes the beam's
    single reflection -- the largest carrier of RPV's hot spot -- from rho(mu_view, mu0, phi) at the azimuth itself, and the modes
    then carry the diffuse part only; `'modes'` sums rho^m(mu_view, mu0).  I, n, status, bounces, bounce_ratio and bounce_orders
    are those of the call without `view_mu`, I_view* those of the call without `view_azimuths`, bit for bit.  Not with the array
    form (R, r0), `azimuths`, `brdf_modes`, `mode_batch`, `aer_set` or phase arrays.

    `delta_m=Lambda` (2 .. 128; default None, the code path as it was): DELTA-M SCALING OF A FORWARD-PEAKED AEROSOL (DESIGN section
    28; `sosrt.deltam`).  The Legendre moments chi_l of the aerosol's phase function are taken on the device, the fraction f =
    chi_Lambda of its scattering is counted as unscattered, and the columns are solved with the table of the series truncated at
    Lambda -- sum over l < Lambda of (2l + 1) (chi_l - f) / (1 - f) P_l -- and the aerosol's tauStar_aer (1 - alb_aer f) and
    (1 - f) alb_aer / (1 - alb_aer f): an ordinary solve of a smooth function, in far fewer orders, and for a function the grid's
    quadrature does not hold (the cloud table 'fwc') the one that solves at all.  I, tau, fluxes and heating rates are those of
    the SCALED column: its direct beam contains the forward-scattered light, which is the method.  BatchResult.delta_m_f,
    tauStar_aer_scaled and alb_aer_scaled [B] say what was solved.  With `view_mu` the first order is the truncated function's,
    the ring mean: TMS is not applied to the azimuth mean.  With `view_mu` and `view_azimuths`, `n_modes` defaults to Lambda - 1,
    where the azimuth series of the truncated function ends, and `view_first_order='exact'` is the TMS FIRST ORDER (Nakajima &
    Tanaka 1988): the aerosol's values at (lane, azimuth) come from the exact function, divided by (1 - f), with the normaliser
    of the truncated table -- the grid's quadrature correction for the function the solve sees; `'modes'` stays the truncated
    series.  For a named aerosol 'hg' / 'fwc' / 'table' / 'mie' / 'eva' / 'wildfire'; not with `azimuths`, `aer_set` or lists,
    `P_aer` / `P0_aer`, `mode_batch`, `surface='brdf'`, `beam='spherical'`, `source='thermal'`, `first_order='readme'` or
    several `devices`.

    `gas_tau` ([L] or [B, L]; default None, the code path as it was): an ABSORBING GAS WHOSE AMOUNT VARIES WITH HEIGHT (DESIGN
    section 29; `solve_profile`).  It is the cumulative absorption optical depth of the gases at the L levels: 0 at the top,
    finite, non-decreasing.  The column is solved on tau = tau0 + gas_tau (tau0 the grid of `inputs.tau_profile`), and the source
    function of row t is weighted by the share of scattering in the layer above it, w_t = dtau0_t / (dtau0_t + dgas_t), w_0 = w_1
    (`inputs.gas_row_weights`), for molecules and aerosol alike: the first order layer by layer with the weights in its
    scattering coefficient, the order loop with the weights on its row coefficients, and with `source='thermal'` the emission
    coefficient 1 - w_t (the zone's albedo) per row, so the gas emits.  Works with `beam='spherical'` (the slant path of the total
    tau), `aer_set` and phase arrays.  BatchResult.tau is the total, gas_tau and row_weight [B, L] say what was solved.  Not with
    `azimuths`, `view_mu` (without `gas_view=True`, below), `view_azimuths`, `mode_batch`, `surface='brdf'`, `delta_m`,
    `first_order='readme'`, `save_orders` or several `devices`: those stages evaluate one constant per zone.

    `gas_view=True` (opt-in, with `gas_tau` and `view_mu`): THE GAS AT VIEW ANGLES.  The view stage runs on
    the resident field while the weights are set, on the weighted entries: the scattered term with the weights on the stage's row
    coefficients, the first term layer by layer with the weights in its scattering coefficient (on tau / mu0, or on the sphere's
    slant path with `beam='spherical', beam_stages=True`), and with `source='thermal'` the weighted emission at the lanes.
    Returns `view_mu_signed`, `I_view_first`, `I_view_scattered` and `I_view` as a view call does; `view_levels` and
    `view_quadrature` as there, and the view stage's own refusals (`aer_set`, phase arrays) hold.  I and n are those of the call
    without `view_mu`.  Still refused under `gas_tau`: `view_azimuths`, `azimuths`, `mode_batch`, `surface='brdf'`, `delta_m`,
    `first_order='readme'`, `save_orders`, several `devices`."""
    gas = _gas_args(gas_tau, lambda: _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer), nb_layers, azimuths,
                    view_mu, view_azimuths, mode_batch, mode_chunk, surface, delta_m, first_order, save_orders, devices, gas_view)
    dm = _delta_m_args(delta_m, aer_phase_fun, azimuths, aer_set, P_aer, P0_aer, mode_batch, mode_chunk, surface, beam, source,
                       first_order, devices)
    if dm is not None and view_azimuths is not None and n_modes is None:
        n_modes = dm.order - 1                               # where the azimuth series of the truncated function ends
    thermal = _thermal_args(source, planck, planck_surface, surface_emissivity,
                            _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer) if source == "thermal" else 0,
                            nb_layers, azimuths, view_azimuths, mode_batch, mode_chunk, beam, first_order, devices)
    ground = _brdf_args(surface, brdf, grd_alb, nb_angles,
                        _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer) if surface == "brdf" else 0,
                        azimuths, view_mu, view_azimuths, mode_batch, mode_chunk, beam, source, first_order, devices, save_orders,
                        brdf_modes, brdf_view)
    if ground:
        surface, grd_alb = "specular", 0.0                   # the series' solves run over a black ground
    spherical = _beam_args(beam, earth_radius, azimuths, view_mu, view_azimuths, mode_batch, mode_chunk, first_order, devices,
                           beam_stages)
    if view_azimuths is not None or view_first_order != "exact":
        vphi, vM, vnphi = _view_azimuth_args(view_azimuths, view_first_order, view_mu, azimuths, n_modes, nphi_modes, mode_batch,
                                             mode_chunk)
        if ground and vM > BRDF_NPHI - 2:
            raise ValueError("brdf_view=True builds the ground's modes on %d azimuth nodes: n_modes must be <= %d (got %d)"
                             % (BRDF_NPHI, BRDF_NPHI - 2, vM))
    if view_mu is not None:
        vmu, vlev, vquad = _view_args(view_mu, view_levels, view_quadrature, nb_layers, P_atm, P_aer, P0_atm, P0_aer, surface,
                                      devices, first_order, azimuths, aer_set, atm_phase_fun, aer_phase_fun)
    if aer_set is not None:
        if azimuths is not None:
            raise ValueError("azimuths are not available with aer_set (the mode driver swaps the handle's one pair of matrices per mode)")
        if first_order != "coded":
            raise ValueError("first_order='readme' is not available with aer_set (it reads one aerosol matrix)")
        if devices is not None and len(devices) > 1:
            raise ValueError("devices=[...] is not available with aer_set: solve each shard with SOS_Aer_batch(device=...)")
    elif np.ndim(P_aer) == 3 or isinstance(aer_phase_fun, (list, tuple)):
        raise ValueError("several aerosols (a stack P_aer [S, 2N, 2N] or a list of names) need aer_set [B]")
    if azimuths is not None:
        M, nphi, lev = _azimuth_args(azimuths, n_modes, nphi_modes, levels, nb_layers, P_atm, P_aer, P0_atm, P0_aer, surface,
                                     devices, first_order, mode_batch=mode_batch, mode_chunk=mode_chunk)
        if ground and M > BRDF_NPHI - 2:
            raise ValueError("brdf_modes=True builds the ground's modes on %d azimuth nodes: n_modes must be <= %d (got %d)"
                             % (BRDF_NPHI, BRDF_NPHI - 2, M))
    elif mode_batch or mode_chunk is not None:
        raise ValueError("mode_batch / mode_chunk belong to the azimuth-resolved call: give azimuths")
    if devices is not None and len(devices) > 1:
        if save_orders:
            raise ValueError("save_orders is not available with devices=[...]")
        if first_order != "coded":
            raise ValueError("first_order='readme' is not available with devices=[...]")
        from .dist import solve_on_devices
        r = solve_on_devices(devices, mu0, tauStar_aer, grd_alb, tauStar_atm=tauStar_atm, alb_atm=alb_atm, alb_aer=alb_aer,
                             z0=z0, z_up=z_up, z_down=z_down, nb_layers=nb_layers, nb_angles=nb_angles,
                             atm_phase_fun=atm_phase_fun, g_atm=g_atm, aer_phase_fun=aer_phase_fun, g_aer=g_aer,
                             mie_atm=mie_atm, mie_aer=mie_aer, P_atm=P_atm,
                             P_aer=P_aer, P0_atm=P0_atm, P0_aer=P0_aer, surface=surface, tol=tol, max_orders=max_orders)
        if raise_on_error:
            _raise_status(r.status, int(nb_angles))
        return r
    if devices is not None and len(devices) == 1:
        device = int(devices[0])
    if azimuths is not None and mode_batch:
        # the handle that serves the mode-0 solve below is the one that takes the batch of c x B columns: made wide enough here
        cols = _broadcast_columns(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer)
        c_cap = _mode_chunk_cap(cols[0].shape[0], int(nb_layers), int(nb_angles), M, mode_chunk)
        get_solver(int(nb_layers), int(nb_angles), c_cap * cols[0].shape[0], max_orders, device)
    s, tau, P0a, P0r, mu, iu, idn, N = _prepare_batch(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, z0, z_up, z_down,
                                                      nb_layers, nb_angles, atm_phase_fun, g_atm, aer_phase_fun, g_aer, mie_atm,
                                                      mie_aer, P_atm, P_aer, P0_atm, P0_aer, surface, max_orders, device,
                                                      aer_set=aer_set, delta_m=dm, gas=gas)
    if dm is not None:
        aer_phase_fun, g_aer, mie_aer = dm.phase             # what the view stages resolve: the truncated table
    sigma = None
    bx = {}
    try:
        if gas is not None:
            mu0v = np.broadcast_to(np.asarray(mu0, dtype=np.float64), (tau.shape[0],))
            gv = {}

            def gas_views(dev, d_tau, d_I, d_sigma, B):
                # the view stage on the resident field, while the weights are set
                gv["first"], gv["scat"] = view_radiance(s, d_tau, d_I, mu0v, vmu, vlev, vquad, atm_phase_fun, g_atm, mie_atm,
                                                        aer_phase_fun, g_aer, mie_aer, device, thermal=thermal, sigma=d_sigma,
                                                        profile=True, dev=dev)
            r, sigma, _ = solve_profile(s, tau, P0a, P0r, gas.w, mu0v,
                                        np.linspace(z0, 0, int(nb_layers)) if spherical else None, earth_radius, thermal, tol, device,
                                        post=gas_views if view_mu is not None else None)
        elif spherical:
            r, sigma, _ = solve_spherical(s, tau, P0a, P0r, np.linspace(z0, 0, int(nb_layers)), earth_radius, tol, save_orders, device)
        elif ground:
            r, bx, _ = solve_brdf(s, tau, P0a, P0r, ground, mu0, tol, max_bounces, device=device,
                                  view=(vmu, vlev) if ground.view else None)
        elif thermal:
            r, _ = solve_thermal(s, tau, *thermal, tol=tol, save_orders=save_orders, device=device)
        else:
            s.set_first_order(first_order)
            r = s.solve(tau, P0a, P0r, tol=tol, save_orders=save_orders)
    finally:
        if not spherical and not thermal:
            s.set_first_order("coded")                       # (the solver is cached)
        if aer_set is not None:
            _columns_to_set0(s, tau.shape[0])
    if raise_on_error:
        _raise_status(r.status, N)
    out = BatchResult(I=r.I, n=r.n, status=r.status, tau=tau, mu=mu, idx_up=iu, idx_down=idn, I_saved=r.I_saved, beam_slant=sigma,
                      bounces=bx.get("bounces"), bounce_ratio=bx.get("bounce_ratio"), bounce_orders=bx.get("bounce_orders"),
                      black_sky_albedo=bx.get("black_sky_albedo"), white_sky_albedo=bx.get("white_sky_albedo"))
    if dm is not None:
        out.delta_m_f, out.tauStar_aer_scaled, out.alb_aer_scaled = dm.f, dm.tauStar_aer, dm.alb_aer
    if gas is not None:
        out.gas_tau, out.row_weight = gas.gas_tau, gas.w
    if azimuths is not None:
        mu0v =np.broadcast_to(np.atleast_1d(np.asarray(mu0, dtype=np.float64)), (tau.shape[0],))
        if mode_batch:
            L_ = tau.shape[1]
            colargs = (np.full(tau.shape[0], iu), np.full(tau.shape[0], idn), cols[0], cols[2], cols[4], cols[5], cols[3] / L_,
                       cols[1] / (idn + 1 - iu), cols[3] + cols[1])
            out.I_azimuth, out.mode_status = azimuth_modes_batched(s, tau, r, colargs, azimuths, M, nphi, lev, atm_phase_fun, g_atm,
                                                                   mie_atm, aer_phase_fun, g_aer, mie_aer, c_cap, device)
        else:
            out.I_azimuth, out.mode_status = azimuth_modes(s, tau, r, mu0v, azimuths, M, nphi, lev, atm_phase_fun, g_atm, mie_atm,
                                                           aer_phase_fun, g_aer, mie_aer, device, ground=ground,
                                                           bounce_orders=bx.get("bounce_orders"), sigma=sigma)
        if raise_on_error:
            _raise_status(out.mode_status, N)
    if view_mu is not None:
        mu0v = np.broadcast_to(np.atleast_1d(np.asarray(mu0, dtype=np.float64)), (tau.shape[0],))
        out.view_mu_signed = np.concatenate((-vmu, vmu))
        if gas is not None:
            out.I_view_first, out.I_view_scattered = gv["first"], gv["scat"]
        else:
            out.I_view_first, out.I_view_scattered = view_radiance(s, tau, r.I, mu0v, vmu, vlev, vquad, atm_phase_fun, g_atm,
                                                                   mie_atm, aer_phase_fun, g_aer, mie_aer, device, thermal=thermal,
                                                                   sigma=sigma)
        out.I_view = out.I_view_first + out.I_view_scattered
        if ground:
            out.I_view_ground = bx["I_view_ground"]
            out.I_view = out.I_view + out.I_view_ground
        if view_azimuths is not None:
            out.I_view_azimuth_first, out.I_view_azimuth_scattered, out.I_view_azimuth_ground, out.view_mode_status = view_azimuth_modes(
                s, tau, r, mu0v, vmu, vlev, vquad, vphi, vM, vnphi, view_first_order, out.I_view_first, out.I_view_scattered,
                atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer, mie_aer, device, ground=ground,
                bounce_orders=bx.get("bounce_orders"),
                ground0=bx.get("I_view_ground" if view_first_order == "modes" else "I_view_ground_diffuse"), sigma=sigma, tms=dm)
            out.I_view_azimuth = out.I_view_azimuth_first + out.I_view_azimuth_scattered
            if ground:
                out.I_view_azimuth = out.I_view_azimuth + out.I_view_azimuth_ground
            if raise_on_error:
                _raise_status(out.view_mode_status, N)
    return out


def _mode_counts(n_modes, nphi_modes):
    """(M, nphi) of a call that sums Fourier modes: n_modes (default 16) and the azimuth nodes its modes are built on."""
    M = 16 if n_modes is None else int(n_modes)
    if not 1 <= M <= _lib.MAX_MODES:
        raise ValueError("n_modes must be in 1..%d (got %d)" % (_lib.MAX_MODES, M))
    nphi = max(25, 2 * M + 1) if nphi_modes is None else int(nphi_modes)
    if M > nphi - 2:
        raise ValueError("n_modes = %d needs nphi_modes >= %d (got %d)" % (M, M + 2, nphi))
    return M, nphi


def _level_rows(levels, nb_layers, keyword):
    """The rows of the keyword `keyword` (`levels` / `view_levels`) as indices from the top: negative ones count from the ground."""
    L = int(nb_layers)
    lev = [int(x) for x in np.atleast_1d(levels)]
    if not lev or any(not -L <= x < L for x in lev):
        raise ValueError("%s must be row indices in [-%d, %d)" % (keyword, L, L))
    return [x + L if x < 0 else x for x in lev]


def _angle_array(angles, keyword):
    """The azimuths of the keyword `keyword` (`azimuths` / `view_azimuths`) as a float64 array."""
    phi = np.asarray(angles, dtype=np.float64)
    if phi.ndim != 1 or phi.size == 0 or not np.all(np.isfinite(phi)):
        raise ValueError("%s must be a non-empty 1-d array of finite angles (radians)" % keyword)
    return phi


def _view_args(view_mu, view_levels, view_quadrature, nb_layers, P_atm, P_aer, P0_atm, P0_aer, surface, devices, first_order,
               azimuths, aer_set, atm_phase_fun, aer_phase_fun):
    """Checks of the view-radiance call, made before any handle exists: (view_mu [V], levels as row indices, quadrature)."""
    if azimuths is not None:
        raise ValueError("view_mu is not available with azimuths (the grid's azimuth synthesis); the radiance at a view cosine "
                         "and an azimuth is view_azimuths=[...]")
    if aer_set is not None or isinstance(aer_phase_fun, (list, tuple)):
        raise ValueError("view_mu is not available with aer_set (the view stage reads one aerosol phase function)")
    if devices is not None and len(devices) > 1:
        raise ValueError("view_mu is not available with devices=[...]")
    if any(x is not None for x in (P_atm, P_aer, P0_atm, P0_aer)):
        raise ValueError("view_mu needs named phase functions: rows at view cosines cannot be derived from arrays on the grid")
    if surface != "specular":
        raise ValueError("view_mu is available with the specular surface only (the Lambertian boundary of the orders n >= 2 "
                         "needs the grid's surface row of every order)")
    if first_order != "coded":
        raise ValueError("view_mu is available with first_order='coded' only")
    if view_quadrature not in ("grid", "linear"):
        raise ValueError("view_quadrature must be 'grid' or 'linear' (got %r)" % (view_quadrature,))
    vmu = np.array(np.atleast_1d(view_mu), dtype=np.float64)
    if vmu.ndim != 1 or not 1 <= vmu.size <= _lib.MAX_VIEWS:
        raise ValueError("view_mu must hold 1..%d cosines" % _lib.MAX_VIEWS)
    if not np.all(np.isfinite(vmu)) or np.any(vmu < 0.01) or np.any(vmu > 1):
        raise ValueError("view_mu must be finite cosines in [0.01, 1]")
    return vmu, _level_rows(view_levels, nb_layers, "view_levels"), view_quadrature


def _view_azimuth_args(view_azimuths, view_first_order, view_mu, azimuths, n_modes, nphi_modes, mode_batch, mode_chunk):
    """Checks of the azimuth-resolved view call, made before any handle exists (what `view_mu` refuses, `_view_args` refuses
    next): (azimuths [n], M, nphi)."""
    if view_first_order not in ("exact", "modes"):
        raise ValueError("view_first_order must be 'exact' or 'modes' (got %r)" % (view_first_order,))
    if view_azimuths is None:
        raise ValueError("view_first_order belongs to the azimuth-resolved view call: give view_azimuths")
    if view_mu is None:
        raise ValueError("view_azimuths are the azimuths of the view cosines: give view_mu")
    if azimuths is not None:
        raise ValueError("view_azimuths are not available with azimuths (one mode loop serves one of them)")
    if mode_batch or mode_chunk is not None:
        raise ValueError("view_azimuths are not available with mode_batch / mode_chunk (the view stage reads one mode's resident field)")
    return (_angle_array(view_azimuths, "view_azimuths"),) + _mode_counts(n_modes, nphi_modes)


def view_rows(s: Solver, view_mu, d_mu0, atm, aer, dev):
    """The rows of both phase functions at the signed view lanes, built on handle `s` (grid set, on torch's stream of `dev`):
    ([rows_atm, rows_aer] each [2V, 2N], [p0rows_atm, p0rows_aer] each [B, 2V] for the suns `d_mu0` [B], a tensor on `dev`).
    `atm`, `aer`: (name, g, mie).  They depend on the view cosines, the phase names and the suns only, so a driver that runs the
    view stage chunk by chunk builds them once (`view_radiance(rows=...)`)."""
    import torch
    B, V2 = d_mu0.shape[0], 2 * len(view_mu)
    sgn = np.concatenate((-view_mu, view_mu))
    rows, p0rows = [], []
    for phase in (atm, aer):
        kind, g = _phase_kind(s, *phase)
        rw = torch.empty((V2, s.D), dtype=torch.float64, device=dev)
        p0 = torch.empty((B, V2), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        s.phase_rows_device(kind, sgn, rw.data_ptr(), g)
        s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p0.data_ptr(), B, g)
        rows.append(rw)
        p0rows.append(p0)
    return rows, p0rows


def view_radiance(s: Solver, tau, I, mu0, view_mu, levels, quadrature, atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer,
                  mie_aer, device=0, thermal=None, sigma=None, profile=False, dev=None, keep_device=False, rows=None):
    """The view stage on the field `I` [B, L, 2N] of handle `s` (whose columns are set): rows of both phase functions at the
    signed lanes, then `Solver.view_radiance_device` with I_src = I.  Returns (first order, scattered), each [B, nlev, 2V].
    `thermal` = (planck [B, L], planck_surface [B], emissivity [B] or None): I is a thermal field, and the first term is the
    emission at the view lanes (`Solver.emission_view_device`) instead of the solar first order.  `sigma` [B, L] (the
    `beam_slant` of `solve_spherical`): the first term is the first order on that beam path at the view lanes
    (`Solver.view_first_order_beam_device`) instead of the plane closed form.  `profile=True`: the handle
    carries per-level weights, and the stage runs on the three weighted entries (`Solver.view_radiance_profile_device`,
    `view_first_order_profile_device`, `emission_view_profile_device`); the first term is always explicit, on `sigma` or, where
    none is given, on the plane beam sigma = tau / mu0 -- no closed form is used under weights.  `dev`: the caller is inside a
    stream scope of its own on that torch device (the `post` of `solve_profile`), and tau, I and sigma are tensors there.
    `keep_device=True`: both terms come back as torch tensors on that device, nothing crosses PCIe, and the sources in `thermal`
    may be tensors there too.  `rows`: what `view_rows` returned for at least these B columns' suns, instead of building them."""
    import torch
    B, L = tau.shape
    V2 = 2 * len(view_mu)
    with (_on_torch_stream(s, device) if dev is None else nullcontext(dev)) as dev:
        # (a copy: broadcast inputs are read-only; a tensor is used where it lies)
        up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)
        # (the field is large and already contiguous: uploaded from where it lies, not through a host copy)
        d_tau = tau if isinstance(tau, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tau)).to(dev)
        d_I = I if isinstance(I, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(I)).to(dev)
        d_mu0 = up(mu0)
        if rows is None:
            rows, p0rows = view_rows(s, view_mu, d_mu0, (atm_phase_fun, g_atm, mie_atm), (aer_phase_fun, g_aer, mie_aer), dev)
        else:
            rows, p0rows = rows[0], [p[:B] for p in rows[1]]
        d_scat = torch.empty((B, len(levels), V2), dtype=torch.float64, device=dev)
        d_first = torch.empty((B, len(levels), V2), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        first, p0_atm, p0_aer = d_first.data_ptr(), p0rows[0].data_ptr(), p0rows[1].data_ptr()
        if profile:
            if thermal is not None:
                d_pl, d_bs = up(thermal[0]), up(thermal[1])
                d_es = None if thermal[2] is None else up(thermal[2])
                s.emission_view_profile_device(view_mu, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), levels, first,
                                               0 if d_es is None else d_es.data_ptr(), B=B)
            else:
                d_sig = d_tau / d_mu0[:, None] if sigma is None else sigma if isinstance(sigma, torch.Tensor) else up(sigma)
                s.view_first_order_profile_device(view_mu, d_tau.data_ptr(), d_sig.data_ptr(), p0_atm, p0_aer, levels, first, B=B)
            s.view_radiance_profile_device(view_mu, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), levels,
                                           d_scat.data_ptr(), quadrature=quadrature, B=B)
            s.synchronize()
            return (d_first, d_scat) if keep_device else (d_first.cpu().numpy(), d_scat.cpu().numpy())
        if thermal is not None:
            # the first term is the emission at the lanes: the view stage gets no first-order addresses and leaves it alone
            d_pl, d_bs = up(thermal[0]), up(thermal[1])
            d_es = None if thermal[2] is None else up(thermal[2])
            s.emission_view_device(view_mu, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), levels, first,
                                   0 if d_es is None else d_es.data_ptr(), B=B)
            first = p0_atm = p0_aer = 0
        elif sigma is not None:
            # likewise: the first order on the slant path is this stage's own
            d_sig = up(sigma)
            s.view_first_order_beam_device(view_mu, d_tau.data_ptr(), d_sig.data_ptr(), p0_atm, p0_aer, levels, first, B=B)
            first = p0_atm = p0_aer = 0
        s.view_radiance_device(view_mu, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), levels,
                               d_scat_out=d_scat.data_ptr(), d_first_out=first, d_p0rows_atm=p0_atm, d_p0rows_aer=p0_aer,
                               quadrature=quadrature, B=B)
        s.synchronize()
        return (d_first, d_scat) if keep_device else (d_first.cpu().numpy(), d_scat.cpu().numpy())


def _columns_to_set0(s, B):
    """A cached handle's columns back on aerosol set 0, from a `finally`: an error here must not hide the one in flight."""
    try:
        s.set_aerosol_sets(np.zeros(B, dtype=np.int32))
    except Exception:
        pass


def _same_aerosol(a, b):
    """Two (name, g, mie dict or None) specifications name the same aerosol (values may be NumPy scalars or arrays)."""
    if a[0] != b[0] or not np.array_equal(a[1], b[1]) or (a[2] is None) != (b[2] is None):
        return False
    return a[2] is None or (set(a[2]) == set(b[2]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2]))


def _spectrum_args(wavelengths, tauStar_aer, angstrom, lambda_ref, aer, alb_aer, tauStar_atm_ref):
    """Checks of `SOS_Aer_spectrum`, made before any handle exists: (wl [W], tauStar_aer [W], tauStar_atm [W], m [W], r_m [W],
    sig [W])."""
    wl = np.atleast_1d(np.asarray(wavelengths, dtype=np.float64))
    if wl.ndim != 1 or wl.size == 0 or not np.all(np.isfinite(wl)) or np.any(wl <= 0):
        raise ValueError("wavelengths must be a non-empty 1-d array of positive numbers (micrometres)")
    if not (np.isfinite(lambda_ref) and lambda_ref > 0):
        raise ValueError("lambda_ref must be positive")
    if not isinstance(aer, dict) or set(aer) - {"m", "r_m", "sig"} or set(("m", "r_m", "sig")) - set(aer):
        raise ValueError("aer must be dict(m=, r_m=, sig=): refractive index (scalar or one per wavelength), median radius and "
                         "geometric standard deviation of the log-normal ensemble")
    if not (alb_aer == "mie" or np.ndim(alb_aer) == 0 or np.shape(alb_aer) == wl.shape):
        raise ValueError("alb_aer must be 'mie' (the ensemble's single-scattering albedo), a number or one number per wavelength")
    if callable(tauStar_aer):
        if angstrom is not None:
            raise ValueError("give tauStar_aer as a function of the wavelength or an Angstrom exponent, not both")
        t_aer = np.array([float(tauStar_aer(w)) for w in wl])
    elif angstrom is not None:
        if np.ndim(tauStar_aer) != 0:
            raise ValueError("with an Angstrom exponent tauStar_aer is the optical depth at lambda_ref (a scalar)")
        t_aer = float(tauStar_aer) * (wl / lambda_ref) ** (-float(angstrom))
    else:
        t_aer = np.asarray(tauStar_aer, dtype=np.float64)
        if t_aer.ndim != 0 and t_aer.shape != wl.shape:
            raise ValueError("tauStar_aer must be a scalar, one value per wavelength or a function of the wavelength")
        t_aer = np.broadcast_to(t_aer, wl.shape).copy()
    if np.any(t_aer < 0) or not np.all(np.isfinite(t_aer)):
        raise ValueError("tauStar_aer must be finite and >= 0")
    t_atm = float(tauStar_atm_ref) * (lambda_ref / wl) ** 4
    try:
        m, r_m, sig = (np.broadcast_to(np.asarray(aer[k]), wl.shape) for k in ("m", "r_m", "sig"))
    except ValueError:
        raise ValueError("aer: m, r_m and sig must be scalars or one value per wavelength") from None
    return wl, t_aer, t_atm, m.astype(complex), r_m.astype(np.float64), sig.astype(np.float64)


def SOS_Aer_spectrum(wavelengths, mu0, tauStar_aer, grd_alb, aer, *, angstrom=None, lambda_ref=0.550, tauStar_atm_ref=0.124,
                     alb_aer="mie", alb_atm=1.0, nb_radius=100, r_min=0.01, r_max=10.0, ntab=6001, indx_convention="absorbing",
                     atm_phase_fun="rayleigh", g_atm=0.0, nb_layers=200, nb_angles=128, max_orders=256, device=0,
                     one_batch=False, **batch_kw):
    """A spectrum of batches: for every wavelength (micrometres) the columns (mu0, grd_alb) of `SOS_Aer_batch` with a log-normal
    Mie aerosol `aer` = dict(m=, r_m=, sig=) (each a scalar or one value per wavelength).  The molecular optical depth is
    tauStar_atm_ref (lambda_ref / wl)^4; the aerosol's is `tauStar_aer`: a function of the wavelength, one value per wavelength,
    a constant, or -- with `angstrom` -- its value at lambda_ref scaled by (wl / lambda_ref)^-angstrom.  `alb_aer='mie'`
    (default) takes every ensemble's own single-scattering albedo.  All ensembles are tabulated in ONE call of the device's
    Mie kernels (`Solver.mie_ensembles_device`); per wavelength the table is handed to the azimuth builders on the device
    (`Solver.set_phase_table_dev`) and the columns go through `SOS_Aer_batch` (further keywords are passed on).
    `one_batch=True`: all W x C columns in ONE solve, the wavelength as the aerosol set of its columns (at most 64 wavelengths;
    `Solver.set_phase_sets`), instead of W small solves in the latency regime; the same list of results, column for column the
    bits of the loop while both take the single pass.  The matrices stay on the device: `Solver.phase_matrix_device` writes
    them where `Solver.set_phase_sets_device` folds them.
    `beam='spherical'` and `earth_radius` are passed on like every further keyword: each wavelength's batch is then solved with
    the pseudo-spherical direct beam, and its BatchResult carries `beam_slant`.  `delta_m` is refused: the batches take their
    aerosol as arrays.
    Returns (list of BatchResult, one per wavelength; bulk [W, 3]: albedo, asymmetry parameter, mean extinction cross-section)."""
    import torch
    from . import mie as _mie
    wl, t_aer, t_atm, m, r_m, sig = _spectrum_args(wavelengths, tauStar_aer, angstrom, lambda_ref, aer, alb_aer, tauStar_atm_ref)
    _beam_args(batch_kw.get("beam", "plane"), batch_kw.get("earth_radius", EARTH_RADIUS_KM), view_mu=batch_kw.get("view_mu"),
               view_azimuths=batch_kw.get("view_azimuths"), first_order=batch_kw.get("first_order", "coded"),
               beam_stages=batch_kw.get("beam_stages", False))
    for k in ("P_aer", "P0_aer", "aer_phase_fun", "mie_aer", "tauStar_atm", "devices", "azimuths"):
        if k in batch_kw:
            raise ValueError("SOS_Aer_spectrum sets %s itself" % k)
    if batch_kw.get("delta_m") is not None:
        raise ValueError("delta_m is not available with SOS_Aer_spectrum: it hands P_aer / P0_aer arrays to every batch; call "
                         "SOS_Aer_batch(delta_m=...) per wavelength")
    if batch_kw.get("gas_tau") is not None:
        raise ValueError("gas_tau is not available with SOS_Aer_spectrum yet: a gas profile belongs to one wavelength; call "
                         "SOS_Aer_batch(gas_tau=...) per wavelength, or bands.band_solar(gas_tau=[K, L])")
    m = np.array([_mie.refractive_index(v, indx_convention) for v in m])
    mu0v, _ = np.broadcast_arrays(np.atleast_1d(np.asarray(mu0, dtype=np.float64)), np.atleast_1d(np.asarray(grd_alb, dtype=np.float64)))
    L, N, W = int(nb_layers), int(nb_angles), wl.size
    C = mu0v.shape[0]
    if one_batch and W > _lib.MAX_PHASE_SETS:
        raise ValueError("one_batch=True takes at most %d wavelengths (got %d)" % (_lib.MAX_PHASE_SETS, W))
    s = get_solver(L, N, W * C if one_batch else C, max_orders, device)
    mu = direction_grid(N)
    if not s.same_grid(mu):
        s.set_grid(mu)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_p = torch.empty((W, int(ntab)), dtype=torch.float64, device=dev)
        d_bulk = torch.empty((W, 3), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        s.mie_ensembles_device(d_p.data_ptr(), d_bulk.data_ptr(), wl, m, r_m, sig, nb_radius, r_min, r_max, ntab)
        s.synchronize()
        bulk = d_bulk.cpu().numpy()
        omega = bulk[:, 0] if isinstance(alb_aer, str) else np.broadcast_to(np.asarray(alb_aer, dtype=np.float64), wl.shape)
        if one_batch:
            P0r = np.empty((W, C, 2 * N))
            d_P = torch.empty((W, 2 * N, 2 * N), dtype=torch.float64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            for w in range(W):
                s.set_phase_table_dev(d_p[w].data_ptr(), int(ntab))
                s.phase_matrix_device("table", d_P[w].data_ptr())
                P0r[w] = s.phase_p0("table", mu0v)
            P_sets = DevicePhaseSets(d_P.data_ptr(), W, keep=d_P)
            rep_w = lambda v: np.repeat(np.asarray(v, dtype=np.float64), C)
            tile_c = lambda v: np.tile(np.broadcast_to(np.atleast_1d(np.asarray(v, dtype=np.float64)), (C,)), W)
            r = SOS_Aer_batch(tile_c(mu0), rep_w(t_aer), tile_c(grd_alb), tauStar_atm=rep_w(t_atm), alb_atm=alb_atm,
                              alb_aer=rep_w(omega), nb_layers=L, nb_angles=N, atm_phase_fun=atm_phase_fun, g_atm=g_atm,
                              P_aer=P_sets, P0_aer=P0r.reshape(W * C, 2 * N), aer_set=np.repeat(np.arange(W, dtype=np.int32), C),
                              max_orders=max_orders, device=device, **batch_kw)
            cut = lambda a, w: None if a is None else a[w * C:(w + 1) * C]
            return [BatchResult(I=cut(r.I, w), n=cut(r.n, w), status=cut(r.status, w), tau=cut(r.tau, w), mu=r.mu, idx_up=r.idx_up,
                                idx_down=r.idx_down, I_saved=cut(r.I_saved, w), beam_slant=cut(r.beam_slant, w))
                    for w in range(W)], bulk
        out = []
        for w in range(W):
            s.set_phase_table_dev(d_p[w].data_ptr(), int(ntab))
            P0r, P_aer = s.phase_p0("table", mu0v), s.phase_matrix("table")
            out.append(SOS_Aer_batch(mu0, t_aer[w], grd_alb, tauStar_atm=t_atm[w], alb_atm=alb_atm, alb_aer=omega[w],
                                     nb_layers=L, nb_angles=N, atm_phase_fun=atm_phase_fun, g_atm=g_atm, P_aer=P_aer, P0_aer=P0r,
                                     max_orders=max_orders, device=device, **batch_kw))
    return out, bulk


def _azimuth_args(azimuths, n_modes, nphi_modes, levels, nb_layers, P_atm, P_aer, P0_atm, P0_aer, surface, devices, first_order,
                  mode_batch=False, mode_chunk=None):
    """Checks of the azimuth-resolved call, made before any handle exists: (M, nphi, levels as row indices)."""
    if not isinstance(mode_batch, (bool, np.bool_)):
        raise ValueError("mode_batch must be True or False (got %r)" % (mode_batch,))
    if mode_chunk is not None:
        if not mode_batch:
            raise ValueError("mode_chunk is the chunk of mode_batch=True")
        if isinstance(mode_chunk, (bool, np.bool_)) or not isinstance(mode_chunk, (int, np.integer)) or not 1 <= mode_chunk <= _lib.MAX_PHASE_SETS:
            raise ValueError("mode_chunk must be an integer in 1..%d (got %r)" % (_lib.MAX_PHASE_SETS, mode_chunk))
    if any(x is not None for x in (P_atm, P_aer, P0_atm, P0_aer)):
        raise ValueError("azimuths need named phase functions: the Fourier modes cannot be derived from azimuth-averaged arrays")
    if surface != "specular" or first_order != "coded":
        raise ValueError("azimuths are available with the specular surface only (the Lambertian terms of modes m >= 1 are not built)")
    if devices is not None and len(devices) > 1:
        raise ValueError("azimuths are not available with devices=[...]")
    _angle_array(azimuths, "azimuths")
    return _mode_counts(n_modes, nphi_modes) + (_level_rows(levels, nb_layers, "levels"),)


@dataclass
class _ModeLoop:
    """What `begin`, `step` and `finish` of `_solve_modes` see.  The loop fills the fields below; a driver keeps buffers of its
    own under `own`."""
    dev: object              # torch device of the handle
    B: int
    L: int
    D: int
    M: int
    nphi: int
    phases: tuple            # ((name, g, mie) of the atmosphere, of the aerosol): what `_phase_kind` takes before a builder
    d_tau: object = None     # [B, L]
    d_mu0: object = None     # [B]
    d_Im: object = None      # [B, L, 2N]: set by `begin` to the mode-0 field; after the solve of mode m, the field of mode m
    d_target: object = None  # [B] int32: the order counts of mode 0, the handle's targets while the modes are solved
    d_status: object = None  # [M, B] int32: the status of the solve of mode m in row m - 1 (set before the first mode)
    d_sigma: object = None   # [B, L]: the beam's slant path (beam='spherical' with beam_stages=True), else None
    own: SimpleNamespace = field(default_factory=SimpleNamespace)


def _beam_mode_first(s: Solver):
    """The per-mode first-order hook of `_solve_modes` for a beam path c.d_sigma: the first order of mode m
    layer by layer on that path from the mode's P0 vectors, into one buffer all modes reuse; its address is the `d_I1` of the
    mode's solve."""
    import torch
    own = {}

    def first(c, m, p0a, p0r):
        if "I1" not in own:
            own["I1"] = torch.empty((c.B, c.L, c.D), dtype=torch.float64, device=c.dev)
        s.first_order_beam_device(c.d_tau.data_ptr(), c.d_sigma.data_ptr(), p0a, p0r, own["I1"].data_ptr(), B=c.B)
        return own["I1"].data_ptr()
    return first


def _solve_modes(s: Solver, tau, r, mu0, M, nphi, phases, device, begin, step, finish, sigma=None, first=None):
    """The loop over the Fourier modes m = 1..M of the solve `r` (the mode-0 result of handle `s`, whose columns are set): per
    mode the matrices and first-order vectors of both phase functions `phases` = ((name, g, mie) of the atmosphere, of the
    aerosol), a solve with the order counts of mode 0 (sosrt_set_order_targets) into the resident c.d_Im, then `step(c, m)`.
    Every builder of the loop and of the steps resolves its phase function with `_phase_kind` (c.phases), which puts a
    Mie-derived function's table on the handle first: the handle holds one table at a time.  `begin(c)` runs
    before the modes are built and sets c.d_Im to the mode-0 field; `finish(c)` after the last mode, and its value is returned
    with the mode status [M + 1, B].  The handle's mode-0 phase matrices are put back and its targets cleared afterwards, also
    on error.  `sigma` [B, L]: a beam path, uploaded to c.d_sigma before `begin`.  `first(c, m, p0a, p0r)` (optional) -> the address
    of a first order [B, L, 2N] of mode m from the mode's P0 vectors (addresses): the mode's solve starts from it (`d_I1`) instead
    of the handle's own first order; without it the loop is the code as it was."""
    import torch
    B, L = tau.shape
    D = s.D
    P_mode0 = s._P
    status = np.zeros((M + 1, B), dtype=np.int32)
    status[0] = r.status
    try:
        with _on_torch_stream(s, device) as dev:
            c = _ModeLoop(dev=dev, B=B, L=L, D=D, M=M, nphi=nphi, phases=tuple(phases))
            c.d_tau = d_tau = torch.from_numpy(np.ascontiguousarray(tau)).to(dev)
            c.d_mu0 = d_mu0 = torch.from_numpy(np.array(mu0, dtype=np.float64)).to(dev)      # (a copy: broadcast views are read-only)
            c.d_target = d_target = torch.from_numpy(np.ascontiguousarray(r.n, dtype=np.int32)).to(dev)
            if sigma is not None:
                c.d_sigma = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)).to(dev)
            begin(c)
            # modes m >= 1 of both phase functions: the matrices to the host (one fold each in set_phase), the first-order
            # vectors where the solve reads them
            Pm, d_P0 = [], []
            for phase in c.phases:
                kind, g = _phase_kind(s, *phase)
                Pm.append(s.phase_modes(kind, 1, M, nphi, g))
                p0 = torch.empty((M, B, D), dtype=torch.float64, device=dev)
                s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p0.data_ptr(), B, 1, M, nphi, g)
                d_P0.append(p0)
            d_n = torch.zeros(B, dtype=torch.int32, device=dev)
            c.d_status = d_st = torch.zeros((M, B), dtype=torch.int32, device=dev)
            s.set_order_targets(d_target.data_ptr())
            for m in range(1, M + 1):
                s.synchronize()                              # (set_phase rewrites the matrices the previous mode's solve read)
                # the solve of mode m takes (-1)^m P^m: its contraction reads P[a][flip b], the stored matrix at phi + pi
                sgn = -1.0 if m & 1 else 1.0
                s.set_phase(sgn * Pm[0][m - 1], sgn * Pm[1][m - 1])
                if first is None:
                    s.solve_device(d_tau.data_ptr(), d_P0[0][m - 1].data_ptr(), d_P0[1][m - 1].data_ptr(), c.d_Im.data_ptr(),
                                   d_n_orders=d_n.data_ptr(), d_status=d_st[m - 1].data_ptr())
                else:
                    d_I1 = first(c, m, d_P0[0][m - 1].data_ptr(), d_P0[1][m - 1].data_ptr())
                    s.solve_device(d_tau.data_ptr(), d_P0[0][m - 1].data_ptr(), d_P0[1][m - 1].data_ptr(), c.d_Im.data_ptr(),
                                   d_I1=d_I1, d_n_orders=d_n.data_ptr(), d_status=d_st[m - 1].data_ptr())
                step(c, m)
            s.synchronize()
            status[1:] = d_st.cpu().numpy()
            result = finish(c)
    finally:
        s.set_order_targets(None)
        if P_mode0[0] is not None:
            s.set_phase(*P_mode0)
    return result, status


def _reflection_buffers(s: Solver, c: _ModeLoop, ground, bounce_orders, brdf_nphi):
    """What `_mode_reflections` reads, under c.own (called from a driver's `begin`): the operators (-1)^m R^m and beam rows r0^m of
    the modes 1..c.M of the named BRDF `ground` on `brdf_nphi` nodes, its scale (a ground of terms: the stacks [M, K, ...] and the
    weights), the reflections' order counts and the buffers."""
    import torch
    o, M1 = c.own, s.N - 1
    o.d_scale = _ground_scale(ground, c.dev)
    o.d_orders = torch.from_numpy(np.ascontiguousarray(bounce_orders, dtype=np.int32)).to(c.dev)
    # (a ground of terms: [M, K, ...], a mode's K operators contiguous; its isotropic term has no mode m >= 1 and stays +0)
    o.d_R = _per_term(ground, c.dev, (c.M, M1, M1), lambda kind, par, out: s.brdf_operator_modes_device(
        kind, out, 1, c.M, par, brdf_nphi, sign_odd=True), axis=1, skip_iso=True)
    o.d_r0 = _per_term(ground, c.dev, (c.M, c.B, M1), lambda kind, par, out: s.brdf_beam_modes_device(
        kind, c.d_mu0.data_ptr(), out, 1, c.M, par, brdf_nphi, B=c.B), axis=1, skip_iso=True)
    o.terms = len(ground.terms or ())
    o.buf = _reflection_scratch(s, c.dev, c.B, c.L)


def _mode_reflections(s: Solver, c: _ModeLoop, m, hook=None):
    """The reflections 1..K of mode m >= 1 on the resident field c.d_Im, which holds the mode's black solve and leaves as the sum
    (DESIGN section 21): `_reflect` with a solve of bounce_orders[k - 1] orders; the statuses join c.d_status[m - 1] and the targets
    go back to mode 0's.  `hook(k, src)` runs after the ground source of reflection k, `src` being the field it reflected."""
    o = c.own
    for k in range(1, o.d_orders.shape[0] + 1):
        s.set_order_targets(o.d_orders[k - 1].data_ptr())
        _reflect(s, c.B, k, c.d_tau, c.d_Im, o.d_R[m - 1], o.d_r0[m - 1], o.d_scale, o.buf, c.d_status[m - 1], hook, o.terms,
                 d_P0_atm=0, d_P0_aer=0)
    s.set_order_targets(c.d_target.data_ptr())


def azimuth_modes(s: Solver, tau, r, mu0, azimuths, M, nphi, levels, atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer,
                  mie_aer, device=0, ground=None, bounce_orders=None, brdf_nphi=BRDF_NPHI, sigma=None):
    """Modes m = 1..M of the solve `r` (the mode-0 result of handle `s`, whose columns are set): per mode the matrices and
    first-order vectors of both phase functions, a solve with the order counts of mode 0 (sosrt_set_order_targets), and the
    synthesis at `levels` (`_solve_modes` with the grid's synthesis as its step).  Returns (I_azimuth [B, nlev, 2N,
    len(azimuths)], mode status [M + 1, B]).  The handle's mode-0 phase matrices are put back and its targets cleared
    afterwards, also on error.

    `ground` (the namespace of `_brdf_args`, `r` then being the result of `solve_brdf` over it) with `bounce_orders` [K, B] of
    that solve: the BRDF GROUND'S MODES.  The operators (-1)^m R^m and beam rows r0^m of the modes 1..M are
    built once, on the `brdf_nphi` nodes of mode 0's; per mode, between its black solve and its synthesis, the reflections 1..K
    run on the resident field (`_mode_reflections`), each a solve of bounce_orders[k - 1] orders, and their statuses join the
    mode's.  A Lambertian ground has no mode m >= 1: no reflections are run for it.

    `sigma` [B, L] (the `beam_slant` of `solve_spherical`, `r` being its result): every mode's solve starts from the first order
    on that beam path (`_beam_mode_first`)."""
    import torch
    nlev = len(levels)
    bounce = ground is not None and ground.kind != "lambertian"

    def begin(c):
        o = c.own
        o.d_lev = torch.tensor(levels, dtype=torch.int32, device=c.dev)
        o.d_phi = torch.from_numpy(np.ascontiguousarray(azimuths, dtype=np.float64)).to(c.dev)
        o.d_out = torch.empty((c.B, nlev, c.D, o.d_phi.numel()), dtype=torch.float64, device=c.dev)
        c.d_Im = torch.from_numpy(np.ascontiguousarray(r.I)).to(c.dev)
        step(c, 0)
        if bounce:
            _reflection_buffers(s, c, ground, bounce_orders, brdf_nphi)

    def step(c, m):
        o = c.own
        if bounce and m >= 1:
            _mode_reflections(s, c, m)
        s.azimuth_accumulate_device(m, c.d_Im.data_ptr(), o.d_lev.data_ptr(), nlev, o.d_phi.data_ptr(), o.d_phi.numel(),
                                    o.d_out.data_ptr(), B=c.B)

    return _solve_modes(s, tau, r, mu0, M, nphi, ((atm_phase_fun, g_atm, mie_atm), (aer_phase_fun, g_aer, mie_aer)), device,
                        begin, step, lambda c: c.own.d_out.cpu().numpy(), sigma=sigma,
                        first=None if sigma is None else _beam_mode_first(s))


def view_azimuth_modes(s: Solver, tau, r, mu0, view_mu, levels, quadrature, azimuths, M, nphi, first_order, first0, scat0,
                       atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer, mie_aer, device=0, ground=None, bounce_orders=None,
                       ground0=None, brdf_nphi=BRDF_NPHI, sigma=None, tms=None):
    """The view stage per Fourier mode: mode 0 is (`first0`, `scat0`), the result of `view_radiance` on
    r.I; per mode m >= 1 `_solve_modes` leaves the field I^m resident, `Solver.view_radiance_device` runs on it with the rows
    (-1)^m rows^m and p0rows^m of both phase functions (built for all modes once, before the loop), and the synthesis adds
    2 cos(m phi) times the result at the view lanes.  first_order 'exact': the first order is one closed-form evaluation per
    azimuth from p(c(lane, mu0, phi)) / Z0, written, not accumulated; 'modes': the sum of the modes' first orders.  Returns
    (first [B, nlev, 2V, len(azimuths)], scattered (same shape), None, mode status [M + 1, B]).

    `ground` (the namespace of `_brdf_args`, a named BRDF; `r` the result of `solve_brdf` over it, `bounce_orders` [K, B] its
    reflections' counts): THE VIEW STAGE OVER THE BRDF GROUND.  Per mode the reflections of
    `_mode_reflections` run between the black solve and the view stage, which then reads the mode's summed field, and per
    reflection the ground's term at the view lanes is accumulated from the same source with (-1)^m R^m at the view cosines
    (`Solver.view_ground_device`).  `ground0` [B, nlev, 2V] is mode 0's ground term from `solve_brdf`: with first_order
    'exact' its diffuse part -- the beam's single reflection is then rho(mu_view, mu0, phi) at the azimuth itself, written once
    per azimuth, and the modes carry the diffuse part only -- with 'modes' the whole, and the modes add rho^m(mu_view, mu0).  A
    Lambertian ground has no mode m >= 1.  The third value is then the ground's term [B, nlev, 2V, len(azimuths)].

    `sigma` [B, L] (the `beam_slant` of `solve_spherical`; `r`, `first0` and `scat0` from it): THE SPHERE IN THE STAGE (DESIGN
    section 27).  Every mode's solve starts from the first order on that beam path, and the first order at the view lanes is
    `Solver.view_first_order_beam_device` on it: per mode with p0rows^m ('modes'), or ONE call with the azimuths as its sets
    ('exact'), which evaluates the lanes' geometry once.

    `tms` (the namespace of `_delta_m_args`; the aerosol of the call is its truncated table): THE TMS FIRST ORDER (DESIGN section
    28).  With first_order 'exact' the aerosol's point values are those of the exact function `tms.exact`, divided by 1 - tms.f,
    with the normaliser of the truncated table: exact / Z_exact from `Solver.phase_p0_rows_azimuth_device`, times Z_exact /
    Z_trunc from two calls of `Solver.p0_normaliser_device`.  Everything else is the stage on the truncated function."""
    import torch
    V2, nlev, nout = 2 * len(view_mu), len(levels), len(azimuths)
    sgn = np.concatenate((-view_mu, view_mu))
    modes_first = first_order == "modes"
    bounce = ground is not None and ground.kind != "lambertian"

    def begin(c):
        dev, B, o = c.dev, c.B, c.own
        c.d_Im = torch.from_numpy(np.ascontiguousarray(r.I)).to(dev)
        o.d_phi = torch.from_numpy(np.ascontiguousarray(azimuths, dtype=np.float64)).to(dev)
        o.rows, o.p0rows, o.p0exact = [], [], []
        # (the handle runs on torch's current stream here: the builders are ordered after the allocations and uploads)
        for i_phase, phase in enumerate(c.phases):
            kind, g = _phase_kind(s, *phase)
            rw = torch.empty((M, V2, c.D), dtype=torch.float64, device=dev)
            s.phase_rows_modes_device(kind, sgn, rw.data_ptr(), 1, M, nphi, g, sign_odd=True)
            o.rows.append(rw)
            if modes_first:
                p0 = torch.empty((M, B, V2), dtype=torch.float64, device=dev)
                s.phase_p0_rows_modes_device(kind, c.d_mu0.data_ptr(), sgn, p0.data_ptr(), B, 1, M, nphi, g)
                o.p0rows.append(p0)
            elif tms is not None and i_phase == 1:
                # the exact function's values with the truncated table's normaliser, over 1 - f (the handle holds one table at
                # a time: the truncated one's normaliser first, then the exact function's values and normaliser)
                d_Z = torch.empty((2, B), dtype=torch.float64, device=dev)
                s.p0_normaliser_device(kind, c.d_mu0.data_ptr(), d_Z[0].data_ptr(), B, g)
                kind, g = _phase_kind(s, *tms.exact)
                p0 = torch.empty((nout, B, V2), dtype=torch.float64, device=dev)
                s.phase_p0_rows_azimuth_device(kind, c.d_mu0.data_ptr(), sgn, o.d_phi.data_ptr(), nout, p0.data_ptr(), B, g)
                s.p0_normaliser_device(kind, c.d_mu0.data_ptr(), d_Z[1].data_ptr(), B, g)
                p0 *= (d_Z[1] / d_Z[0] / (1.0 - tms.f))[None, :, None]
                o.p0exact.append(p0)
            else:
                p0 = torch.empty((nout, B, V2), dtype=torch.float64, device=dev)
                s.phase_p0_rows_azimuth_device(kind, c.d_mu0.data_ptr(), sgn, o.d_phi.data_ptr(), nout, p0.data_ptr(), B, g)
                o.p0exact.append(p0)
        o.d_scat = torch.from_numpy(np.ascontiguousarray(scat0)).to(dev)
        o.d_first = torch.from_numpy(np.ascontiguousarray(first0)).to(dev)
        o.d_out_scat = torch.empty((B, nlev, V2, nout), dtype=torch.float64, device=dev)
        o.d_out_first = torch.empty((B, nlev, V2, nout), dtype=torch.float64, device=dev) if modes_first else None
        if ground is not None:
            o.d_gr = torch.from_numpy(np.ascontiguousarray(ground0)).to(dev)
            o.d_out_gr = torch.empty((B, nlev, V2, nout), dtype=torch.float64, device=dev)
            o.d_scale = _ground_scale(ground, dev)
            if not modes_first:
                # (a ground of terms: [nout, K, B, V], the terms' values at the azimuth, summed with the weights by the terms kernel)
                o.d_r0phi = _per_term(ground, dev, (nout, B, V2 // 2), lambda kind, par, out: s.brdf_view_beam_azimuth_device(
                    kind, c.d_mu0.data_ptr(), view_mu, o.d_phi.data_ptr(), nout, out, par, B=B), axis=1)
        if bounce:
            _reflection_buffers(s, c, ground, bounce_orders, brdf_nphi)
            o.d_Rv = _per_term(ground, dev, (M, s.N - 1, V2 // 2), lambda kind, par, out: s.brdf_view_rows_modes_device(
                kind, view_mu, out, 1, M, par, brdf_nphi, sign_odd=True), axis=1, skip_iso=True)
            if modes_first:
                o.d_r0v = _per_term(ground, dev, (M, B, V2 // 2), lambda kind, par, out: s.brdf_view_beam_modes_device(
                    kind, c.d_mu0.data_ptr(), view_mu, out, 1, M, par, brdf_nphi, B=B), axis=1, skip_iso=True)
        accumulate(c, 0)

    def accumulate(c, m):
        o = c.own
        s.view_azimuth_accumulate_device(m, o.d_scat.data_ptr(), nlev, V2, o.d_phi.data_ptr(), nout, o.d_out_scat.data_ptr(), B=c.B)
        if modes_first:
            s.view_azimuth_accumulate_device(m, o.d_first.data_ptr(), nlev, V2, o.d_phi.data_ptr(), nout, o.d_out_first.data_ptr(),
                                             B=c.B)
        if ground is not None and (m == 0 or bounce):
            s.view_azimuth_accumulate_device(m, o.d_gr.data_ptr(), nlev, V2, o.d_phi.data_ptr(), nout, o.d_out_gr.data_ptr(), B=c.B)

    def view_ground(c, m, k, src):
        # reflection k of mode m at the view lanes, from the source the ground source has just read; the beam's share only where
        # the modes carry it
        o = c.own
        _view_ground(s, ground, view_mu, c.d_tau.data_ptr(), levels, o.d_gr.data_ptr(), o.d_scale.data_ptr(), d_I=src.data_ptr(),
                     d_Rv=o.d_Rv[m - 1].data_ptr(), d_r0v=o.d_r0v[m - 1].data_ptr() if modes_first and k == 1 else 0,
                     accumulate=k > 1, B=c.B)

    def step(c, m):
        o = c.own
        if bounce:
            _mode_reflections(s, c, m, hook=lambda k, src: view_ground(c, m, k, src))
        plane_first = modes_first and sigma is None
        if modes_first and sigma is not None:
            s.view_first_order_beam_device(view_mu, c.d_tau.data_ptr(), c.d_sigma.data_ptr(), o.p0rows[0][m - 1].data_ptr(),
                                           o.p0rows[1][m - 1].data_ptr(), levels, o.d_first.data_ptr(), B=c.B)
        s.view_radiance_device(view_mu, c.d_tau.data_ptr(), c.d_Im.data_ptr(), o.rows[0][m - 1].data_ptr(),
                               o.rows[1][m - 1].data_ptr(), levels, d_scat_out=o.d_scat.data_ptr(),
                               d_first_out=o.d_first.data_ptr() if plane_first else 0,
                               d_p0rows_atm=o.p0rows[0][m - 1].data_ptr() if plane_first else 0,
                               d_p0rows_aer=o.p0rows[1][m - 1].data_ptr() if plane_first else 0, quadrature=quadrature, B=c.B)
        accumulate(c, m)

    def finish(c):
        o = c.own
        if modes_first:
            first = o.d_out_first.cpu().numpy()
        else:
            d_f = torch.empty((nout, c.B, nlev, V2), dtype=torch.float64, device=c.dev)
            if sigma is not None:
                # the azimuths as the sets of one call: a lane's geometry does not depend on the azimuth
                s.view_first_order_beam_device(view_mu, c.d_tau.data_ptr(), c.d_sigma.data_ptr(), o.p0exact[0].data_ptr(),
                                               o.p0exact[1].data_ptr(), levels, d_f.data_ptr(), nset=nout, B=c.B)
            else:
                for i in range(nout):
                    s.view_radiance_device(view_mu, c.d_tau.data_ptr(), 0, 0, 0, levels, d_first_out=d_f[i].data_ptr(),
                                           d_p0rows_atm=o.p0exact[0][i].data_ptr(), d_p0rows_aer=o.p0exact[1][i].data_ptr(),
                                           quadrature=quadrature, B=c.B)
            s.synchronize()
            first = d_f.permute(1, 2, 3, 0).contiguous().cpu().numpy()   # (the azimuth last, as the synthesis writes it)
        gr = None
        if ground is not None:
            if not modes_first:
                # the beam's single reflection at every azimuth itself, added to the synthesis of the diffuse part
                d_gb = torch.empty((nout, c.B, nlev, V2), dtype=torch.float64, device=c.dev)
                for i in range(nout):
                    _view_ground(s, ground, view_mu, c.d_tau.data_ptr(), levels, d_gb[i].data_ptr(), o.d_scale.data_ptr(),
                                 d_r0v=o.d_r0phi[i].data_ptr(), B=c.B)
                s.synchronize()
                o.d_out_gr += d_gb.permute(1, 2, 3, 0)
            gr = o.d_out_gr.cpu().numpy()
        return first, o.d_out_scat.cpu().numpy(), gr

    (first, scat, gr), status = _solve_modes(s, tau, r, mu0, M, nphi, ((atm_phase_fun, g_atm, mie_atm), (aer_phase_fun, g_aer, mie_aer)),
                                             device, begin, step, finish, sigma=sigma,
                                             first=None if sigma is None else _beam_mode_first(s))
    return first, scat, gr, status


# mode_batch=True: a chunk of c modes is a batch of c x B columns, and every field buffer of the handle (and the chunk's share of
# the driver's) holds c B L 2N doubles.  The chunk is cut so that one such buffer stays within MODE_BATCH_FIELD_BYTES (2621
# columns at L = 200, N = 128).  The chunk does not bound the whole call: the one synthesis launch at the end reads the fields of
# ALL modes, so the driver holds M B L 2N doubles whatever c is (the loop holds one mode's) -- 3.4 GB for M = 16 modes of 512
# columns at L = 200, N = 128.  A call whose modes exceed MODE_BATCH_MODES_BYTES is refused.
MODE_BATCH_FIELD_BYTES = 1 << 30
MODE_BATCH_MODES_BYTES = 16 << 30


def _mode_chunk_cap(B, L, N, M, mode_chunk):
    """Modes per chunk by the size of the field and the number of phase sets (the combined-matrix cache is asked later, of the
    handle): the forced `mode_chunk`, or min(M, 64, what MODE_BATCH_FIELD_BYTES holds).  Refuses a call whose M fields
    [B, L, 2N], which the driver keeps for the one synthesis launch whatever the chunk, exceed MODE_BATCH_MODES_BYTES."""
    field = B * L * 2 * N * 8
    if M * field > MODE_BATCH_MODES_BYTES:
        raise ValueError("mode_batch=True keeps the fields of all %d modes of these %d columns for the synthesis: %d bytes, more than "
                         "MODE_BATCH_MODES_BYTES = %d; mode_batch=False works" % (M, B, M * field, MODE_BATCH_MODES_BYTES))
    if mode_chunk is not None:
        return int(mode_chunk)
    c = min(M, _lib.MAX_PHASE_SETS, MODE_BATCH_FIELD_BYTES // field)
    if c < 1:
        raise ValueError("mode_batch=True: one mode of these %d columns is a field of %d bytes, more than MODE_BATCH_FIELD_BYTES = %d; "
                         "mode_batch=False works" % (B, field, MODE_BATCH_FIELD_BYTES))
    return int(c)


def azimuth_modes_batched(s: Solver, tau, r, colargs, azimuths, M, nphi, levels, atm_phase_fun, g_atm, mie_atm, aer_phase_fun,
                          g_aer, mie_aer, c_cap, device=0):
    """`azimuth_modes` with the modes solved as batches: a chunk of c modes is ONE solve of c x B columns with column index
    (m, b) -- mode m as the atmosphere set and the aerosol set of its B columns (Solver.set_atm_phase_sets /
    set_phase_sets_device), P0 rows from the mode builder's [m][B][2N] layout, tau, the column scalars `colargs` (the arguments
    of `Solver.set_columns` for the B columns) and the order targets r.n tiled -- and one launch sums all modes.  Same return
    value, same bits.  c = min(c_cap, cache of combined matrices // distinct slab coefficient pairs of the B columns).  The
    handle's columns, mode-0 matrices and targets are put back afterwards, also on error."""
    import torch
    B, L = tau.shape
    D = s.D
    P_mode0 = s._P
    status = np.zeros((M + 1, B), dtype=np.int32)
    status[0] = r.status
    # distinct (ca, cr) of the columns' slabs, as the handle will count them per phase set (spec:321)
    da, dr = colargs[6], colargs[7]
    pairs = len({((wa / 4) * (a / (a + b)), (wr / 4) * (b / (a + b))) for wa, wr, a, b in zip(colargs[4], colargs[5], da, dr)})
    cache = s.phase_sets_info()["group_cap"]
    c = min(c_cap, cache // pairs, s.max_batch // B)
    if c < 1:
        raise ValueError("mode_batch=True: the %d distinct slab coefficient pairs of these columns do not fit the cache of %d combined "
                         "matrices even for one mode; mode_batch=False works" % (pairs, cache))
    tile = lambda v, k: np.tile(np.asarray(v), k)
    try:
        with _on_torch_stream(s, device) as dev:
            d_tau = torch.from_numpy(np.ascontiguousarray(tau)).to(dev)
            d_mu0 = torch.from_numpy(np.array(colargs[2], dtype=np.float64)).to(dev)      # (a copy: broadcast views are read-only)
            d_target = torch.from_numpy(np.ascontiguousarray(r.n, dtype=np.int32)).to(dev)
            d_lev = torch.tensor(levels, dtype=torch.int32, device=dev)
            d_phi = torch.from_numpy(np.ascontiguousarray(azimuths, dtype=np.float64)).to(dev)
            nlev, nout = len(levels), d_phi.numel()
            d_out = torch.empty((B, nlev, D, nout), dtype=torch.float64, device=dev)
            d_I0 = torch.from_numpy(np.ascontiguousarray(r.I)).to(dev)
            d_Im = torch.empty((M, B, L, D), dtype=torch.float64, device=dev)
            # modes 1..M: the atmosphere's matrices to the host (their low-rank factorisation is host code), the aerosol's stay on
            # the device, both as (-1)^m P^m (the solve of mode m reads the stored matrix at phi + pi); the first-order vectors
            d_P0 = []
            d_Paer = torch.empty((M, D, D), dtype=torch.float64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            for which, phase in enumerate(((atm_phase_fun, g_atm, mie_atm), (aer_phase_fun, g_aer, mie_aer))):
                kind, g = _phase_kind(s, *phase)
                if which == 0:
                    sgn = np.where(np.arange(1, M + 1) & 1, -1.0, 1.0)[:, None, None]
                    P_atm_m = sgn * s.phase_modes(kind, 1, M, nphi, g)
                else:
                    s.phase_modes_device(kind, d_Paer.data_ptr(), 1, M, nphi, g, sign_odd=True)
                p0 = torch.empty((M, B, D), dtype=torch.float64, device=dev)
                s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p0.data_ptr(), B, 1, M, nphi, g)
                d_P0.append(p0)
            d_st = torch.zeros((M, B), dtype=torch.int32, device=dev)
            for m0 in range(1, M + 1, c):
                cc = min(c, M + 1 - m0)
                s.synchronize()                              # (the setters rewrite what the previous chunk's solve read)
                s.set_columns(*[tile(v, cc) for v in colargs])
                s.set_phase_sets_device(P_atm_m[m0 - 1], d_Paer[m0 - 1].data_ptr(), cc)
                try:
                    s.set_atm_phase_sets(P_atm_m[m0 - 1:m0 - 1 + cc])
                    sets = np.repeat(np.arange(cc, dtype=np.int32), B)
                    s.set_aerosol_sets(sets)
                    s.set_atmosphere_sets(sets)
                except ValueError as e:
                    raise ValueError("mode_batch=True is not available here: %s; mode_batch=False works" % e) from None
                d_tau_c, d_tgt_c = d_tau.repeat(cc, 1), d_target.repeat(cc)
                d_n = torch.zeros(cc * B, dtype=torch.int32, device=dev)
                s.set_order_targets(d_tgt_c.data_ptr())
                s.solve_device(d_tau_c.data_ptr(), d_P0[0][m0 - 1].data_ptr(), d_P0[1][m0 - 1].data_ptr(),
                               d_Im[m0 - 1].data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st[m0 - 1].data_ptr())
                s.synchronize()                              # (d_tau_c, d_tgt_c and d_n go out of scope)
                s.set_order_targets(None)
            s.azimuth_synthesize_device(M, d_I0.data_ptr(), d_Im.data_ptr(), d_lev.data_ptr(), nlev, d_phi.data_ptr(), nout,
                                        d_out.data_ptr(), B=B)
            s.synchronize()
            status[1:] = d_st.cpu().numpy()
            I_az = d_out.cpu().numpy()
    finally:
        s.set_order_targets(None)
        # the cached handle as the plain call left it: its B columns (on set 0 of both kinds), then the mode-0 matrices
        s.set_columns(*colargs)
        if P_mode0[0] is not None:
            s.set_phase(*P_mode0)
    return I_az, status


def _prepare_batch(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, z0, z_up, z_down, nb_layers, nb_angles,
                   atm_phase_fun, g_atm, aer_phase_fun, g_aer, mie_atm, mie_aer, P_atm, P_aer, P0_atm, P0_aer, surface,
                   max_orders, device, p0_on_host=True, aer_set=None, delta_m=None, gas=None):
    """Everything before the order loop (spec:23-96): optical-depth grids, direction grid, phase matrices folded into the
    handle, per-column scalars.  Returns the solver and the per-column inputs.  `delta_m` (the namespace of `_delta_m_args`):
    the aerosol is delta-M-scaled first (`_delta_m_aerosol`) -- its P0 and P come from the truncated table, and the optical-depth
    grid and the columns from the scaled tauStar_aer and alb_aer -- and the namespace is filled.  `gas` (the namespace of
    `_gas_args`): the returned tau and the columns' tauStar_tot include the gas, and the namespace gets tau0 and the row weights w
    (`inputs.gas_row_weights`); dtau_atm and dtau_aer stay the scattering column's, they only form the fractions."""
    mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer = _broadcast_columns(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm,
                                                                                  alb_aer)
    B = mu0.shape[0]
    L, N = int(nb_layers), int(nb_angles)
    if z_down > z_up:
        z_down, z_up = z_up, z_down
    mu = direction_grid(N)
    iu, idn = slab_indices(z0, z_up, z_down, L)
    if delta_m is not None:
        s = get_solver(L, N, B, max_orders, device)
        if not s.same_grid(mu):
            s.set_grid(mu)
        (aer_phase_fun, g_aer, mie_aer), tauStar_aer, alb_aer = _delta_m_aerosol(s, delta_m, aer_phase_fun, g_aer, mie_aer,
                                                                                 tauStar_aer, alb_aer, device)
    tau = np.stack([tau_profile(tauStar_atm[b], tauStar_aer[b], z0, z_up, z_down, L) for b in range(B)])
    tauStar_tot = tauStar_atm + tauStar_aer
    if gas is not None:
        gas.tau0 = tau
        tau, gas.w = gas_row_weights(tau, gas.gas_tau)
        tauStar_tot = tauStar_tot + gas.gas_tau[:, -1]
    s = get_solver(L, N, B, max_orders, device)
    if not s.same_grid(mu):
        s.set_grid(mu)
    # the inputs of the path that are not handed in: P0(mu, mu0[b]) per column and P(mu, mu') on the device
    # (phase:79-133; the Mie-derived functions as tables on the scattering cosine)
    P0a = P0r = None
    if P_atm is None or P0_atm is None:
        P0a, Pm = device_phase(s, atm_phase_fun, mu0, g_atm, mie_atm, matrix=P_atm is None)
        P_atm = Pm if P_atm is None else P_atm
    if aer_set is not None:
        sets = np.ascontiguousarray(aer_set)
        if sets.shape != (B,) or not np.issubdtype(sets.dtype, np.integer):
            raise ValueError("aer_set must be %d integers (one aerosol per column)" % B)
        on_device = isinstance(P_aer, DevicePhaseSets)
        if on_device:
            if P0_aer is None or np.shape(P0_aer) != (B, 2 * N):
                raise ValueError("aer_set with matrices on the device needs P0_aer [B, 2N] (each column the P0 of its aerosol)")
        elif P_aer is not None:
            P_aer = np.ascontiguousarray(P_aer, dtype=np.float64)
            if P_aer.ndim != 3 or P0_aer is None or np.shape(P0_aer) != (B, 2 * N):
                raise ValueError("aer_set with arrays needs P_aer [S, 2N, 2N] and P0_aer [B, 2N] (each column the P0 of its aerosol)")
        else:
            if not isinstance(aer_phase_fun, (list, tuple)):
                raise ValueError("aer_set needs a list of names in aer_phase_fun (or a stack P_aer [S, 2N, 2N] with P0_aer)")
            S = len(aer_phase_fun)
            per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * S
            gs, ms = per(g_aer), per(mie_aer)
            if len(gs) != S or len(ms) != S:
                raise ValueError("g_aer and mie_aer must be single values or lists as long as aer_phase_fun")
            if sets.size and (sets.min() < 0 or sets.max() >= S):
                raise ValueError("aer_set names aerosol %d, aer_phase_fun has %d" % (int(sets.max() if sets.max() >= S else sets.min()), S))
            built, P0r = [], np.zeros((B, 2 * N))
            for k in range(S):
                # (an aerosol that no column uses still gets its matrix: set indices keep their meaning; its P0 row is not needed)
                cols = np.flatnonzero(sets == k)
                p0, Pm = device_phase(s, aer_phase_fun[k], mu0[cols] if cols.size else mu0[:1], gs[k], ms[k])
                if cols.size:
                    P0r[cols] = p0
                built.append(Pm)
            P_aer = np.stack(built)
        if P0_aer is not None:
            P0r = np.ascontiguousarray(P0_aer, dtype=np.float64)
        if on_device:
            s.set_phase_sets_device(P_atm, P_aer.address, P_aer.S)
        elif not s.same_phase(P_atm, P_aer):
            s.set_phase_sets(P_atm, P_aer)
    else:
        if P_aer is None or P0_aer is None:
            P0r, Pm = device_phase(s, aer_phase_fun, mu0, g_aer, mie_aer, matrix=P_aer is None)
            P_aer = Pm if P_aer is None else P_aer
        if P0_aer is not None:
            P0r = np.ascontiguousarray(np.broadcast_to(P0_aer, (B, 2 * N)))
        if not s.same_phase(P_atm, P_aer):
            s.set_phase(P_atm, P_aer)
    if P0_atm is not None:
        P0a = np.ascontiguousarray(np.broadcast_to(P0_atm, (B, 2 * N)))
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, grd_alb, alb_atm, alb_aer,
                  tauStar_atm / L, tauStar_aer / (idn + 1 - iu), tauStar_tot, surface=surface)
    if aer_set is not None:
        s.set_aerosol_sets(sets.astype(np.int32))
    return s, tau, P0a, P0r, mu, iu, idn, N


def solve_batch_device(mu0, tauStar_aer, grd_alb, *, tauStar_atm=0.124, alb_atm=1.0, alb_aer=1.0, z0=120, z_up=25, z_down=17,
                       nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7,
                       mie_atm=None, mie_aer=None, P_atm=None, P_aer=None, P0_atm=None, P0_aer=None, surface="specular",
                       tol=1e-4, max_orders=256, device=0, beam="plane", earth_radius=EARTH_RADIUS_KM, source="solar",
                       planck=None, planck_surface=None, surface_emissivity=None, aer_set=None, brdf=None,
                       max_bounces=MAX_BOUNCES, delta_m=None, gas_tau=None, profile_post=None):
    """`SOS_Aer_batch` with the RESULT LEFT ON THE DEVICE: returns ({"I": [B, L, 2N] float64, "n": [B] int32, "status": [B]
    int32, "tau": [B, L]} as torch tensors on cuda:`device`, (mu, idx_up, idx_down)).  The solve is enqueued on torch's
    current stream for that device, so the tensors are ordered like any torch result.  What `dist.solve_sharded` gathers.
    `beam='spherical'` (with `earth_radius`, km): the pseudo-spherical direct beam of `SOS_Aer_batch`; the dict then also holds
    "beam_slant" [B, L].  `source='thermal'` (with `planck`, `planck_surface`, `surface_emissivity`): the thermal field of
    `SOS_Aer_batch`.  `aer_set` [B] with a list of names in `aer_phase_fun` (or a stack `P_aer`): several aerosols in one batch,
    as in `SOS_Aer_batch`; the cached handle's columns are back on aerosol set 0 when the call returns, also on error.
    `surface='brdf'` with `brdf=` (and `max_bounces`): the BRDF ground of `SOS_Aer_batch`; the dict then also holds "bounces"
    and "bounce_ratio" [B].  `delta_m=Lambda`: the delta-M-scaled aerosol of `SOS_Aer_batch` (same refusals); the dict then also
    holds "delta_m_f" (a float) and the host arrays "tauStar_aer_scaled", "alb_aer_scaled" [B], and I and tau are the scaled
    column's.  `gas_tau` ([L] or [B, L]): the absorbing gas of `SOS_Aer_batch` (same refusals); tau is the total, and the dict then
    also holds the host arrays "gas_tau" and "row_weight" [B, L]; `profile_post` is then the `post` of `solve_profile`: it runs
    behind the solve while the weights are set (the view stage of `bands.band_solar`)."""
    gas = _gas_args(gas_tau, lambda: _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer), nb_layers, surface=surface,
                    delta_m=delta_m)
    dm = _delta_m_args(delta_m, aer_phase_fun, aer_set=aer_set, P_aer=P_aer, P0_aer=P0_aer, surface=surface, beam=beam, source=source)
    thermal = _thermal_args(source, planck, planck_surface, surface_emissivity,
                            _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer) if source == "thermal" else 0,
                            nb_layers, beam=beam)
    spherical = _beam_args(beam, earth_radius)
    ground = _brdf_args(surface, brdf, grd_alb, nb_angles,
                        _batch_width(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer) if surface == "brdf" else 0,
                        beam=beam, source=source)
    if ground:
        surface, grd_alb = "specular", 0.0
    s, tau, P0a, P0r, mu, iu, idn, N = _prepare_batch(mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, z0, z_up, z_down,
                                                      nb_layers, nb_angles, atm_phase_fun, g_atm, aer_phase_fun, g_aer, mie_atm,
                                                      mie_aer, P_atm, P_aer, P0_atm, P0_aer, surface, max_orders, device,
                                                      aer_set=aer_set, delta_m=dm, gas=gas)
    try:
        if gas is not None:
            out = solve_profile(s, tau, P0a, P0r, gas.w, np.broadcast_to(np.asarray(mu0, dtype=np.float64), (tau.shape[0],)),
                                np.linspace(z0, 0, int(nb_layers)) if spherical else None, earth_radius, thermal, tol, device,
                                keep_device=True, post=profile_post)
            return dict(out, gas_tau=gas.gas_tau, row_weight=gas.w), (mu, iu, idn)
        if dm is not None:
            out = _solve_resident(s, tau, P0a, P0r, None, None, tol, device=device, keep_device=True)
            return dict(out, delta_m_f=dm.f, tauStar_aer_scaled=dm.tauStar_aer, alb_aer_scaled=dm.alb_aer), (mu, iu, idn)
        if spherical:
            return solve_spherical(s, tau, P0a, P0r, np.linspace(z0, 0, int(nb_layers)), earth_radius, tol, device=device,
                                   keep_device=True), (mu, iu, idn)
        if thermal:
            return solve_thermal(s, tau, *thermal, tol=tol, keep_device=True, device=device), (mu, iu, idn)
        if ground:
            return solve_brdf(s, tau, P0a, P0r, ground, mu0, tol, max_bounces, device=device, keep_device=True), (mu, iu, idn)
        return _solve_resident(s, tau, P0a, P0r, None, None, tol, device=device, keep_device=True), (mu, iu, idn)
    finally:
        if aer_set is not None:
            _columns_to_set0(s, tau.shape[0])


def SOS_Aer_layers(mu0, grd_alb, slabs, *, tauStar_atm=0.124, alb_atm=1.0, z0=120, nb_layers=200, nb_angles=128,
                   atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7, mie_atm=None, mie_aer=None, P_atm=None,
                   P_aer=None, surface="specular", tol=1e-4, max_orders=256, device=0, raise_on_error=True, beam="plane",
                   earth_radius=EARTH_RADIUS_KM, source="solar", planck=None, planck_surface=None,
                   surface_emissivity=None, brdf=None, max_bounces=MAX_BOUNCES, delta_m=None, gas_tau=None) -> BatchResult:
    """Columns with SEVERAL aerosol layers (the reference has one): `slabs` = [(z_up, z_down, tauStar_aer,
    alb_aer), ...] from the top down, shared by the B columns of the arrays `mu0`, `grd_alb`.  Every formula of the path is
    evaluated per zone as the reference writes it for its three zones; one layer gives `SOS_Aer_batch`'s result bit for
    bit.  A slab may name ITS OWN AEROSOL in a fifth entry -- a phase-function name ('hg' with `g_aer`, 'eva', 'wildfire', ...)
    or a dict(name=, g=, and the keywords of `mie_aer`) -- e.g. slabs=[(25, 17, 0.12, 0.97, "eva"), (15, 14, 0.0075, 0.9,
    "wildfire")]; slabs without one take (`aer_phase_fun`, `g_aer`, `mie_aer`), and when no slab has one all layers share
    that phase function exactly as before.  `P_aer` cannot be combined with a fifth entry.  `idx_up` / `idx_down` of the
    result are those of the first layer.  `beam='spherical'` (with `earth_radius`, km): the pseudo-spherical direct beam of
    `SOS_Aer_batch`, BatchResult.beam_slant [B, L].  `source='thermal'` (with `planck`, `planck_surface`,
    `surface_emissivity`): the thermal field of `SOS_Aer_batch`; every aerosol layer emits with its own albedo.
    `surface='brdf'` with `brdf=` (and `max_bounces`): the BRDF ground of `SOS_Aer_batch`; BatchResult.bounces / bounce_ratio.
    `delta_m` is refused: every slab would need its own truncated fraction.  `gas_tau` is refused too (an open item of DESIGN
    section 29)."""
    from .inputs import tau_profile_slabs
    if gas_tau is not None:
        raise ValueError("gas_tau is not available with SOS_Aer_layers yet: SOS_Aer_batch(gas_tau=...) takes the gas profile of its "
                         "one-slab columns")
    if delta_m is not None:
        raise ValueError("delta_m is not available with SOS_Aer_layers: every slab would need its own truncated fraction; "
                         "SOS_Aer_batch(delta_m=...) scales the one slab of its columns")
    thermal = _thermal_args(source, planck, planck_surface, surface_emissivity,
                            _batch_width(mu0, grd_alb) if source == "thermal" else 0, nb_layers, beam=beam)
    spherical = _beam_args(beam, earth_radius)
    ground = _brdf_args(surface, brdf, grd_alb, nb_angles, _batch_width(mu0, grd_alb) if surface == "brdf" else 0, beam=beam,
                        source=source)
    if ground:
        surface, grd_alb = "specular", np.zeros(_batch_width(mu0, grd_alb))
    mu0, grd_alb = np.broadcast_arrays(np.atleast_1d(np.asarray(mu0, dtype=np.float64)), np.atleast_1d(np.asarray(grd_alb, dtype=np.float64)))
    B, L, N = mu0.shape[0], int(nb_layers), int(nb_angles)
    mu = direction_grid(N)
    tau, r0, mix, dta = tau_profile_slabs(tauStar_atm, [s[:3] for s in slabs], z0, L)
    zwr = np.zeros(len(r0))
    zwr[1::2] = [s[3] for s in slabs]
    s = get_solver(L, N, B, max_orders, device)
    if not s.same_grid(mu):
        s.set_grid(mu)
    # P0(mu, mu0) per column, and the matrices that were not handed in, on the device
    P0a, Pm = device_phase(s, atm_phase_fun, mu0, g_atm, mie_atm, matrix=P_atm is None)
    P_atm = Pm if P_atm is None else P_atm
    own = any(len(x) > 4 for x in slabs)
    if own:
        if P_aer is not None:
            raise ValueError("P_aer cannot be combined with slabs that name their own aerosol")
        # the distinct aerosols of the slabs, in order of appearance: one phase set each
        def spec(x):
            a = x[4] if len(x) > 4 else None
            if a is None:
                return (aer_phase_fun, g_aer, mie_aer)
            if isinstance(a, str):
                return (a, g_aer, None)
            a = dict(a)
            return (a.pop("name", aer_phase_fun), a.pop("g", g_aer), a or None)
        specs, zset = [], np.zeros(len(r0), dtype=np.int32)
        for j, x in enumerate(slabs):
            sp = spec(x)
            k = next((i for i, y in enumerate(specs) if _same_aerosol(y, sp)), len(specs))
            if k == len(specs):
                specs.append(sp)
            zset[1 + 2 * j] = k
        built = [device_phase(s, name, mu0, g, mie) for name, g, mie in specs]
        P0r = np.zeros((B, len(r0), 2 * N))
        for j in range(len(slabs)):
            P0r[:, 1 + 2 * j] = built[zset[1 + 2 * j]][0]
        P_sets = np.stack([b[1] for b in built])
        if not s.same_phase(P_atm, P_sets):
            s.set_phase_sets(P_atm, P_sets)
    else:
        P0r, Pm = device_phase(s, aer_phase_fun, mu0, g_aer, mie_aer, matrix=P_aer is None)
        P_aer = Pm if P_aer is None else P_aer
        if not s.same_phase(P_atm, P_aer):
            s.set_phase(P_atm, P_aer)
    s.set_columns_zones(np.tile(r0, (B, 1)), mix, mu0, grd_alb, alb_atm, tauStar_atm / L, zwr, dta,
                        tauStar_atm + sum(x[2] for x in slabs), surface=surface)
    try:
        if own:
            s.set_aerosol_sets(np.tile(zset, (B, 1)))
        sigma = None
        bx = {}
        if spherical:
            r, sigma, _ = solve_spherical(s, np.tile(tau, (B, 1)), P0a, P0r, np.linspace(z0, 0, L), earth_radius, tol, device=device)
        elif ground:
            r, bx, _ = solve_brdf(s, np.tile(tau, (B, 1)), P0a, P0r, ground, mu0, tol, max_bounces, device=device)
        elif thermal:
            r, _ = solve_thermal(s, np.tile(tau, (B, 1)), *thermal, tol=tol, device=device)
        else:
            r = s.solve(np.tile(tau, (B, 1)), P0a, P0r, tol=tol)
    finally:
        if own:                                              # (the solver is cached: its columns go back to set 0)
            _columns_to_set0(s, B)
    if raise_on_error:
        _raise_status(r.status, N)
    return BatchResult(I=r.I, n=r.n, status=r.status, tau=np.tile(tau, (B, 1)), mu=mu, idx_up=int(r0[1]), idx_down=int(r0[2]) - 1,
                       beam_slant=sigma, bounces=bx.get("bounces"), bounce_ratio=bx.get("bounce_ratio"),
                       bounce_orders=bx.get("bounce_orders"), black_sky_albedo=bx.get("black_sky_albedo"),
                       white_sky_albedo=bx.get("white_sky_albedo"))


def SOS_Aer(surface="specular", tol=1e-4, max_orders=256, P_atm=None, P0_atm=None, P_aer=None, P0_aer=None, device=0,
            first_order="coded", beam="plane", earth_radius=EARTH_RADIUS_KM, source="solar", planck=None, planck_surface=None,
            surface_emissivity=None, brdf=None, max_bounces=MAX_BOUNCES, delta_m=None, gas_tau=None, **overrides) -> ColumnResult:
    """One column with the reference's parameter names (spec:19-96).  `surface` selects the file of
    the reference that would be run ('specular' | 'lambertian'); P*/P0* accept pre-built phase
    arrays.  `beam='spherical'` (with `earth_radius`, km): the pseudo-spherical direct beam of `SOS_Aer_batch`;
    ColumnResult.beam_slant [L].  `source='thermal'` (with `planck` [L], `planck_surface`, `surface_emissivity`): the thermal
    field of `SOS_Aer_batch`.  `surface='brdf'` with `brdf=` (and `max_bounces`): the BRDF ground of `SOS_Aer_batch`;
    ColumnResult.bounces / bounce_ratio; I_saved is None (the field is a sum over ground reflections) and n the black solve's.
    `delta_m=Lambda`: the delta-M-scaled aerosol of `SOS_Aer_batch` (same refusals); I, I_saved and tau are the scaled column's,
    ColumnResult.delta_m_f / tauStar_aer_scaled / alb_aer_scaled say what was solved.  `gas_tau` [L]: the absorbing gas of
    `SOS_Aer_batch` (same refusals); tau is the total, ColumnResult.gas_tau / row_weight say what was solved, and I_saved is None
    (the per-order history is not kept under weights)."""
    _gas_args(gas_tau, 1, overrides.get("nb_layers", DEFAULTS["nb_layers"]), surface=surface, delta_m=delta_m, first_order=first_order)
    _delta_m_args(delta_m, overrides.get("aer_phase_fun", DEFAULTS["aer_phase_fun"]), P_aer=P_aer, P0_aer=P0_aer, surface=surface,
                  beam=beam, source=source, first_order=first_order)
    _thermal_args(source, planck, planck_surface, surface_emissivity, 1,
                  overrides.get("nb_layers", DEFAULTS["nb_layers"]), beam=beam, first_order=first_order)
    _beam_args(beam, earth_radius, first_order=first_order)
    ground = _brdf_args(surface, brdf, overrides.get("grd_alb", DEFAULTS["grd_alb"]), overrides.get("nb_angles", DEFAULTS["nb_angles"]),
                        1, beam=beam, source=source, first_order=first_order)
    unknown = set(overrides) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown parameter(s): %s" % ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **overrides)
    N, L = int(p["nb_angles"]), int(p["nb_layers"])
    mie = {k: dict(r=p["r_" + k], lambda0=p["lambda0_" + k], indx=p["indx_" + k], r_m=p["r_m_" + k], sig=p["sig_" + k])
           for k in ("atm", "aer")}
    r = SOS_Aer_batch(p["mu0"], p["tauStar_aer"], p["grd_alb"], tauStar_atm=p["tauStar_atm"], alb_atm=p["alb_atm"],
                      alb_aer=p["alb_aer"], z0=p["z0"], z_up=p["z_up"], z_down=p["z_down"], nb_layers=L, nb_angles=N,
                      atm_phase_fun=p["atm_phase_fun"], g_atm=p["g_atm"], aer_phase_fun=p["aer_phase_fun"], g_aer=p["g_aer"],
                      mie_atm=mie["atm"], mie_aer=mie["aer"], P_atm=P_atm, P_aer=P_aer,
                      P0_atm=None if P0_atm is None else np.asarray(P0_atm)[None],
                      P0_aer=None if P0_aer is None else np.asarray(P0_aer)[None],
                      surface=surface, tol=tol, max_orders=max_orders, save_orders=not ground and gas_tau is None, device=device,
                      first_order=first_order, gas_tau=gas_tau,
                      beam=beam, earth_radius=earth_radius, source=source, planck=planck, planck_surface=planck_surface,
                      surface_emissivity=surface_emissivity, brdf=brdf, max_bounces=max_bounces, delta_m=delta_m)
    n = int(r.n[0])
    return ColumnResult(I=r.I[0], I_saved=None if ground or gas_tau is not None else r.I_saved[0, :n].copy(), n=n, tau=r.tau[0], mu=r.mu, idx_up=r.idx_up,
                        idx_down=r.idx_down, status=int(r.status[0]), beam_slant=None if r.beam_slant is None else r.beam_slant[0],
                        bounces=None if r.bounces is None else int(r.bounces[0]),
                        bounce_ratio=None if r.bounce_ratio is None else float(r.bounce_ratio[0]),
                        black_sky_albedo=None if r.black_sky_albedo is None else float(r.black_sky_albedo[0]),
                        white_sky_albedo=None if r.white_sky_albedo is None else float(r.white_sky_albedo[0]),
                        delta_m_f=r.delta_m_f,
                        tauStar_aer_scaled=None if r.tauStar_aer_scaled is None else float(r.tauStar_aer_scaled[0]),
                        alb_aer_scaled=None if r.alb_aer_scaled is None else float(r.alb_aer_scaled[0]),
                        gas_tau=None if r.gas_tau is None else r.gas_tau[0], row_weight=None if r.row_weight is None else r.row_weight[0])
