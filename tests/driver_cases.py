"""The cases of tests/test_gpu_driver_bits.py and tools/record_driver_bits.py: every Python driver of sosrt (main, forcing, thermal,
bands) on the smallest shapes at which a driver can mix up columns, chunks or modes -- L = 24, N = 32, three columns that differ in
mu0, aerosol optical depth and ground, Rayleigh + Henyey-Greenstein (g = 0.7).  A case returns (outputs by name, the status arrays
of its solves); `run(name)` starts it from fresh handles and returns (SHA-256 of the bytes of every output, the statuses).  The
drivers are host code over one library: their outputs are compared bit for bit with those of an earlier commit's package on the
same library (tests/golden/driver_bits.json).

The optical depths are small because the grid is coarse: the order loop's mu -> 0 search compares second differences of the field
with an absolute 1e-4, and at N = 32 it runs off the grid (status 1) for depths that a finer grid takes."""
import dataclasses
import hashlib

import numpy as np

L, N = 24, 32
SHAPE = dict(nb_layers=L, nb_angles=N)
MU0 = np.array([0.3, 0.5, 0.8])
# (tauStar_aer = [0.1, 0.3, 0.2] halved: at the full depths column 1 ends with status 1)
T_AER = np.array([0.05, 0.15, 0.1])
RHO = np.array([0.1, 0.3, 0.0])
PHASE = dict(atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
# thermal cases: grey columns, so that the layers emit (the albedos of tools/time_thermal.py); a Planck ramp that differs per column
# (tauStar_atm = 0.5 and tauStar_aer = [0.1, 0.3, 0.2] quartered: at the full and at the halved depths two columns end with status 1)
GREY = dict(tauStar_atm=0.125, alb_atm=0.5, alb_aer=0.8)
GREY_T_AER = np.array([0.025, 0.075, 0.05])
PLANCK = np.linspace(0.4, 1.0, L)[None, :] * (1 + 0.1 * np.arange(3))[:, None]
THERMAL = dict(source="thermal", planck=PLANCK, planck_surface=np.array([1.0, 1.1, 0.9]))
TWO_AEROSOLS = dict(atm_phase_fun="rayleigh", aer_phase_fun=["hg", "rayleigh"], g_aer=[0.7, 0.0])
VIEW_MU = np.array([0.3, 0.9])
# BRDF ground.  Lambertian: T_AER halved once more (at T_AER column 1 ends with status 1).  RPV: no aerosol depth helps column 0,
# whose low sun (mu0 = 0.3) leaves the ground's unscattered rows so steep towards mu -> 0 that their search runs off the grid at
# tauStar_atm = 0.124 and below, however thin the aerosol; under tauStar_atm = 0.25 the beam at the ground is weak enough, and T_AER stays
RPV = ("rpv", 0.2, 0.8, -0.1)
RPV_T_ATM = 0.25
# two aerosol layers (rows 12..15 and 18..20 of the 24), each with its own aerosol
SLABS = [(58, 42, 0.05, 0.9, dict(name="hg", g=0.7)), (25, 17, 0.1, 0.8, "rayleigh")]


def fresh():
    """Close the cached handles."""
    from sosrt import main as M
    for s in list(M._solvers.values()):
        s.close()
    M._solvers.clear()


def _batch(names, t_aer=T_AER, rho=RHO, **kw):
    from sosrt.main import SOS_Aer_batch
    r = SOS_Aer_batch(MU0, GREY_T_AER if kw.get("source") == "thermal" else t_aer, rho, raise_on_error=False, **SHAPE,
                      **dict(PHASE, **kw))
    st = [r.status] + [getattr(r, k) for k in ("mode_status", "view_mode_status") if getattr(r, k) is not None]
    return {k: getattr(r, k) for k in names}, st


def _device(**kw):
    from sosrt.main import solve_batch_device
    d, _ = solve_batch_device(MU0, GREY_T_AER if kw.get("source") == "thermal" else T_AER, RHO, **SHAPE, **dict(PHASE, **kw))
    d = {k: v.cpu().numpy() for k, v in d.items()}
    return d, [d["status"]]


def _layers(**kw):
    from sosrt.main import SOS_Aer_layers
    r = SOS_Aer_layers(MU0, RHO, SLABS, atm_phase_fun="rayleigh", raise_on_error=False, **SHAPE, **kw)
    out = {k: getattr(r, k) for k in ("I", "n", "status")}
    if r.beam_slant is not None:
        out["beam_slant"] = r.beam_slant
    return out, [r.status]


def _toa_net_flux(**kw):
    from sosrt.forcing import toa_net_flux
    return {"net_toa": toa_net_flux(0.5, 0.124, T_AER, 0.1, 1.0, [0.9, 0.95, 1.0], g_aer=0.7, **SHAPE, **kw)}, []


def _thermal_toa_flux():
    from sosrt.thermal import thermal_toa_flux
    return {"flux_up": thermal_toa_flux(GREY_T_AER, RHO, PLANCK, THERMAL["planck_surface"], **GREY, **SHAPE, **PHASE)}, []


def _band(r):
    return {k: v for k, v in dataclasses.asdict(r).items() if v is not None}, [r.status]


# K = 3 points x C = 2 columns in chunks of 2 points: the last chunk is ragged
BAND = dict(points_per_solve=2, per_point=True, **SHAPE)
BAND_T_AER = np.array([[0.05, 0.15], [0.1, 0.025], [0.15, 0.075]])


def _band_thermal():
    from sosrt.bands import band_thermal
    T = np.stack([np.linspace(220.0, 288.0, L), np.linspace(210.0, 280.0, L)])
    return _band(band_thermal(([100.0, 500.0, 900.0], [500.0, 900.0, 1300.0]), T, [288.0, 281.0], BAND_T_AER / 2, [0.1, 0.3],
                              tauStar_atm=[0.1, 0.125, 0.15], alb_atm=0.5, alb_aer=0.8, weights=[0.5, 1.0, 1.5], **BAND, **PHASE))


def _band_solar():
    from sosrt.bands import band_solar
    return _band(band_solar([1.5, 1.0, 0.5], [0.3, 0.8], BAND_T_AER, [0.1, 0.3], tauStar_atm=[0.2, 0.124, 0.05], alb_atm=1.0,
                            alb_aer=0.95, point_aerosol=[0, 1, 0], **BAND, **TWO_AEROSOLS))


def _spectrum(one_batch):
    from sosrt.main import SOS_Aer_spectrum
    res, bulk = SOS_Aer_spectrum([0.45, 0.65], [0.3, 0.8], 0.1, [0.1, 0.3], dict(m=1.44 + 0.001j, r_m=0.35, sig=1.5), angstrom=1.3,
                                 tauStar_atm_ref=0.06, nb_radius=40, ntab=2001, one_batch=one_batch, raise_on_error=False, **SHAPE)
    out = {"bulk": bulk}
    for w, r in enumerate(res):
        out.update({"%s_%d" % (k, w): getattr(r, k) for k in ("I", "n", "status")})
    return out, [r.status for r in res]


def _brdf_stages():
    """The stages of the BRDF ground through the `Solver` methods, on a handle with the grid and three black columns: the six
    builders of RPV on nphi = 300 nodes (two chunks of the kernels' 256) for the modes 0..9 (two launches of 8, the second ragged),
    with and without the odd sign, at the grid's nodes and at V = 3 view cosines of which one is a node, for B = 3 columns; the
    rows at azimuths; the ground source and the view ground with and without their optional terms."""
    import torch
    from sosrt import inputs
    from sosrt.solver import Solver
    dev = torch.device("cuda", 0)
    B, M1, nm, nphi, p = 3, N - 1, 10, 300, RPV[1:]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    f64 = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    mu = inputs.direction_grid(N)
    mv = np.array([0.3, mu[N + 1 + 5], 0.9])
    V = len(mv)
    rng = np.random.default_rng(2432)
    d_I = up(0.05 + rng.random((B, L, 2 * N)) * (1 + np.arange(2 * N) / N))
    d_tau = up(np.linspace(0, 1, L)[None, :] * np.array([0.2, 0.3, 0.4])[:, None])
    d_mu0, d_scale, d_phi = up(MU0), up([0.5, 1.0, 2.0]), up([0.0, 1.0, 2.0])
    s = Solver(L, N, max_batch=B)
    try:
        s.set_grid(mu)
        iu, idn = inputs.slab_indices(120, 25, 17, L)
        s.set_columns(np.full(B, iu), np.full(B, idn), MU0, 0.0, 1.0, 0.95, 0.124 / L, 0.3 / (idn + 1 - iu), 0.424)
        torch.cuda.synchronize()
        o = dict(operator=f64(M1, M1), beam=f64(B, M1), beam_modes=f64(nm, B, M1), view_beam_modes=f64(nm, B, V),
                 view_beam_azimuth=f64(3, B, V))
        s.brdf_operator_device("rpv", o["operator"].data_ptr(), p, nphi)
        s.brdf_beam_device("rpv", d_mu0.data_ptr(), o["beam"].data_ptr(), p, nphi, B=B)
        s.brdf_beam_modes_device("rpv", d_mu0.data_ptr(), o["beam_modes"].data_ptr(), 0, nm, p, nphi, B=B)
        s.brdf_view_beam_modes_device("rpv", d_mu0.data_ptr(), mv, o["view_beam_modes"].data_ptr(), 0, nm, p, nphi, B=B)
        s.brdf_view_beam_azimuth_device("rpv", d_mu0.data_ptr(), mv, d_phi.data_ptr(), 3, o["view_beam_azimuth"].data_ptr(), p, B=B)
        for sign in (False, True):
            R, Rv = f64(nm, M1, M1), f64(nm, M1, V)
            s.brdf_operator_modes_device("rpv", R.data_ptr(), 0, nm, p, nphi, sign_odd=sign)
            s.brdf_view_rows_modes_device("rpv", mv, Rv.data_ptr(), 0, nm, p, nphi, sign_odd=sign)
            o["operator_modes_sign%d" % sign], o["view_rows_modes_sign%d" % sign] = R, Rv
        for name, opt in (("plain", False), ("beam_scale", True)):
            o["ground_source_" + name] = S = f64(B, M1)
            s.ground_source_device(d_I.data_ptr(), d_tau.data_ptr(), o["operator"].data_ptr(), S.data_ptr(),
                                   o["beam"].data_ptr() if opt else 0, d_scale.data_ptr() if opt else 0, B=B)
        Rv0, r0v = o["view_rows_modes_sign0"][0], o["view_beam_modes"][0]
        lev, vg, o["view_ground_S"] = [0, L - 1], f64(B, 2, 2 * V), f64(B, V)
        s.view_ground_device(mv, d_tau.data_ptr(), lev, vg.data_ptr(), d_I=d_I.data_ptr(), d_Rv=Rv0.data_ptr(), d_r0v=r0v.data_ptr(),
                             d_scale=d_scale.data_ptr(), d_S_out=o["view_ground_S"].data_ptr(), B=B)
        s.synchronize()
        o["view_ground_written"] = vg.clone()
        s.view_ground_device(mv, d_tau.data_ptr(), lev, vg.data_ptr(), d_I=d_I.data_ptr(), d_Rv=Rv0.data_ptr(), accumulate=True, B=B)
        o["view_ground_accumulated"] = vg
        s.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}, []
    finally:
        s.close()


SOLVE = ("I", "n", "status", "I_saved")
AZIMUTH = dict(azimuths=[0, 1.0, 3.0], n_modes=3)
VIEW_AZIMUTH = dict(view_mu=VIEW_MU, view_azimuths=[0, 2.0], n_modes=3)
VIEW_AZIMUTH_OUT = ("I_view_azimuth", "I_view_azimuth_first", "I_view_azimuth_scattered", "view_mode_status")
THERMAL_VIEW = dict(THERMAL, **GREY, save_orders=True, view_mu=VIEW_MU)
THERMAL_VIEW_OUT = ("I", "I_saved", "I_view_first", "I_view_scattered")
# the BRDF ground: every field the result carries for the mode
BRDF_OUT = ("I", "n", "status", "bounces", "bounce_ratio", "bounce_orders")
BRDF_VIEW_OUT = BRDF_OUT + ("I_view", "I_view_first", "I_view_scattered", "I_view_ground")
BRDF_VIEW_AZIMUTH_OUT = BRDF_VIEW_OUT + VIEW_AZIMUTH_OUT + ("I_view_azimuth_ground",)
_rpv = lambda names, **kw: _batch(names, T_AER, 1.0, surface="brdf", brdf=RPV, tauStar_atm=RPV_T_ATM, **kw)

CASES = {
    "batch_plain": lambda: _batch(SOLVE, save_orders=True),
    "batch_spherical": lambda: _batch(SOLVE + ("beam_slant",), save_orders=True, beam="spherical"),
    "batch_thermal_view_grid": lambda: _batch(THERMAL_VIEW_OUT, view_quadrature="grid", **THERMAL_VIEW),
    "batch_thermal_view_linear": lambda: _batch(THERMAL_VIEW_OUT, view_quadrature="linear", **THERMAL_VIEW),
    "aer_set_plane": lambda: _batch(("I", "n", "status"), aer_set=[0, 1, 0], **TWO_AEROSOLS),
    "aer_set_spherical": lambda: _batch(("I", "n", "status", "beam_slant"), aer_set=[0, 1, 0], beam="spherical", **TWO_AEROSOLS),
    "azimuth_loop": lambda: _batch(("I_azimuth", "mode_status"), **AZIMUTH),
    "azimuth_mode_batch": lambda: _batch(("I_azimuth", "mode_status"), mode_batch=True, mode_chunk=2, **AZIMUTH),     # (chunks of 2 and 1 modes)
    # (tauStar_aer quartered once more: with T_AER the forward-peaked aerosol leaves column 1 with status 1)
    "azimuth_loop_eva_device": lambda: _batch(("I_azimuth", "mode_status"), T_AER / 4, azimuths=[0, 1.0, 3.0], n_modes=2,
                                              aer_phase_fun="eva", mie_aer=dict(device=True)),
    "view_azimuth_exact": lambda: _batch(VIEW_AZIMUTH_OUT, view_first_order="exact", **VIEW_AZIMUTH),
    "view_azimuth_modes": lambda: _batch(VIEW_AZIMUTH_OUT, view_first_order="modes", **VIEW_AZIMUTH),
    "device_plain": lambda: _device(),
    "device_spherical": lambda: _device(beam="spherical"),
    "device_thermal": lambda: _device(**THERMAL, **GREY),
    "layers_solar": lambda: _layers(),
    "layers_spherical": lambda: _layers(beam="spherical"),
    "layers_thermal": lambda: _layers(tauStar_atm=0.125, alb_atm=0.5, **THERMAL),
    "toa_net_flux_plane": lambda: _toa_net_flux(),
    "toa_net_flux_spherical": lambda: _toa_net_flux(beam="spherical"),
    "thermal_toa_flux": _thermal_toa_flux,
    "band_thermal": _band_thermal,
    "band_solar": _band_solar,
    "spectrum_loop": lambda: _spectrum(False),
    "spectrum_one_batch": lambda: _spectrum(True),
    "brdf_lambertian": lambda: _batch(BRDF_OUT, T_AER / 2, surface="brdf", brdf="lambertian"),
    "brdf_rpv": lambda: _rpv(BRDF_OUT),
    "brdf_rpv_azimuth": lambda: _rpv(BRDF_OUT + ("I_azimuth", "mode_status"), brdf_modes=True, **AZIMUTH),
    "brdf_rpv_view": lambda: _rpv(BRDF_VIEW_OUT, view_mu=VIEW_MU, brdf_view=True),
    "brdf_rpv_view_azimuth_exact": lambda: _rpv(BRDF_VIEW_AZIMUTH_OUT, view_first_order="exact", brdf_view=True, **VIEW_AZIMUTH),
    "brdf_rpv_view_azimuth_modes": lambda: _rpv(BRDF_VIEW_AZIMUTH_OUT, view_first_order="modes", brdf_view=True, **VIEW_AZIMUTH),
    "brdf_stages": _brdf_stages,
}


def run(name):
    """({output name: SHA-256 of its bytes}, the statuses of the case's solves as one flat list), from fresh handles, which are
    closed again.  The flux drivers of forcing, thermal and bands raise on a status of their own."""
    fresh()
    try:
        out, status = CASES[name]()
    finally:
        fresh()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {k: sha(v) for k, v in out.items()}, [int(x) for st in status for x in np.ravel(st)]
