"""Channel radiances and brightness temperatures in the band drivers on the device (csrc/brightness.hip, csrc/api_bands.hip,
sosrt/bands.py) through the C ABI and the drivers: the brightness kernel against the NumPy model of
tests/band_view_np.py, its NaN cases, refusals and the handle's state; `band_thermal(view_mu=...)` and `band_solar(view_mu=...)`
against the per-point path (one `SOS_Aer_batch(view_mu=...)` per spectral point, summed in NumPy), against the hand chain of
`Solver` calls bit for bit, over `points_per_solve`, with and without `gas_tau`; and the existing paths on the cached handle."""
import ctypes
import functools

import numpy as np
import pytest

import band_view_np as V
import bands_np as M
import sos_oracle as O
import thermal_np as T
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

RTOL = 1e-10         # the view terms against the per-point path, of the maximum (the bar of test_gpu_bands.py for the fluxes)
BAR = 1e-12          # T_b relative, device against the model (tests/test_band_view_host.py: why)
GUARD = 16           # doubles after the output, which must stay as they were


def _torch():
    return pytest.importorskip("torch")


def dev(a, dtype=np.float64):
    torch = _torch()
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(torch.device("cuda", 0))


def dfull(shape, fill=np.nan):
    torch = _torch()
    return torch.full(tuple(shape), fill, dtype=torch.float64, device=torch.device("cuda", 0))


def host(t, s):
    s.synchronize()
    return t.cpu().numpy()


def sync():
    _torch().cuda.synchronize()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- a. the kernel alone against the model --------------------------------------------------------------------------------------
BANDS = [p[:2] for p in M.THERMAL_POINTS] + [(float(a), float(b)) for a, b in M.LW_BANDS]
# (C, K, M): one element; a wave that is not full; exactly one wave per column; a column boundary inside a wave; five waves per
# column and sixteen bands; the most bands the entry takes
SHAPES = [(1, 1, 1), (3, 5, 63), (2, 5, 64), (2, 5, 65), (5, 16, 257), (2, 64, 4)]
SENTINEL = -7.0


def run_bt(s, R, lo, hi, w=None):
    C, Mm = R.shape
    d_R, d_w = dev(R), None if w is None else dev(w)
    d_T = dfull((C * Mm + GUARD,), SENTINEL)
    sync()
    s.brightness_temperature_device(d_R.data_ptr(), d_T.data_ptr(), lo, hi, C, Mm, 0 if d_w is None else d_w.data_ptr())
    out = host(d_T, s)
    assert np.all(out[C * Mm:] == SENTINEL), "the stage wrote past [C][M]"
    return out[:C * Mm].reshape(C, Mm)


def kernel_case(C, K, Mm, null_weights):
    rng = np.random.default_rng(1000 * C + 10 * K + Mm)
    lo = np.array([BANDS[k % len(BANDS)][0] for k in range(K)])
    hi = np.array([BANDS[k % len(BANDS)][1] for k in range(K)])
    Tt = rng.uniform(150.0, 350.0, (C, Mm))
    if C * Mm >= 3:
        Tt.reshape(-1)[[1, -1]] = 60.0, 3000.0
    w = None
    if not null_weights:
        w = rng.uniform(0.2, 2.0, (K, C))
        if K > 1:
            w[K // 2, C - 1] = 0.0
    ww = np.ones((K, C)) if w is None else w
    R = np.zeros((C, Mm))
    for k in range(K):
        R += ww[k][:, None] * M.planck_band(Tt, lo[k], hi[k])
    return lo, hi, w, Tt, R


@pytest.mark.parametrize("null_weights", [False, True], ids=["weights", "null weights"])
@pytest.mark.parametrize("C,K,Mm", SHAPES, ids=lambda v: str(v))
def test_kernel_against_the_model(C, K, Mm, null_weights):
    lo, hi, w, Tt, R = kernel_case(C, K, Mm, null_weights)
    s = Solver(24, 32, max_batch=1)
    got = run_bt(s, R, lo, hi, w)
    s.close()
    ref = V.brightness_temperature(R, lo, hi, None if w is None else w[:, :, None])
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    e_model, e_trip = float(np.max(np.abs(got / ref - 1))), float(np.max(np.abs(got / Tt - 1)))
    print("C=%d K=%d M=%d %s: T_b device vs model %.3e, round trip %.3e" % (C, K, Mm, "null weights" if w is None else "weights",
                                                                         e_model, e_trip))
    assert e_model <= BAR and e_trip <= BAR


# ---- b. the kernel's edge cases ---------------------------------------------------------------------------------------------------
def test_every_nan_case_in_its_own_element():
    C, K, Mm = 4, 5, 8
    lo, hi, w, Tt, R = kernel_case(C, K, Mm, False)
    s = Solver(24, 32, max_batch=1)
    clean = run_bt(s, R, lo, hi, w)
    assert np.all(np.isfinite(clean))
    top = V.channel(np.array([1e5]), lo, hi, w[:, 2:3])[0][0]
    bad = R.copy()
    where = {(0, 1): 0.0, (0, 3): -1.0, (1, 0): np.nan, (1, 5): np.inf, (1, 6): -np.inf, (2, 2): 2.0 * top, (2, 7): top}
    for (c, m), v in where.items():
        bad[c, m] = v
    for col3 in (np.zeros(K), np.where(np.arange(K) == 1, -0.5, 1.0)):        # all zero; one negative
        wb = w.copy()
        wb[:, 3] = col3
        got = run_bt(s, bad, lo, hi, wb)
        nan = np.zeros((C, Mm), dtype=bool)
        nan[3, :] = True
        for cm in where:
            nan[cm] = True
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan], clean[~nan]), "a NaN element changed a neighbour"
    # the model has the same NaNs
    assert np.array_equal(np.isnan(V.brightness_temperature(bad, lo, hi, wb[:, :, None])), nan)
    s.close()


def test_a_column_does_not_depend_on_its_batch_or_its_neighbours():
    C, K, Mm = 3, 5, 65
    lo, hi, w, Tt, R = kernel_case(C, K, Mm, False)
    s = Solver(24, 32, max_batch=1)
    full = run_bt(s, R, lo, hi, w)
    alone = run_bt(s, R[1:2], lo, hi, w[:, 1:2])                             # C = 1
    assert np.array_equal(alone[0], full[1])
    folded = run_bt(s, R[1].reshape(5, 13), lo, hi, np.tile(w[:, 1:2], (1, 5)))  # the same values as five columns of M = 13
    assert np.array_equal(folded.reshape(-1), full[1])
    other = w.copy()
    other[:, 0], other[:, 2] = 3.0, np.where(np.arange(K) == 0, -1.0, 0.5)   # the neighbours' weights, one of them refused
    got = run_bt(s, R, lo, hi, other)
    assert np.array_equal(got[1], full[1]) and np.all(np.isnan(got[2])) and not np.array_equal(got[0], full[0])
    s.close()


def test_refusals_leave_the_output_untouched():
    from sosrt import _lib
    C, K, Mm = 2, 3, 7
    lo, hi = np.array([350.0, 630.0, 820.0]), np.array([500.0, 700.0, 980.0])
    s = Solver(24, 32, max_batch=1)
    d_R, d_w, d_T = dev(np.ones((C, Mm))), dev(np.ones((K, C))), dfull((C * Mm + GUARD,), SENTINEL)
    sync()
    bt = lambda **k: s.brightness_temperature_device(k.get("R", d_R.data_ptr()), k.get("T", d_T.data_ptr()), k.get("lo", lo),
                                                     k.get("hi", hi), k.get("C", C), k.get("M", Mm), d_w.data_ptr())

    def refused(call, word):
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), str(ei.value)
        assert np.all(host(d_T, s) == SENTINEL), "a refused call wrote to the output"

    for name in ("C", "M"):
        for v in (0, -1):
            refused(lambda: bt(**{name: v}), name + "=")
    refused(lambda: bt(lo=[], hi=[]), "K=0")
    lo65 = 100.0 + 20.0 * np.arange(65)
    refused(lambda: bt(lo=lo65, hi=lo65 + 20.0), "at most 64")
    refused(lambda: bt(R=0), "null")
    refused(lambda: bt(T=0), "null")
    for v in (float("nan"), float("inf"), -1.0):
        refused(lambda: bt(lo=[350.0, v, 820.0]), "finite")
    refused(lambda: bt(hi=[500.0, float("inf"), 980.0]), "finite")
    refused(lambda: bt(hi=[500.0, 630.0, 980.0]), "nu_hi must be > nu_lo")
    refused(lambda: bt(hi=[500.0, 600.0, 980.0]), "nu_hi must be > nu_lo")
    # null edge arrays, which the binding cannot send: the symbol itself
    vp, p = ctypes.c_void_p, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    raw = lambda lo_, hi_: _lib.check(_lib.lib().sosrt_brightness_temperature_dev(s._h, C, K, Mm, lo_, hi_, vp(d_w.data_ptr()),
                                                                                 vp(d_R.data_ptr()), vp(d_T.data_ptr())))
    refused(lambda: raw(None, p(hi)), "null")
    refused(lambda: raw(p(lo), None), "null")
    # the stage still works on this handle, and then writes; 64 bands are taken
    bt()
    out = host(d_T, s)
    assert np.all(np.isfinite(out[:C * Mm])) and np.all(out[C * Mm:] == SENTINEL)
    d_w = dev(np.ones((64, C)))
    sync()
    bt(lo=lo65[:64], hi=lo65[:64] + 20.0)
    assert np.all(np.isfinite(host(d_T, s)[:C * Mm]))
    s.close()


def test_the_stage_leaves_the_handle_untouched():
    cols = [T.column(O, 32, 24, 0.1, 1.0, 0.0, 0.3, 0.6), T.column(O, 32, 24, 0.3, 1.0, 0.0, 0.3, 0.6)]
    L, c0 = 24, cols[0]
    z = T.altitudes(L)
    s = Solver(L, 32, max_batch=2, max_orders=64)
    s.set_grid(c0.mu)
    s.set_phase(c0.P_atm, c0.P_aer)
    col = lambda f: [f(c) for c in cols]
    s.set_columns(col(lambda c: c.idx_up), col(lambda c: c.idx_down), col(lambda c: c.mu0), col(lambda c: c.grd_alb),
                  col(lambda c: c.alb_atm), col(lambda c: c.alb_aer), col(lambda c: c.dtau_atm), col(lambda c: c.dtau_aer),
                  col(lambda c: c.tauStar_tot), surface=c0.surface)
    tau = np.stack([c.tau for c in cols])
    P0a, P0r = np.stack([c.P0_atm for c in cols]), np.stack([c.P0_aer for c in cols])
    f0 = s.first_order(tau, P0a, P0r)
    r0 = s.solve(tau, P0a, P0r)
    assert np.all(r0.status == 0)
    e0 = s.epilogue(z_profile=z)
    lo, hi, w, Tt, R = kernel_case(3, 5, 63, False)
    run_bt(s, R, lo, hi, w)
    e1 = s.epilogue(z_profile=z)                                 # the resident field and tau: same bytes
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    r1 = s.solve(tau, P0a, P0r)                                  # the columns and the phase state: the same solve, bit for bit
    assert np.array_equal(r0.I, r1.I) and np.array_equal(r0.n, r1.n)
    assert np.array_equal(s.first_order(tau, P0a, P0r), f0)
    s.close()


# ---- c. band_thermal(view_mu=...) ---------------------------------------------------------------------------------------------------
GEOM = dict(z0=M.Z0, nb_layers=M.L_, nb_angles=M.N_, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=T.G_AER)
VIEW = dict(view_mu=np.array([0.05, 0.5, 1.0]), view_levels=[0, 7, -1])
NV = 3
VIEW_FIELDS = ("I_view_first", "I_view_scattered", "I_view")
EPI = ("flux_down", "flux_up", "heating_rate", "net_toa")
W_KC = np.array([[0.5, 1.0], [1.0, 1.0], [2.0, 0.25], [1.0, 3.0], [0.3, 1.0]])
# a stepped gas per point: absorption between the rows 4 and 9, a trace elsewhere, a strength per point
_STEP = np.concatenate(([0.0], np.cumsum(np.where((np.arange(1, M.L_) >= 4) & (np.arange(1, M.L_) <= 9), 0.05, 0.004))))
GAS_THERMAL = _STEP[None, :] * np.array([1.0, 2.0, 0.5, 1.5, 0.25])[:, None]
GAS_SOLAR = _STEP[None, :] * np.array([0.4, 1.0, 2.0, 0.1])[:, None]


def thermal_args():
    pts = M.THERMAL_POINTS
    pp = lambda i: np.array([p[i] for p in pts])
    t_aer = np.stack([pp(4), np.zeros(len(pts))], axis=1)         # column 0 with the layer, column 1 without
    return ((pp(0), pp(1)), M.temperature_profile(M.L_), M.T_SURFACE, t_aer, M.RHO), dict(tauStar_atm=pp(2), alb_atm=pp(3), alb_aer=pp(5), **GEOM)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def thermal_per_point(gas):
    """The per-point path: one thermal view call of the two columns per band, fed the model's normalised source.
    (scale [K], first [K, 2, nlev, 2V], scattered [K, 2, nlev, 2V])"""
    from sosrt import main
    scale, first, scat = [], [], []
    for k, (lo, hi, t_atm, w_atm, t_aer, w_aer, _, _) in enumerate(M.THERMAL_POINTS):
        b, bs, sc = M.planck_bands(M.temperature_profile(M.L_), M.T_SURFACE, [lo], [hi], True)
        kw = dict(gas_tau=GAS_THERMAL[k], gas_view=True) if gas else {}
        r = main.SOS_Aer_batch(0.5, [t_aer, 0.0], M.RHO, tauStar_atm=t_atm, alb_atm=w_atm, alb_aer=w_aer, source="thermal",
                               planck=b[0, 0], planck_surface=float(bs[0, 0]), **VIEW, **GEOM, **kw)
        assert np.all(r.status == 0)
        scale.append(float(sc[0, 0]))
        first.append(r.I_view_first)
        scat.append(r.I_view_scattered)
    return _frozen(np.array(scale), np.stack(first), np.stack(scat))


def thermal_hand_chain(gas, weights, quad="grid"):
    """What band_thermal(view_mu=...) stands for with all points in one solve, call by call on the cached handle: the Planck
    stage, the columns, (the weights,) the emission, the solve from it, the rows at the lanes, the emission at the lanes and the
    scattered term on the resident field, the two reduces, their sum and its brightness temperature."""
    from sosrt import main
    torch = _torch()
    pos, kw = thermal_args()
    (lo, hi), Tp, Ts, t_aer, rho = pos
    K, C, L = 5, 2, M.L_
    B = K * C
    col = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64)[:, None], (K, C)).reshape(B)
    ns = None if gas is None else main._gas_args(np.repeat(gas, C, axis=0), B, L)
    s = main.get_solver(L, M.N_, B, 256, 0)
    with main._on_torch_stream(s, 0) as dv:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dv)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dv)
        d_T, d_Ts, d_w = up(np.tile(Tp, (C, 1))), up(np.full(C, Ts)), up(weights)
        d_pl, d_bs, d_sc = new(K, C, L), new(K, C), new(K, C)
        s.planck_bands_device(d_T.data_ptr(), d_Ts.data_ptr(), lo, hi, d_pl.data_ptr(), d_bs.data_ptr(), d_sc.data_ptr(), C=C)
        s.synchronize()
    s, tau, _, _, _, _, _, _ = main._prepare_batch(np.full(B, 0.5), t_aer.reshape(B), np.full(B, rho), col(kw["tauStar_atm"]),
                                                   col(kw["alb_atm"]), col(kw["alb_aer"]), M.Z0, 25, 17, L, M.N_, "rayleigh", 0.0, "hg",
                                                   T.G_AER, None, None, None, None, None, None, "specular", 256, 0, gas=ns)
    mv, lev = VIEW["view_mu"], [x % L for x in VIEW["view_levels"]]
    sgn = np.concatenate((-mv, mv))
    V2 = len(sgn)
    with main._on_torch_stream(s, 0) as dv:
        d_tau, d_mu0 = up(tau), up(np.full(B, 0.5))
        d_I0, d_I = new(B, L, s.D), new(B, L, s.D)
        d_n, d_st = torch.zeros(B, dtype=torch.int32, device=dv), torch.zeros(B, dtype=torch.int32, device=dv)
        d_first, d_scat = new(B, len(lev), V2), new(B, len(lev), V2)
        try:
            if ns is not None:
                d_rw = up(ns.w)
                s.set_row_weights_device(d_rw.data_ptr(), d_rw.data_ptr(), B=B)
                s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr(), B=B)
            else:
                s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr(), B=B)
            s.solve_device(d_tau.data_ptr(), 0, 0, d_I.data_ptr(), d_I1=d_I0.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            rows = []
            for kind, g in (("rayleigh", 0.0), ("hg", T.G_AER)):
                rw, p0 = new(V2, s.D), new(B, V2)
                torch.cuda.current_stream(dv).synchronize()
                s.phase_rows_device(kind, sgn, rw.data_ptr(), g)
                s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p0.data_ptr(), B, g)
                rows.append(rw)
            if ns is not None:
                s.emission_view_profile_device(mv, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), lev, d_first.data_ptr(), B=B)
                s.view_radiance_profile_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), lev,
                                               d_scat.data_ptr(), quadrature=quad, B=B)
            else:
                s.emission_view_device(mv, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), lev, d_first.data_ptr(), B=B)
                s.view_radiance_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), lev,
                                       d_scat_out=d_scat.data_ptr(), quadrature=quad, B=B)
            s.synchronize()
        finally:
            s.set_row_weights_device(0, 0)
        Mm = len(lev) * V2
        s_first, s_scat = new(C, len(lev), V2), new(C, len(lev), V2)
        for x, o in ((d_first, s_first), (d_scat, s_scat)):
            s.band_reduce_device(x.data_ptr(), o.data_ptr(), C, K, Mm, d_w.data_ptr(), d_sc.data_ptr())
        d_view = s_first + s_scat
        d_Tb = new(C, len(lev), V2)
        s.brightness_temperature_device(d_view.data_ptr(), d_Tb.data_ptr(), lo, hi, C, Mm, d_w.data_ptr())
        s.synchronize()
        out = {k: v.cpu().numpy() for k, v in dict(I_view_first=s_first, I_view_scattered=s_scat, I_view=d_view,
                                                   brightness_temperature=d_Tb, n=d_n).items()}
    out["n"] = out["n"].reshape(K, C)
    return out


def _same_bits(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        assert x is None or np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("gas", [False, True], ids=["no gas", "gas_tau"])
def test_band_thermal_views(gas):
    from sosrt import bands
    pos, kw = thermal_args()
    if gas:
        kw = dict(kw, gas_tau=GAS_THERMAL)
    scale, first, scat = thermal_per_point(gas)
    one = np.ones((5, 2))
    r = bands.band_thermal(*pos, **kw, **VIEW, per_point=True)
    assert np.array_equal(r.view_mu_signed, np.concatenate((-VIEW["view_mu"], VIEW["view_mu"])))
    assert r.I_view.shape == r.brightness_temperature.shape == (2, 3, 2 * NV) and r.point_I_view.shape == (5, 2, 3, 2 * NV)
    ref = dict(I_view_first=V.channel_sum(first, one, np.tile(scale[:, None], (1, 2))),
               I_view_scattered=V.channel_sum(scat, one, np.tile(scale[:, None], (1, 2))))
    ref["I_view"] = ref["I_view_first"] + ref["I_view_scattered"]
    for k in VIEW_FIELDS:
        e = _rel(getattr(r, k), ref[k])
        print("band_thermal(view_mu%s) %s vs the per-point path: %.3e of its maximum" % (", gas_tau" if gas else "", k, e))
        assert e <= RTOL, k
    assert np.array_equal(r.I_view, r.I_view_first + r.I_view_scattered)
    e = _rel(r.point_I_view, (first + scat) * scale[:, None, None, None])
    print("point_I_view vs the per-point calls: %.3e of its maximum" % e)
    assert e <= RTOL
    # the hand chain of Solver calls on the same batch: bit for bit
    chain = thermal_hand_chain(GAS_THERMAL if gas else None, one)
    for k in VIEW_FIELDS + ("brightness_temperature", "n"):
        assert np.array_equal(getattr(r, k), chain[k], equal_nan=True), k
    # the chunking; the fluxes are those of the call without view_mu; want=() leaves only the views
    plain = bands.band_thermal(*pos, **kw, weights=W_KC)
    runs = [bands.band_thermal(*pos, **kw, **VIEW, weights=W_KC, points_per_solve=P, per_point=True) for P in (1, 2, 5)]
    for other in runs[1:]:
        _same_bits(other, runs[0], VIEW_FIELDS + EPI + ("brightness_temperature", "point_I_view", "point_net_toa", "n", "status", "scale"))
    _same_bits(runs[0], plain, EPI + ("n", "status", "scale"))
    only = bands.band_thermal(*pos, **kw, **VIEW, weights=W_KC, want=(), points_per_solve=2)
    _same_bits(only, runs[0], VIEW_FIELDS + ("brightness_temperature", "n", "status"))
    assert all(getattr(only, k) is None for k in EPI) and only.point_I_view is None and only.point_net_toa is None
    # [K, C] weights against the NumPy sum
    w_first = V.channel_sum(first, W_KC, np.tile(scale[:, None], (1, 2)))
    assert _rel(runs[0].I_view_first, w_first) <= RTOL
    assert _rel(runs[0].I_view, w_first + V.channel_sum(scat, W_KC, np.tile(scale[:, None], (1, 2)))) <= RTOL
    assert np.array_equal(thermal_hand_chain(GAS_THERMAL if gas else None, W_KC)["I_view"], runs[0].I_view)
    # brightness=False leaves it out and changes nothing else
    off = bands.band_thermal(*pos, **kw, **VIEW, weights=W_KC, brightness=False)
    assert off.brightness_temperature is None and np.array_equal(off.I_view, runs[0].I_view)


def test_brightness_temperature_of_the_channel():
    """The channel of the five points with the driver's default weights (ones).  The bounds are the profile's own, 216.5 K aloft
    and 288 K at the ground; they are the channel's, not every point's: the layer scatters, and a point whose layer looks into a
    cold sky from the isothermal stratosphere has a source below B(216.5 K) there -- 820-980 cm^-1 alone comes out at 216.33 K at
    mu = 0.05 (and a channel that weighs that point twice, W_KC, at 216.43 K), the column without the layer at 216.87 K."""
    from sosrt import bands
    pos, kw = thermal_args()
    lo, hi = pos[0]
    for w in (W_KC, np.ones((5, 2))):
        for gas in (None, GAS_THERMAL):
            x = bands.band_thermal(*pos, **kw, **VIEW, weights=w, want=(), gas_tau=gas)
            ref = V.brightness_temperature(x.I_view, lo, hi, w[:, :, None, None])
            ok = np.isfinite(ref)
            assert np.array_equal(np.isnan(x.brightness_temperature), ~ok)
            e = float(np.max(np.abs(x.brightness_temperature[ok] / ref[ok] - 1)))
            print("brightness_temperature vs the model on the driver's I_view: %.3e" % e)
            assert e <= BAR
    r = bands.band_thermal(*pos, **kw, **VIEW, want=())
    g = bands.band_thermal(*pos, **kw, **VIEW, want=(), gas_tau=GAS_THERMAL)
    for x in (r, g):
        up = x.brightness_temperature[:, 0, NV:]                 # TOA, the upward lanes
        print("TOA upward T_b (mu = 0.05, 0.5, 1): %s" % up.tolist())
        assert np.all(up > 216.5) and np.all(up < 288.0)
        assert np.all(x.I_view[:, 0, :NV] == 0.0) and np.all(np.isnan(x.brightness_temperature[:, 0, :NV]))   # nothing comes down at the top
        assert np.all(up[:, 0] < up[:, 2]), "limb darkening under a lapse rate"
    assert np.all(g.brightness_temperature[:, 0, 2 * NV - 1] < r.brightness_temperature[:, 0, 2 * NV - 1]), "the gas cools the nadir"


def test_isothermal_column_has_its_own_temperature():
    from sosrt import bands
    lo, hi = np.array([350.0, 820.0, 1180.0]), np.array([500.0, 980.0, 1390.0])
    r = bands.band_thermal((lo, hi), np.full(M.L_, 260.0), 260.0, 0.0, 0.0, tauStar_atm=[2.0, 0.3, 1.0], alb_atm=0.0, alb_aer=0.5,
                           weights=[1.0, 0.5, 2.0], want=(), **VIEW, **GEOM)
    up = r.brightness_temperature[0, 0, NV:]
    e = float(np.max(np.abs(up / 260.0 - 1)))
    print("isothermal 260 K: TOA upward T_b %s, %.3e from 260 K" % (up.tolist(), e))
    assert e <= 1e-10


# ---- d. band_solar(view_mu=...) ------------------------------------------------------------------------------------------------------
def solar_args():
    pts = M.SOLAR_POINTS
    pp = lambda i: np.array([p[i] for p in pts])
    return ((np.array(M.SOLAR_WEIGHTS), np.array(M.SOLAR_MU0), pp(2), M.RHO), dict(tauStar_atm=pp(0), alb_atm=pp(1), alb_aer=pp(3), **GEOM))


@functools.lru_cache(maxsize=None)
def solar_per_point(gas):
    """One view call of the two suns per point: (first [K, 2, nlev, 2V], scattered [K, 2, nlev, 2V])"""
    from sosrt import main
    first, scat = [], []
    for k, (t_atm, w_atm, t_aer, w_aer) in enumerate(M.SOLAR_POINTS):
        kw = dict(gas_tau=GAS_SOLAR[k], gas_view=True) if gas else {}
        r = main.SOS_Aer_batch(np.array(M.SOLAR_MU0), t_aer, M.RHO, tauStar_atm=t_atm, alb_atm=w_atm, alb_aer=w_aer, **VIEW, **GEOM, **kw)
        assert np.all(r.status == 0)
        first.append(r.I_view_first)
        scat.append(r.I_view_scattered)
    return _frozen(np.stack(first), np.stack(scat))


def solar_hand_chain(gas, weights, quad="grid"):
    """What band_solar(view_mu=...) stands for with all points in one solve, call by call on the cached handle."""
    from sosrt import main
    torch = _torch()
    pos, kw = solar_args()
    K, C, L = 4, 2, M.L_
    B = K * C
    col = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64)[:, None], (K, C)).reshape(B)
    mu0 = np.tile(np.array(M.SOLAR_MU0), K)
    ns = None if gas is None else main._gas_args(np.repeat(gas, C, axis=0), B, L)
    s, tau, P0a, P0r, _, _, _, _ = main._prepare_batch(mu0, col(pos[2]), np.full(B, M.RHO), col(kw["tauStar_atm"]), col(kw["alb_atm"]),
                                                       col(kw["alb_aer"]), M.Z0, 25, 17, L, M.N_, "rayleigh", 0.0, "hg", T.G_AER, None,
                                                       None, None, None, None, None, "specular", 256, 0, gas=ns)
    mv, lev = VIEW["view_mu"], [x % L for x in VIEW["view_levels"]]
    sgn = np.concatenate((-mv, mv))
    V2 = len(sgn)
    with main._on_torch_stream(s, 0) as dv:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dv)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dv)
        d_tau, d_mu0, d_w, d_P0a, d_P0r = up(tau), up(mu0), up(weights), up(P0a), up(P0r)
        d_I1, d_I = new(B, L, s.D), new(B, L, s.D)
        d_n, d_st = torch.zeros(B, dtype=torch.int32, device=dv), torch.zeros(B, dtype=torch.int32, device=dv)
        d_first, d_scat = new(B, len(lev), V2), new(B, len(lev), V2)
        try:
            if ns is not None:
                d_rw, d_sig = up(ns.w), up(tau / mu0[:, None])
                s.set_row_weights_device(d_rw.data_ptr(), d_rw.data_ptr(), B=B)
                s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr(), B=B)
                s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_I1=d_I1.data_ptr(),
                               d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            else:
                s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr(),
                               d_status=d_st.data_ptr())
            rows, p0rows = [], []
            for kind, g in (("rayleigh", 0.0), ("hg", T.G_AER)):
                rw, p0 = new(V2, s.D), new(B, V2)
                torch.cuda.current_stream(dv).synchronize()
                s.phase_rows_device(kind, sgn, rw.data_ptr(), g)
                s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p0.data_ptr(), B, g)
                rows.append(rw)
                p0rows.append(p0)
            if ns is not None:
                s.view_first_order_profile_device(mv, d_tau.data_ptr(), d_sig.data_ptr(), p0rows[0].data_ptr(), p0rows[1].data_ptr(), lev,
                                                  d_first.data_ptr(), B=B)
                s.view_radiance_profile_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), lev,
                                               d_scat.data_ptr(), quadrature=quad, B=B)
            else:
                s.view_radiance_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), lev,
                                       d_scat_out=d_scat.data_ptr(), d_first_out=d_first.data_ptr(), d_p0rows_atm=p0rows[0].data_ptr(),
                                       d_p0rows_aer=p0rows[1].data_ptr(), quadrature=quad, B=B)
            s.synchronize()
        finally:
            s.set_row_weights_device(0, 0)
        Mm = len(lev) * V2
        s_first, s_scat = new(C, len(lev), V2), new(C, len(lev), V2)
        for x, o in ((d_first, s_first), (d_scat, s_scat)):
            s.band_reduce_device(x.data_ptr(), o.data_ptr(), C, K, Mm, d_w.data_ptr(), 0)
        d_view = s_first + s_scat
        s.synchronize()
        out = {k: v.cpu().numpy() for k, v in dict(I_view_first=s_first, I_view_scattered=s_scat, I_view=d_view, n=d_n).items()}
    out["n"] = out["n"].reshape(K, C)
    return out


@pytest.mark.parametrize("gas", [False, True], ids=["no gas", "gas_tau"])
def test_band_solar_views(gas):
    from sosrt import bands
    pos, kw = solar_args()
    if gas:
        kw = dict(kw, gas_tau=GAS_SOLAR)
    first, scat = solar_per_point(gas)
    w = np.tile(np.array(M.SOLAR_WEIGHTS)[:, None], (1, 2))
    r = bands.band_solar(*pos, **kw, **VIEW, per_point=True)
    assert r.brightness_temperature is None and r.scale is None
    assert np.array_equal(r.view_mu_signed, np.concatenate((-VIEW["view_mu"], VIEW["view_mu"])))
    ref = dict(I_view_first=V.channel_sum(first, w), I_view_scattered=V.channel_sum(scat, w))
    ref["I_view"] = ref["I_view_first"] + ref["I_view_scattered"]
    for k in VIEW_FIELDS:
        e = _rel(getattr(r, k), ref[k])
        print("band_solar(view_mu%s) %s vs the per-point path: %.3e of its maximum" % (", gas_tau" if gas else "", k, e))
        assert e <= RTOL, k
    assert _rel(r.point_I_view, first + scat) <= RTOL
    chain = solar_hand_chain(GAS_SOLAR if gas else None, w)
    for k in VIEW_FIELDS + ("n",):
        assert np.array_equal(getattr(r, k), chain[k]), k
    plain = bands.band_solar(*pos, **kw)
    for P in (1, 3):
        other = bands.band_solar(*pos, **kw, **VIEW, per_point=True, points_per_solve=P)
        _same_bits(other, r, VIEW_FIELDS + EPI + ("point_I_view", "point_net_toa", "n", "status"))
    _same_bits(r, plain, EPI + ("n", "status"))
    only = bands.band_solar(*pos, **kw, **VIEW, want=(), points_per_solve=3)
    _same_bits(only, r, VIEW_FIELDS + ("n", "status"))
    assert all(getattr(only, k) is None for k in EPI)
    # [K, C] weights
    w2 = w * np.array([1.0, 0.5])
    r2 = bands.band_solar(w2, *pos[1:], **kw, **VIEW, want=())
    assert _rel(r2.I_view, V.channel_sum(first, w2) + V.channel_sum(scat, w2)) <= RTOL


def test_band_depth_at_nadir():
    from sosrt import bands
    pos, kw = solar_args()
    bare = bands.band_solar(*pos, **kw, **VIEW, want=())
    band = bands.band_solar(*pos, **kw, **VIEW, want=(), gas_tau=GAS_SOLAR)
    nadir = 2 * NV - 1                                           # TOA, mu = 1, upward
    print("summed nadir TOA I_view: %s without the gas, %s with it" % (bare.I_view[:, 0, nadir].tolist(), band.I_view[:, 0, nadir].tolist()))
    assert np.all(band.I_view[:, 0, nadir] < bare.I_view[:, 0, nadir]) and np.all(band.I_view[:, 0, nadir] > 0)


# ---- e. the existing paths on the cached handle -----------------------------------------------------------------------------------------
def test_existing_paths_keep_their_bits_after_a_band_view_call():
    from sosrt import bands, main
    t_aer, rho = np.array([0.3, 0.12, 0.0]), np.array([0.1, 0.3, 0.0])
    drv = dict(GEOM, tauStar_atm=1.0, alb_atm=0.1, alb_aer=0.6)
    gas3 = _STEP[None, :] * np.array([1.0, 0.5, 2.0])[:, None]
    pos, kw = thermal_args()
    spos, skw = solar_args()

    def calls():
        a = main.SOS_Aer_batch(0.5, t_aer, rho, **VIEW, **drv)
        b = main.SOS_Aer_batch(0.5, t_aer, rho, gas_tau=gas3, gas_view=True, **VIEW, **drv)
        c = main.SOS_Aer_batch(0.5, t_aer, rho, source="thermal", planck=T.planck_profile(M.L_), planck_surface=1.0, **VIEW, **drv)
        d = bands.band_thermal(*pos, **kw, points_per_solve=2)
        e = bands.band_solar(*spos, **skw)
        return [getattr(x, k) for x in (a, b, c) for k in ("I", "n") + VIEW_FIELDS] + [getattr(x, k) for x in (d, e) for k in EPI + ("n",)]

    before = calls()
    for gas in (None, GAS_THERMAL):
        bands.band_thermal(*pos, **kw, **VIEW, gas_tau=gas, points_per_solve=2)
        assert all(np.array_equal(x, y) for x, y in zip(calls(), before))
    for gas in (None, GAS_SOLAR):
        bands.band_solar(*spos, **skw, **VIEW, gas_tau=gas, points_per_solve=3)
        assert all(np.array_equal(x, y) for x, y in zip(calls(), before))
