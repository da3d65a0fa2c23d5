"""Band integration on the device (csrc/bands.hip, csrc/api_bands.hip, sosrt/bands.py) through the C ABI: the
Planck stage and the reduce stage against the NumPy model of tests/bands_np.py (which tests/test_bands_host.py pins to quadrature
and to the oracle), every refusal, the handle's state, and the band drivers against the per-point path -- one batched solve per
spectral point, its epilogue, and a NumPy weighted sum."""
import functools

import numpy as np
import pytest

import bands_np as M
import sos_oracle as O
import thermal_np as T
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

RTOL = 1e-10


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


GUARD = 16                                                      # doubles after every output, which must stay NaN


# ---- a. the Planck stage against the model ---------------------------------------------------------------------------------------
# the five bands of the thermal table, both edges below the split (at 320 K), across it (at 288 K), the far tail (at 180 K), all of it
BANDS = [p[:2] for p in M.THERMAL_POINTS] + [(10.0, 100.0), (100.0, 350.0), (2600.0, 3250.0), (0.0, 1e6)]
# (C, K, L): one wave; one of everything; L + 1 = 71 and 131 lanes (two and three waves: the maximum crosses waves through LDS);
# 70 columns; 301 values on 256 lanes (the strided walk); 70 bands (two launches of 64 and 6)
PLANCK_SHAPES = [(3, 5, 24), (1, 1, 24), (2, 3, 70), (70, 2, 24), (2, 2, 130), (2, 2, 300), (1, 70, 24)]


def run_planck(s, T_lev, T_sfc, lo, hi, normalise, scale_out=True):
    C, L = T_lev.shape
    K = len(lo)
    d_T, d_Ts = dev(T_lev), dev(T_sfc)
    d_b, d_bs, d_sc = dfull((K * C * L + GUARD,)), dfull((K * C + GUARD,)), dfull((K * C + GUARD,))
    sync()
    s.planck_bands_device(d_T.data_ptr(), d_Ts.data_ptr(), lo, hi, d_b.data_ptr(), d_bs.data_ptr(),
                          d_sc.data_ptr() if scale_out else 0, C=C, normalise=normalise)
    b, bs, sc = host(d_b, s), host(d_bs, s), host(d_sc, s)
    for a, n in ((b, K * C * L), (bs, K * C), (sc, K * C)):
        assert np.all(np.isnan(a[n:])), "the stage wrote past an output"
    return b[:K * C * L].reshape(K, C, L), bs[:K * C].reshape(K, C), sc[:K * C].reshape(K, C)


def check_planck(T_lev, T_sfc, lo, hi, label):
    s = Solver(T_lev.shape[1], 32, max_batch=1)
    raw_m, raws_m, _ = M.planck_bands(T_lev, T_sfc, lo, hi, False)
    nrm_m, nrms_m, sc_m = M.planck_bands(T_lev, T_sfc, lo, hi, True)
    raw, raws, one = run_planck(s, T_lev, T_sfc, lo, hi, False)
    top = np.maximum(raw_m.max(axis=2), raws_m)                  # per (k, c)
    e_raw = max(np.max(np.abs(raw - raw_m) / top[:, :, None]), np.max(np.abs(raws - raws_m) / top))
    assert np.all(one == 1.0)
    # normalise = 0 takes no scale output either
    raw2, raws2, untouched = run_planck(s, T_lev, T_sfc, lo, hi, False, scale_out=False)
    assert np.array_equal(raw2, raw) and np.array_equal(raws2, raws) and np.all(np.isnan(untouched))
    nrm, nrms, sc = run_planck(s, T_lev, T_sfc, lo, hi, True)
    assert np.all(np.maximum(nrm.max(axis=2), nrms) == 1.0), "the normalised maximum is exactly 1.0"
    assert np.array_equal(sc, np.maximum(raw.max(axis=2), raws))
    e_nrm = max(np.max(np.abs(nrm - nrm_m)), np.max(np.abs(nrms - nrms_m)), np.max(np.abs(sc / sc_m - 1)))
    e_back = max(np.max(np.abs(nrm * sc[:, :, None] / raw - 1)), np.max(np.abs(nrms * sc / raws - 1)))
    print("%s: Planck stage vs model %.3e of the maximum (normalised %.3e); scale x normalised vs raw %.3e" % (label, e_raw, e_nrm, e_back))
    assert e_raw <= 1e-13 and e_nrm <= 1e-13 and e_back <= 4e-16
    s.close()
    return e_raw


@pytest.mark.parametrize("C,K,L", PLANCK_SHAPES, ids=lambda v: str(v))
def test_planck_stage_shapes(C, K, L):
    T_lev = np.stack([M.temperature_profile(L) - 3.0 * (c % 11) for c in range(C)])
    T_sfc = 288.0 + 1.5 * (np.arange(C) % 7)
    bands = [BANDS[k % len(BANDS)] for k in range(K)]
    check_planck(T_lev, T_sfc, np.array([b[0] for b in bands]), np.array([b[1] for b in bands]), "C=%d K=%d L=%d" % (C, K, L))


def test_planck_stage_every_band_at_every_temperature():
    L = 24
    T_lev = np.stack([t - 0.5 * np.arange(L) for t in M.LW_TEMPERATURES])      # 180, 216.5, 288, 320 K and 11.5 K below
    T_sfc = np.array(M.LW_TEMPERATURES)
    lo, hi = np.array([b[0] for b in BANDS]), np.array([b[1] for b in BANDS])
    x = M.C2 * np.array([[10.0, 100.0], [100.0, 350.0], [2600.0, 3250.0]]) / np.array([[320.0], [288.0], [180.0]])
    assert x[0, 1] < 1 and x[1, 0] < 1 <= x[1, 1] and x[2, 0] > 20             # below, across, far above the split
    check_planck(T_lev, T_sfc, lo, hi, "nine bands x four temperatures")
    # pi B(0, 1e6) = sigma T^4 on the device
    s = Solver(L, 32, max_batch=1)
    _, bs, _ = run_planck(s, T_lev, T_sfc, [0.0], [1e6], False)
    assert np.max(np.abs(np.pi * bs[0] / (M.SIGMA * T_sfc ** 4) - 1)) <= 1e-13
    s.close()


def test_a_temperature_that_is_not_positive_gives_nan_there():
    L = 24
    T_lev = M.temperature_profile(L)[None, :].copy()
    T_lev[0, 5], T_lev[0, 9] = 0.0, -40.0
    s = Solver(L, 32, max_batch=1)
    raw, raws, _ = run_planck(s, T_lev, np.array([288.0]), [350.0], [500.0], False)
    ok = np.ones(L, dtype=bool)
    ok[[5, 9]] = False
    assert np.all(np.isnan(raw[0, 0, ~ok])) and np.all(np.isfinite(raw[0, 0, ok])) and np.isfinite(raws[0, 0])
    s.close()


def test_a_point_whose_radiances_all_underflow_has_scale_zero_and_the_driver_says_so():
    # 9000-10000 cm^-1 at 10 K: x = c2 nu / T > 1290, e^-x = 0 in double precision, every radiance 0.  The stage documents scale 0 and
    # NaN outputs (0 / 0) for such a (band, column) and leaves the other band as it is; band_thermal raises before any solve.
    from sosrt import bands
    L = M.L_
    cold = np.full((1, L), 10.0)
    assert M.C2 * 9000.0 / 10.0 > 745.2
    s = Solver(L, 32, max_batch=1)
    raw, raws, _ = run_planck(s, cold, np.array([10.0]), [9000.0, 0.0], [10000.0, 100.0], False)
    assert np.all(raw[0] == 0.0) and raws[0, 0] == 0.0 and np.all(raw[1] > 0)
    nrm, nrms, sc = run_planck(s, cold, np.array([10.0]), [9000.0, 0.0], [10000.0, 100.0], True)
    assert sc[0, 0] == 0.0 and np.all(np.isnan(nrm[0])) and np.isnan(nrms[0, 0])
    assert sc[1, 0] > 0 and max(nrm[1].max(), nrms[1, 0]) == 1.0
    s.close()
    with pytest.raises(ValueError, match=r"band 1 = \[9000, 10000\] cm\^-1 has no Planck radiance.*column 0"):
        bands.band_thermal(([0.0, 9000.0], [100.0, 10000.0]), cold[0], 10.0, 0.1, M.RHO, tauStar_atm=1.0, alb_atm=0.0, alb_aer=0.6, **GEOM)


# ---- b. the reduce stage against NumPy in extended precision------------------------------------------------------------------------
REDUCE_SHAPES = [(3, 5, 24), (1, 1, 1), (2, 7, 1), (3, 4, 1000), (70, 3, 24)]


def reduce_inputs(C, K, Mm, seed=0):
    rng = np.random.default_rng(100 * C + 10 * K + Mm + seed)
    x = rng.standard_normal((K, C, Mm)) * 10.0 ** rng.integers(-3, 4, (K, C, Mm))
    return x, rng.uniform(0.1, 2.0, (K, C)), rng.uniform(1.0, 30.0, (K, C))


def run_reduce(s, x, w=None, sc=None, d_out=None, accumulate=False):
    K, C, Mm = x.shape
    d_x = dev(x)
    d_w, d_s = None if w is None else dev(w), None if sc is None else dev(sc)
    if d_out is None:
        d_out = dfull((C * Mm + GUARD,))
    sync()
    s.band_reduce_device(d_x.data_ptr(), d_out.data_ptr(), C, K, Mm, 0 if d_w is None else d_w.data_ptr(),
                         0 if d_s is None else d_s.data_ptr(), accumulate=accumulate)
    out = host(d_out, s)
    assert np.all(np.isnan(out[C * Mm:])), "the stage wrote past [C][M]"
    return out[:C * Mm].reshape(C, Mm), d_out


@pytest.mark.parametrize("C,K,Mm", REDUCE_SHAPES, ids=lambda v: str(v))
def test_reduce_stage_against_extended_precision(C, K, Mm):
    x, w, sc = reduce_inputs(C, K, Mm)
    s = Solver(24, 32, max_batch=1)
    one = np.ones((K, C))
    for ww, ss in ((w, sc), (None, sc), (w, None), (None, None)):
        got, _ = run_reduce(s, x, ww, ss)
        ws = ((one if ww is None else ww) * (one if ss is None else ss))
        ref = np.sum(ws.astype(np.longdouble)[:, :, None] * x.astype(np.longdouble), axis=0)
        mag = np.sum(np.abs(ws[:, :, None] * x), axis=0)
        e = float(np.max(np.abs(got - ref).astype(np.float64) / mag))
        print("C=%d K=%d M=%d weight %s scale %s: reduce vs extended precision %.3e of sum |w s x|"
              % (C, K, Mm, ww is not None, ss is not None, e))
        assert e <= 1e-15
    if C * K * Mm <= 400:                                        # the bits of the model: ascending k, one fused multiply-add each
        got, _ = run_reduce(s, x, w, sc)
        assert np.array_equal(got, M.band_reduce(x, w, sc))
    s.close()


def test_reduce_split_over_accumulating_calls_gives_the_same_bits():
    C, K, Mm = 3, 5, 24
    x, w, sc = reduce_inputs(C, K, Mm, seed=1)
    s = Solver(24, 32, max_batch=1)
    one, _ = run_reduce(s, x, w, sc)
    _, d = run_reduce(s, x[:2], w[:2], sc[:2])
    two, _ = run_reduce(s, x[2:], w[2:], sc[2:], d_out=d, accumulate=True)
    assert np.array_equal(one, two)
    d = None
    for k in range(K):
        five, d = run_reduce(s, x[k:k + 1], w[k:k + 1], sc[k:k + 1], d_out=d, accumulate=k > 0)
    assert np.array_equal(one, five)
    # accumulate = 0 does not read the output: a NaN there is overwritten
    assert np.all(np.isfinite(one))
    s.close()


# ---- c. refusals: SOSRT_E_INVALID, a message, outputs untouched ------------------------------------------------------------------------
def _refused(call, outputs, s, word=None):
    with pytest.raises(ValueError) as ei:
        call()
    assert str(ei.value), "a refusal carries a message"
    if word:
        assert word in str(ei.value), str(ei.value)
    for o in outputs:
        assert np.all(np.isnan(host(o, s))), "a refused call wrote to an output"


def test_refusals_leave_the_outputs_untouched():
    from sosrt import _lib
    import ctypes
    L, C, K = 24, 2, 3
    s = Solver(L, 32, max_batch=1)
    d_T, d_Ts = dev(np.tile(M.temperature_profile(L), (C, 1))), dev(np.full(C, 288.0))
    o_b, o_bs, o_sc = dfull((K, C, L)), dfull((K, C)), dfull((K, C))
    outs = [o_b, o_bs, o_sc]
    lo, hi = np.array([350.0, 630.0, 820.0]), np.array([500.0, 700.0, 980.0])
    sync()
    pl = lambda **k: s.planck_bands_device(k.get("T", d_T.data_ptr()), k.get("Ts", d_Ts.data_ptr()), k.get("lo", lo), k.get("hi", hi),
                                           k.get("b", o_b.data_ptr()), k.get("bs", o_bs.data_ptr()), k.get("sc", o_sc.data_ptr()),
                                           C=k.get("C", C), normalise=k.get("normalise", True))
    for bad in (0, -1):
        _refused(lambda: pl(C=bad), outs, s, "C=")
    _refused(lambda: pl(lo=[], hi=[]), outs, s, "K=0")
    for k in ("T", "Ts", "b", "bs"):
        _refused(lambda: pl(**{k: 0}), outs, s, "null")
        _refused(lambda: pl(**{k: 0}, normalise=False), outs, s, "null")
    _refused(lambda: pl(sc=0), outs, s, "d_scale_out")
    for bad in (float("nan"), float("inf"), -1.0):
        _refused(lambda: pl(lo=[350.0, bad, 820.0]), outs, s, "finite")
    _refused(lambda: pl(hi=[500.0, float("inf"), 980.0]), outs, s, "finite")
    _refused(lambda: pl(hi=[500.0, 630.0, 980.0]), outs, s, "nu_hi must be > nu_lo")
    _refused(lambda: pl(hi=[500.0, 600.0, 980.0]), outs, s, "nu_hi must be > nu_lo")
    # null edge arrays and a normalise that is neither 0 nor 1, which the binding cannot send: the symbol itself
    vp, p = ctypes.c_void_p, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    raw = lambda lo_, hi_, nrm: _lib.check(_lib.lib().sosrt_planck_bands_dev(s._h, C, K, vp(d_T.data_ptr()), vp(d_Ts.data_ptr()), lo_, hi_, nrm,
                                                                             vp(o_b.data_ptr()), vp(o_bs.data_ptr()), vp(o_sc.data_ptr())))
    _refused(lambda: raw(None, p(hi), 1), outs, s, "null")
    _refused(lambda: raw(p(lo), None, 1), outs, s, "null")
    _refused(lambda: raw(p(lo), p(hi), 2), outs, s, "normalise")
    # the reduce stage
    Mm = 7
    d_x, o_r = dev(np.ones((K, C, Mm))), dfull((C, Mm))
    sync()
    rd = lambda **k: s.band_reduce_device(k.get("x", d_x.data_ptr()), k.get("out", o_r.data_ptr()), k.get("C", C), k.get("K", K), k.get("M", Mm))
    for name in ("C", "K", "M"):
        for bad in (0, -1):
            _refused(lambda: rd(**{name: bad}), outs + [o_r], s, name + "=")
    _refused(lambda: rd(x=0), outs + [o_r], s, "null")
    _refused(lambda: rd(out=0), outs + [o_r], s, "null")
    # both stages still work on this handle, and then write
    pl()
    rd()
    assert all(np.all(np.isfinite(host(o, s))) for o in outs + [o_r])
    assert np.all(host(o_r, s) == K)
    s.close()


# ---- d. the stages leave the handle as it was ------------------------------------------------------------------------------------------
def test_the_stages_leave_the_handle_untouched():
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
    e0 = s.epilogue(z_profile=z)                                 # what the resident field and optical depths give
    run_planck(s, np.tile(M.temperature_profile(L), (3, 1)), np.full(3, 288.0), [350.0, 630.0], [500.0, 700.0], True)
    run_reduce(s, *reduce_inputs(3, 5, 24))
    e1 = s.epilogue(z_profile=z)                                 # the resident field and tau: same bytes
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    r1 = s.solve(tau, P0a, P0r)                                  # the columns and the phase state: the same solve, bit for bit
    assert np.array_equal(r0.I, r1.I) and np.array_equal(r0.n, r1.n)
    assert np.array_equal(s.first_order(tau, P0a, P0r), f0)
    s.close()


# ---- e. the thermal band solve ----------------------------------------------------------------------------------------------------------
GEOM = dict(z0=M.Z0, nb_layers=M.L_, nb_angles=M.N_, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=T.G_AER)
EPI = ("flux_down", "flux_up", "heating_rate", "net_toa")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def thermal_args():
    pts = M.THERMAL_POINTS
    pp = lambda i: np.array([p[i] for p in pts])
    t_aer = np.stack([pp(4), np.zeros(len(pts))], axis=1)         # column 0 with the layer, column 1 without
    return ((pp(0), pp(1)), M.temperature_profile(M.L_), M.T_SURFACE, t_aer, M.RHO), dict(tauStar_atm=pp(2), alb_atm=pp(3), alb_aer=pp(5), **GEOM)


@functools.lru_cache(maxsize=None)
def thermal_per_point():
    """The per-point path: one thermal batch of the two columns per band, fed the model's normalised source; its NumPy epilogue.
    (n [K, 2], scale [K], dict name -> [K, 2, L] or [K, 2])"""
    from sosrt import main
    z = T.altitudes(M.L_)
    n, scale, epi = [], [], {k: [] for k in EPI}
    for lo, hi, t_atm, w_atm, t_aer, w_aer, _, _ in M.THERMAL_POINTS:
        b, bs, sc = M.planck_bands(M.temperature_profile(M.L_), M.T_SURFACE, [lo], [hi], True)
        r = main.SOS_Aer_batch(0.5, [t_aer, 0.0], M.RHO, tauStar_atm=t_atm, alb_atm=w_atm, alb_aer=w_aer, source="thermal",
                               planck=b[0, 0], planck_surface=float(bs[0, 0]), **GEOM)
        assert np.all(r.status == 0)
        n.append(r.n)
        scale.append(float(sc[0, 0]))
        e = [T.epilogue_emission(r.I[c], r.mu, M.N_, z_profile=z, slabs=[(r.idx_up, r.idx_down)]) for c in range(2)]
        for k in EPI:
            epi[k].append(np.stack([e[c][k] for c in range(2)]))
    out = (np.stack(n), np.array(scale), {k: np.stack(v) for k, v in epi.items()})
    for a in (out[0], out[1]) + tuple(out[2].values()):
        a.setflags(write=False)
    return out


def weighted(epi, ws):
    """sum_k ws[k, c] epi[k, c, ...]"""
    return {k: np.sum(ws.reshape(ws.shape + (1,) * (v.ndim - 2)) * v, axis=0) for k, v in epi.items()}


def test_band_thermal_against_the_per_point_path():
    from sosrt import bands
    pos, kw = thermal_args()
    n_ref, scale_ref, epi_ref = thermal_per_point()
    r = bands.band_thermal(*pos, **kw, per_point=True)
    table = np.array([p[6:8] for p in M.THERMAL_POINTS])
    print("orders with / without the layer: %s (table %s)" % (r.n.tolist(), table.tolist()))
    assert np.array_equal(r.n, table) and np.array_equal(r.n, n_ref) and np.all(r.status == 0)
    assert r.scale.shape == (5, 2) and np.max(np.abs(r.scale / scale_ref[:, None] - 1)) <= 1e-13
    ref = weighted(epi_ref, np.tile(scale_ref[:, None], (1, 2)))
    for k in EPI:
        got = getattr(r, k)
        assert got.shape == ((2,) if k == "net_toa" else (2, M.L_))
        e = _rel(got, ref[k])
        print("band_thermal %s vs the per-point path: %.3e of its maximum" % (k, e))
        assert e <= RTOL, k
    olr = r.flux_up[:, 0]
    print("band-summed outgoing flux: %.4f with the layer, %.4f without; forcing %.4f" % (olr[0], olr[1], olr[1] - olr[0]))
    assert abs(olr[0] / M.OLR_WITH - 1) <= 1e-4 and abs(olr[1] / M.OLR_WITHOUT - 1) <= 1e-4
    # every point's own net flux
    point_ref = epi_ref["net_toa"] * scale_ref[:, None]
    assert r.point_net_toa.shape == (5, 2) and _rel(r.point_net_toa, point_ref) <= RTOL
    # the forcing driver: without minus with, one batch of both
    f = bands.band_thermal_forcing(pos[0], pos[1], pos[2], pos[3][:, 0], pos[4], **kw)
    print("band_thermal_forcing %.4f" % f[0])
    assert f.shape == (1,) and abs(f[0] - 1.7092) <= 2e-4 and abs(f[0] - (olr[1] - olr[0])) <= 2 * RTOL * olr[1]


def test_band_thermal_points_per_solve_gives_the_same_bits():
    from sosrt import bands
    pos, kw = thermal_args()
    w = np.array([[0.5, 1.0], [1.0, 1.0], [2.0, 0.25], [1.0, 3.0], [0.3, 1.0]])
    runs = [bands.band_thermal(*pos, **kw, weights=w, points_per_solve=P, per_point=True) for P in (1, 2, 5)]
    for r in runs[1:]:
        for k in EPI + ("n", "status", "scale", "point_net_toa"):
            assert np.array_equal(getattr(r, k), getattr(runs[0], k)), k
    assert np.array_equal(bands.band_thermal(*pos, **kw, weights=w).flux_up, runs[0].flux_up)      # the default rule: one solve
    # [K, C] weights against the NumPy sum; a subset of `want` leaves the others out
    n_ref, scale_ref, epi_ref = thermal_per_point()
    ref = weighted(epi_ref, w * scale_ref[:, None])
    for k in EPI:
        assert _rel(getattr(runs[0], k), ref[k]) <= RTOL, k
    only = bands.band_thermal(*pos, **kw, weights=w, want=("net_toa",))
    assert only.flux_up is None and only.heating_rate is None and np.array_equal(only.net_toa, runs[0].net_toa)
    # per-column temperatures [C, L], surface temperatures and emissivities [C]
    Tp = M.temperature_profile(M.L_)
    a = bands.band_thermal(pos[0], np.stack([Tp, Tp]), [M.T_SURFACE] * 2, pos[3], [M.RHO] * 2, surface_emissivity=[1 - M.RHO] * 2,
                           weights=w, **kw)
    assert np.array_equal(a.flux_up, runs[0].flux_up)


# ---- f. the solar band solve ----------------------------------------------------------------------------------------------------------------
def solar_args(t_aer=None):
    pts = M.SOLAR_POINTS
    pp = lambda i: np.array([p[i] for p in pts])
    return ((np.array(M.SOLAR_WEIGHTS), np.array(M.SOLAR_MU0), pp(2) if t_aer is None else t_aer, M.RHO),
            dict(tauStar_atm=pp(0), alb_atm=pp(1), alb_aer=pp(3), **GEOM))


@functools.lru_cache(maxsize=None)
def solar_per_point(beam_norm, aerosol="hg", with_layer=True):
    """One plain batch of the two suns per point, the handle's epilogue: (n [K, 2], dict name -> [K, 2, L] or [K, 2])."""
    from sosrt import main
    z = T.altitudes(M.L_)
    n, epi = [], {k: [] for k in EPI}
    for t_atm, w_atm, t_aer, w_aer in M.SOLAR_POINTS:
        kw = dict(GEOM, aer_phase_fun=aerosol)
        r = main.SOS_Aer_batch(np.array(M.SOLAR_MU0), t_aer if with_layer else 0.0, M.RHO, tauStar_atm=t_atm, alb_atm=w_atm,
                               alb_aer=w_aer, **kw)
        assert np.all(r.status == 0)
        e = main.get_solver(M.L_, M.N_, 2, 256).epilogue(z_profile=z, beam_norm=beam_norm, want=EPI)
        n.append(r.n)
        for k in EPI:
            epi[k].append(e[k])
    out = (np.stack(n), {k: np.stack(v) for k, v in epi.items()})
    for a in (out[0],) + tuple(out[1].values()):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("beam_norm", ["crit", "graphe"])
def test_band_solar_against_the_per_point_path(beam_norm):
    from sosrt import bands
    pos, kw = solar_args()
    n_ref, epi_ref = solar_per_point(beam_norm)
    w = np.tile(np.array(M.SOLAR_WEIGHTS)[:, None], (1, 2))
    ref = weighted(epi_ref, w)
    runs = [bands.band_solar(*pos, **kw, beam_norm=beam_norm, points_per_solve=P, per_point=True) for P in (None, 1, 3)]
    r = runs[0]
    print("solar orders %s" % r.n.tolist())
    assert np.array_equal(r.n, n_ref) and np.array_equal(r.n, np.array(M.SOLAR_ORDERS[True])) and r.scale is None
    for k in EPI:
        e = _rel(getattr(r, k), ref[k])
        print("band_solar(%s) %s vs the per-point path: %.3e of its maximum" % (beam_norm, k, e))
        assert e <= RTOL, k
    assert _rel(r.point_net_toa, epi_ref["net_toa"]) <= RTOL
    for other in runs[1:]:
        for k in EPI + ("n", "point_net_toa"):
            assert np.array_equal(getattr(other, k), getattr(r, k)), k
    # the same points without the layer: the oracle's orders
    bare = bands.band_solar(pos[0], pos[1], 0.0, pos[3], **kw, beam_norm=beam_norm, want=("net_toa",))
    assert np.array_equal(bare.n, np.array(M.SOLAR_ORDERS[False]))
    # [K, C] weights
    w2 = w * np.array([1.0, 0.5])
    r2 = bands.band_solar(w2, *pos[1:], **kw, beam_norm=beam_norm)
    assert _rel(r2.net_toa, weighted(epi_ref, w2)["net_toa"]) <= RTOL


def test_band_solar_with_an_aerosol_per_point():
    from sosrt import bands, forcing
    pos, kw = solar_args()
    kw = dict(kw, aer_phase_fun=["hg", "iso"])
    which = np.array([0, 1, 1, 0])
    r = bands.band_solar(*pos, **kw, point_aerosol=which, per_point=True, points_per_solve=3)
    n_hg, epi_hg = solar_per_point("crit", "hg")
    n_iso, epi_iso = solar_per_point("crit", "iso")
    assert not np.array_equal(epi_hg["net_toa"], epi_iso["net_toa"])
    for k, a in enumerate(which):
        n_ref, net_ref = (n_hg, epi_hg["net_toa"]) if a == 0 else (n_iso, epi_iso["net_toa"])
        assert np.array_equal(r.n[k], n_ref[k])
        assert _rel(r.point_net_toa[k], net_ref[k]) <= RTOL
    mixed = {k: np.where((which == 0).reshape((-1,) + (1,) * (epi_hg[k].ndim - 1)), epi_hg[k], epi_iso[k]) for k in EPI}
    ref = weighted(mixed, np.tile(np.array(M.SOLAR_WEIGHTS)[:, None], (1, 2)))
    for k in EPI:
        assert _rel(getattr(r, k), ref[k]) <= RTOL, k
    # the forcing: with minus without the layer, the sign of forcing.radiative_forcing; both halves in one batch
    f = bands.band_solar_forcing(*pos, **kw, point_aerosol=which)
    _, epi0 = solar_per_point("crit", "hg", False)               # (no aerosol: its phase function does not matter)
    ref_f = ref["net_toa"] - weighted(epi0, np.tile(np.array(M.SOLAR_WEIGHTS)[:, None], (1, 2)))["net_toa"]
    print("band_solar_forcing %s, per-point %s" % (f, ref_f))
    assert f.shape == (2,) and np.max(np.abs(f - ref_f)) <= 2 * RTOL * np.max(np.abs(ref["net_toa"]))
    # one point, one sun: radiative_forcing itself
    t_atm, w_atm, t_aer, w_aer = M.SOLAR_POINTS[1]
    one = bands.band_solar_forcing([1.0], 0.5, t_aer, M.RHO, tauStar_atm=t_atm, alb_atm=w_atm, alb_aer=w_aer, **GEOM)
    rf = forcing.radiative_forcing(0.5, t_atm, [t_aer], M.RHO, w_atm, [w_aer], z0=M.Z0, nb_layers=M.L_, nb_angles=M.N_, g_aer=T.G_AER)
    assert np.sign(one[0]) == np.sign(rf[0]) and abs(one[0] - rf[0]) <= 2 * RTOL * abs(epi_hg["net_toa"][1, 0])


# ---- g. the existing paths on the cached handle -----------------------------------------------------------------------------------------
def test_existing_paths_keep_their_bits_after_a_band_call(monkeypatch):
    from sosrt import bands, main
    t_aer, rho = np.array([0.3, 0.12, 0.0]), np.array([0.1, 0.3, 0.0])
    drv = dict(GEOM, tauStar_atm=1.0, alb_atm=0.1, alb_aer=0.6)
    pl = T.planck_profile(M.L_)
    plain = main.SOS_Aer_batch(0.5, t_aer, rho, **drv)
    th = main.SOS_Aer_batch(0.5, t_aer, rho, source="thermal", planck=pl, planck_surface=1.0, **drv)

    def same():
        a = main.SOS_Aer_batch(0.5, t_aer, rho, **drv)
        b = main.SOS_Aer_batch(0.5, t_aer, rho, source="thermal", planck=pl, planck_surface=1.0, **drv)
        return (np.array_equal(a.I, plain.I) and np.array_equal(a.n, plain.n) and np.array_equal(b.I, th.I) and np.array_equal(b.n, th.n))

    pos, kw = thermal_args()
    bands.band_thermal(*pos, **kw, points_per_solve=2)
    assert same()
    spos, skw = solar_args()
    bands.band_solar(*spos, **dict(skw, aer_phase_fun=["hg", "iso"]), point_aerosol=[0, 1, 1, 0])
    assert same()

    def boom(self, *a, **k):
        raise RuntimeError("raised in between")
    for name in ("band_reduce_device", "epilogue_emission_device", "epilogue_device"):
        with monkeypatch.context() as mp:
            mp.setattr(Solver, name, boom)
            if name != "epilogue_device":
                with pytest.raises(RuntimeError, match="in between"):
                    bands.band_thermal(*pos, **kw)
            if name != "epilogue_emission_device":
                with pytest.raises(RuntimeError, match="in between"):
                    bands.band_solar(*spos, **dict(skw, aer_phase_fun=["hg", "iso"]), point_aerosol=[0, 1, 1, 0])
        assert same()
