"""Per-level weights on the source function on the device (csrc/profile.hip, csrc/api_profile.hip, sosrt_set_row_weights_dev;
DESIGN section 29) through the C ABI: the weighted source function, the two stage kernels and whole solves against the NumPy
model of tests/profile_np.py (which tests/test_profile_host.py pins to the oracle), the constant-weight identity, the handle's
state with every guarded entry, and the drivers against the chain of calls they stand for."""
import functools

import numpy as np
import pytest

import driver_cases as DC
import profile_np as P
import sos_oracle as O
import spherical_np as S
import thermal_np as T
from sosrt import _lib
from sosrt.solver import Solver
from util import rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-10                                                   # the project's parity bar
KERNEL_BAR = 1e-12                                             # a stage kernel against its model, of the field maximum
UNIT_BAR = 1e-14                                               # ... and with unit weights against the kernel it generalises


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


def _err(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- the columns of the tests: per shape, shared by the tests and never changed -------------------------------------------------
# (L, N, B, slabs): (41, 33) is odd in both (the general transport kernel), (24, 128) two waves per column, the two-slab table has
# five zones, (200, 128) is the shipped shape
SHAPES = {"L40-N32-B5": (40, 32, 5, None), "L41-N33-B3": (41, 33, 3, None), "L24-N128-B2": (24, 128, 2, None),
          "L48-N32-B3-2slabs": (48, 32, 3, S.TWO_SLABS), "L200-N128-B3": (200, 128, 3, None)}
SMALL = [k for k in SHAPES if not k.startswith("L200")]
# (mu0, rho, alb_atm, alb_aer) of column b
PAR = [(0.6, 0.3, 1.0, 0.97), (0.45, 0.0, 0.9, 0.8), (0.83, 0.5, 1.0, 1.0), (0.3, 0.1, 0.95, 0.9), (0.7, 0.2, 0.8, 0.97)]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def shape_columns(name, surface="specular"):
    L, N, B, slabs = SHAPES[name]
    return tuple(P.column(O, N, L, PAR[b][0], PAR[b][1], slabs, surface, alb_atm=PAR[b][2], alb_aer=PAR[b][3]) for b in range(B))


@functools.lru_cache(maxsize=None)
def shape_weights(name):
    """(w_atm [B, L], w_aer [B, L]) drawn independently in [0.2, 1], with a jump at the slab's first and last row and rows of exact
    1.0 and 0.0 (profile_np.random_weights); the last column keeps unit weights on the atmosphere."""
    cols = shape_columns(name)
    w = [P.random_weights(c, 100 + b) for b, c in enumerate(cols)]
    wa, wr = np.stack([x[0] for x in w]), np.stack([x[1] for x in w])
    wa[-1] = 1.0
    return _frozen(wa, wr)


def handle(cols, phase=True, max_orders=64, B_max=None):
    c0 = cols[0]
    L, N, B = len(c0.tau), c0.N, len(cols)
    s = Solver(L, N, max_batch=B_max or B, max_orders=max_orders)
    s.set_grid(c0.mu)
    if phase:
        s.set_phase(c0.P_atm, c0.P_aer)
    set_cols(s, cols)
    return s, np.stack([c.tau for c in cols])


def set_cols(s, cols):
    c0 = cols[0]
    col = lambda f: [f(c) for c in cols]
    if c0.zone_table is None:
        s.set_columns(col(lambda c: c.idx_up), col(lambda c: c.idx_down), col(lambda c: c.mu0), col(lambda c: c.grd_alb),
                      col(lambda c: c.alb_atm), col(lambda c: c.alb_aer), col(lambda c: c.dtau_atm), col(lambda c: c.dtau_aer),
                      col(lambda c: c.tauStar_tot), surface=c0.surface)
    else:
        s.set_columns_zones(np.array([[z.r0 for z in c.zone_table] for c in cols]), [int(z.kind == "mix") for z in c0.zone_table],
                            col(lambda c: c.mu0), col(lambda c: c.grd_alb), col(lambda c: c.alb_atm), col(lambda c: c.dtau_atm),
                            np.array([[z.alb_aer for z in c.zone_table] for c in cols]),
                            np.array([[z.dtau_aer for z in c.zone_table] for c in cols]), col(lambda c: c.tauStar_tot),
                            surface=c0.surface)


def set_weights(s, wa, wr, B=None):
    """Uploads and sets the weights (None: the NULL pointer); returns the tensors, which the copy has already read in stream order."""
    d_wa, d_wr = None if wa is None else dev(wa), None if wr is None else dev(wr)
    sync()
    s.set_row_weights_device(0 if d_wa is None else d_wa.data_ptr(), 0 if d_wr is None else d_wr.data_ptr(), B=B)
    s.synchronize()
    return d_wa, d_wr


def sigma_of(cols, path):
    if path == "plane":
        return np.stack([S.plane_path(c.tau, c.mu0) for c in cols])
    return np.stack([S.slant_path(c.tau, S.altitudes(len(c.tau)), c.mu0) for c in cols])


def p0(cols):
    return np.stack([c.P0_atm for c in cols]), np.stack([c.P0_aer for c in cols])


def run_first_order(s, tau, sigma, P0a, P0r, profile=True, B=None):
    d = [dev(x) for x in (tau, sigma, P0a, P0r)]
    d_I1 = dfull(tau.shape + (s.D,))
    sync()
    f = s.first_order_profile_device if profile else s.first_order_beam_device
    f(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_I1.data_ptr(), B=B)
    return host(d_I1, s)


def run_emission(s, tau, planck, bs, es=None, profile=True):
    d = [dev(x) for x in (tau, planck, bs)]
    d_es = None if es is None else dev(es)
    d_I0 = dfull(tau.shape + (s.D,))
    sync()
    f = s.emission_profile_device if profile else s.emission_device
    f(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_I0.data_ptr(), 0 if d_es is None else d_es.data_ptr())
    return host(d_I0, s)


def solve_dev(s, tau, P0a, P0r, I1=None):
    torch = _torch()
    B, L = tau.shape
    d_tau, d_P0a, d_P0r = dev(tau), dev(P0a), dev(P0r)
    d_I1 = None if I1 is None else dev(I1)
    d_I = dfull((B, L, s.D))
    d_n = torch.zeros(B, dtype=torch.int32, device=d_tau.device)
    d_st = torch.zeros(B, dtype=torch.int32, device=d_tau.device)
    sync()
    s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_I1=0 if d_I1 is None else d_I1.data_ptr(),
                   d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
    s.synchronize()
    return d_I.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()


# ---- 1. sosrt_source with weights against the model's Jn ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_first_order(name, path="plane"):
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    sig = sigma_of(cols, path)
    return _frozen(np.stack([P.first_order_profile(c, sig[b], wa[b], wr[b]) for b, c in enumerate(cols)]))


@pytest.mark.parametrize("mix_groups", [None, "0"], ids=["mix-default", "mix-0"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_source_with_weights(name, mix_groups, monkeypatch):
    if mix_groups is None:
        monkeypatch.delenv("SOSRT_MIX_GROUPS", raising=False)
    else:
        monkeypatch.setenv("SOSRT_MIX_GROUPS", mix_groups)
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    x = model_first_order(name)
    s, _ = handle(cols)
    before = s.phase_sets_info()["groups"]
    assert (before > 0) == (mix_groups is None)
    plain = s.source(x)
    keep = set_weights(s, wa, wr)
    assert s.phase_sets_info()["groups"] == 0                  # slab rows take the two passes while weights are set
    got = s.source(x)
    worst = 0.0
    for b, c in enumerate(cols):
        ref = P.source_function(O, c, x[b], wa[b], wr[b])
        worst = max(worst, rel_err(got[b], ref))
    print("%s SOSRT_MIX_GROUPS=%s: weighted source function vs the model %.3e" % (name, mix_groups, worst))
    assert worst <= RTOL
    # rows of weight exactly 0 on both constituents are exactly 0; clearing restores the grouping and the bits
    zero = (wa == 0) & ((wr == 0) | np.stack([P.zone_of_rows(c) % 2 == 0 for c in cols]))
    assert zero.any() and np.all(got[zero] == 0)
    set_weights(s, None, None)
    assert s.phase_sets_info()["groups"] == before
    assert np.array_equal(s.source(x), plain)
    del keep
    s.close()


# ---- 2. the two new kernels against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plane", "slant"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_first_order_profile_kernel(name, path):
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    sig = sigma_of(cols, path)
    P0a, P0r = p0(cols)
    s, tau = handle(cols, phase=False)
    set_weights(s, wa, wr)
    got = run_first_order(s, tau, sig, P0a, P0r)
    assert np.all(np.isfinite(got))
    ref = model_first_order(name, path)
    worst = max(_err(got[b], ref[b]) for b in range(len(cols)))
    print("%s %s: first-order profile kernel vs the model %.3e of the field maximum" % (name, path, worst))
    assert worst <= KERNEL_BAR
    if len(cols) > 2:                                          # the first columns alone
        assert np.array_equal(run_first_order(s, tau[:2], sig[:2], P0a[:2], P0r[:2], B=2), got[:2])
    # unit weights: the beam kernel
    set_weights(s, np.ones_like(wa), None)
    unit = run_first_order(s, tau, sig, P0a, P0r)
    set_weights(s, None, None)
    beam = run_first_order(s, tau, sig, P0a, P0r, profile=False)
    e = max(_err(unit[b], beam[b]) for b in range(len(cols)))
    print("%s %s: unit weights vs sosrt_first_order_beam_dev %.3e (bit-equal: %s)" % (name, path, e, np.array_equal(unit, beam)))
    assert e <= UNIT_BAR
    s.close()


def test_first_order_profile_kernel_with_a_p0_per_zone():
    """[B][nzmax][2N] P0 of the aerosol, as the beam kernel takes it after sosrt_set_aerosol_sets with a zone table."""
    name = "L48-N32-B3-2slabs"
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    sig = sigma_of(cols, "plane")
    s = Solver(48, 32, max_batch=3)
    s.set_grid(cols[0].mu)
    P_b = O.phase_hg(32, cols[0].mu, 0.5, 0.3)[1]
    s.set_phase_sets(cols[0].P_atm, np.stack([cols[0].P_aer, P_b]))
    set_cols(s, cols)
    s.set_aerosol_sets(np.tile(np.array([0, 0, 0, 1, 0], dtype=np.int32), (3, 1)))
    P0z = np.zeros((3, 5, 64))
    for b, c in enumerate(cols):
        P0z[b, 1] = c.P0_aer
        P0z[b, 3] = O.phase_hg(32, c.mu, c.mu0, 0.3)[0]
    set_weights(s, wa, wr)
    got = run_first_order(s, np.stack([c.tau for c in cols]), sig, p0(cols)[0], P0z)
    ref = [P.first_order_profile(c, sig[b], wa[b], wr[b], P0_aer_zone=P0z[b]) for b, c in enumerate(cols)]
    worst = max(_err(got[b], ref[b]) for b in range(3))
    print("per-zone P0: first-order profile kernel vs the model %.3e" % worst)
    assert worst <= KERNEL_BAR
    # the sets cannot be regrouped under weights
    with pytest.raises(_lib.SosrtError, match="weights"):
        s.set_aerosol_sets(np.zeros((3, 5), dtype=np.int32))
    s.close()


def planck_of(cols):
    L, B = len(cols[0].tau), len(cols)
    b = np.arange(B)
    return T.planck_profile(L)[None, :] * (1 + 0.1 * b[:, None]), 1 + 0.05 * b, 0.95 - 0.01 * b


# (the Lambertian grounds at the small shapes: their sum over the column's waves does not depend on L)
@pytest.mark.parametrize("name,surface", [(n, sf) for n in SHAPES for sf in ("specular", "lambertian", "lambertian_readme")
                                          if sf == "specular" or n in SMALL])
def test_emission_profile_kernel(name, surface):
    cols = shape_columns(name, surface)
    wa, wr = shape_weights(name)
    pl, bs, es = planck_of(cols)
    s, tau = handle(cols, phase=False)
    set_weights(s, wa, wr)
    for explicit in (False, True):
        got = run_emission(s, tau, pl, bs, es if explicit else None)
        assert np.all(np.isfinite(got))
        ref = [P.emission_profile(c, pl[b], bs[b], wa[b], wr[b], es[b] if explicit else None) for b, c in enumerate(cols)]
        worst = max(_err(got[b], ref[b]) for b in range(len(cols)))
        print("%s %s emissivity %s: emission profile kernel vs the model %.3e of the field maximum"
              % (name, surface, "given" if explicit else "1 - rho", worst))
        assert worst <= KERNEL_BAR
    set_weights(s, None, np.ones_like(wr))
    unit = run_emission(s, tau, pl, bs)
    set_weights(s, None, None)
    plain = run_emission(s, tau, pl, bs, profile=False)
    e = max(_err(unit[b], plain[b]) for b in range(len(cols)))
    print("%s %s: unit weights vs sosrt_emission_dev %.3e (bit-equal: %s)" % (name, surface, e, np.array_equal(unit, plain)))
    assert e <= UNIT_BAR
    s.close()


# ---- 3. whole solves against the model loop fed the device's first order ---------------------------------------------------------
KNOBS = ("SOSRT_TRANSPORT", "SOSRT_SCAN_SPLIT", "SOSRT_RING_MOMENTS", "SOSRT_SCAN_MOMENTS", "SOSRT_SCAN_MOMENTS_MIN", "SOSRT_GROUPS",
         "SOSRT_SPLIT_MIN", "SOSRT_MIX_GROUPS")
# SOSRT_SPLIT_MIN=2 with SOSRT_GROUPS unset: two column groups also for these few columns
TRANSPORTS = {"ring": dict(SOSRT_TRANSPORT="ring"), "scan-split": dict(SOSRT_TRANSPORT="scan", SOSRT_SCAN_SPLIT="1"),
              "scan-one": dict(SOSRT_TRANSPORT="scan", SOSRT_SCAN_SPLIT="0"), "general": dict(SOSRT_TRANSPORT="general")}
MOMENTS = {"records": dict(SOSRT_RING_MOMENTS="1", SOSRT_SCAN_MOMENTS="1", SOSRT_SCAN_MOMENTS_MIN="1"),
           "rows": dict(SOSRT_RING_MOMENTS="0", SOSRT_SCAN_MOMENTS="0")}
GROUPS = {"groups-1": dict(SOSRT_GROUPS="1"), "groups-auto": dict(SOSRT_SPLIT_MIN="2")}
_solved = {}


def weighted_solve(name, env, monkeypatch):
    """(I, n, status, the device's first order, moment orders) of the shape's columns under `env`"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    P0a, P0r = p0(cols)
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    I1 = run_first_order(s, tau, sigma_of(cols, "plane"), P0a, P0r)
    I, n, st = solve_dev(s, tau, P0a, P0r, I1)
    ring, scan = _lib.c_int(), _lib.c_int()
    total = _lib.c_int()
    _lib.check(_lib.lib().sosrt_ring_moments_stats(s._h, ring, total))
    _lib.check(_lib.lib().sosrt_scan_moments_stats(s._h, scan, total))
    s.close()
    return I, n, st, I1, ring.value + scan.value


def model_solve(name, I1):
    """The model loop from the device's first order (the same bits under every environment), solved once per shape"""
    if name not in _solved:
        cols = shape_columns(name)
        wa, wr = shape_weights(name)
        _solved[name] = (I1.copy(), [P.solve_column(O, c, wa[b], wr[b], I1[b]) for b, c in enumerate(cols)])
    first, sols = _solved[name]
    assert np.array_equal(first, I1), "the first order changed with the environment"
    return sols


@pytest.mark.parametrize("groups", list(GROUPS))
@pytest.mark.parametrize("moments", list(MOMENTS))
@pytest.mark.parametrize("transport", list(TRANSPORTS))
@pytest.mark.parametrize("name", SMALL)
def test_whole_solves(name, transport, moments, groups, monkeypatch):
    env = dict(TRANSPORTS[transport], **MOMENTS[moments], **GROUPS[groups])
    I, n, st, I1, mom = weighted_solve(name, env, monkeypatch)
    sols = model_solve(name, I1)
    worst = max(rel_err(I[b], r.I) for b, r in enumerate(sols))
    print("%s %s %s %s: n = %s (model %s), field vs the model loop %.3e, %d orders on moment records"
          % (name, transport, moments, groups, list(n), [r.n for r in sols], worst, mom))
    assert list(st) == [0] * len(sols)
    assert list(n) == [r.n for r in sols]
    assert worst <= RTOL
    if moments == "rows":
        assert mom == 0
    if name == "L24-N128-B2" and moments == "records" and transport != "general":
        assert mom > 0, "the record modes did not engage: their agreement with the rows of Jn below would not be exercised"
    # the record modes stay enabled under weights: they must agree with the rows of Jn
    other = dict(TRANSPORTS[transport], **MOMENTS["rows" if moments == "records" else "records"], **GROUPS[groups])
    if moments == "records" and mom > 0:
        I2, n2, _, _, mom2 = weighted_solve(name, other, monkeypatch)
        e = max(_err(I[b], I2[b]) for b in range(len(sols)))
        print("%s %s %s: moment records vs rows of Jn %.3e" % (name, transport, groups, e))
        assert mom2 == 0 and list(n2) == list(n) and e <= 1e-12


def test_whole_solve_at_the_shipped_shape(monkeypatch):
    name = "L200-N128-B3"
    I, n, st, I1, mom = weighted_solve(name, {}, monkeypatch)
    sols = model_solve(name, I1)
    worst = max(rel_err(I[b], r.I) for b, r in enumerate(sols))
    print("%s default knobs: n = %s (model %s), field vs the model loop %.3e, %d orders on moment records"
          % (name, list(n), [r.n for r in sols], worst, mom))
    assert list(st) == [0, 0, 0] and list(n) == [r.n for r in sols] and worst <= RTOL


def test_order_loop_launch_stays_off_under_weights(monkeypatch):
    """With sosrt_set_order_loop(1) the shipped shape's last orders run in one order-loop launch; under weights the plan keeps it
    off (OrderInputs::row_weights), and the solve is the two-launch solve: the model's field, the bits of order-loop mode 0."""
    name = "L200-N128-B3"
    base = weighted_solve(name, {}, monkeypatch)               # order-loop mode 0 (the default)
    sols = model_solve(name, base[3])
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    P0a, P0r = p0(cols)
    s, tau = handle(cols)
    s.set_order_loop(1)
    plain = solve_dev(s, tau, P0a, P0r)
    launches_plain = s.order_loop_stats()[0]
    set_weights(s, wa, wr)
    I1 = run_first_order(s, tau, sigma_of(cols, "plane"), P0a, P0r)
    I, n, st = solve_dev(s, tau, P0a, P0r, I1)
    launches_weighted = s.order_loop_stats()[0]
    set_weights(s, None, None)
    again = solve_dev(s, tau, P0a, P0r)
    launches_again = s.order_loop_stats()[0]
    s.close()
    print("order-loop launches: %d without weights, %d with, %d after clearing" % (launches_plain, launches_weighted, launches_again))
    assert launches_plain >= 1 and launches_again >= 1, "the shape does not plan the order-loop launch: the check below would be vacuous"
    assert launches_weighted == 0
    assert np.array_equal(I, base[0]) and np.array_equal(n, base[1]) and list(st) == [0, 0, 0]
    assert list(n) == [r.n for r in sols] and max(rel_err(I[b], r.I) for b, r in enumerate(sols)) <= RTOL
    assert all(np.array_equal(a, b) for a, b in zip(again, plain))


def test_thermal_whole_solve():
    name = "L40-N32-B5"
    cols = tuple(P._with_albedos(c, 0.5 * c.alb_atm, 0.6) for c in shape_columns(name))
    wa, wr = shape_weights(name)
    pl, bs, _ = planck_of(cols)
    P0a, P0r = p0(cols)
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    I0 = run_emission(s, tau, pl, bs)
    I, n, st = solve_dev(s, tau, P0a, P0r, I0)
    s.close()
    for b, c in enumerate(cols):
        r = P.solve_column(O, c, wa[b], wr[b], I0[b])
        e = rel_err(I[b], r.I)
        print("thermal column %d: n = %d (model %d), %.3e" % (b, n[b], r.n, e))
        assert st[b] == 0 and n[b] == r.n and e <= RTOL


# ---- 4. the constant-w identity on the device ----------------------------------------------------------------------------------------
def test_constant_weight_identity_through_the_driver():
    """SOS_Aer_batch(gas_tau = tau0 (1 / w - 1)) is SOS_Aer_batch on the columns with both albedos times w and both optical depths
    over w.  mu0 = 0.6 and 0.45 are 1.3e-2 and 1.6e-3 from the nearest node of N = 32: the ordinary call's closed-form first
    order has no limit branch in play."""
    from sosrt.inputs import tau_profile
    from sosrt.main import SOS_Aer_batch
    DC.fresh()
    w, L, N = 0.8, 40, 32
    mu0, t_aer, t_atm = np.array([0.6, 0.45]), np.array([0.05, 0.1]), 0.124
    tau0 = np.stack([tau_profile(t_atm, t, 120, 25, 17, L) for t in t_aer])
    kw = dict(nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
    got = SOS_Aer_batch(mu0, t_aer, 0.3, tauStar_atm=t_atm, alb_atm=1.0, alb_aer=0.9, gas_tau=tau0 * (1 / w - 1), **kw)
    ref = SOS_Aer_batch(mu0, t_aer / w, 0.3, tauStar_atm=t_atm / w, alb_atm=w, alb_aer=0.9 * w, **kw)
    assert np.allclose(got.row_weight, w, rtol=0, atol=1e-13) and np.allclose(got.tau, ref.tau, rtol=1e-14)
    e = max(_err(got.I[b], ref.I[b]) for b in range(2))
    print("constant w = %g through SOS_Aer_batch: n = %s / %s, %.3e of the field maximum" % (w, list(got.n), list(ref.n), e))
    assert list(got.n) == list(ref.n) and list(got.status) == [0, 0]
    assert e <= RTOL
    DC.fresh()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------
def test_clearing_gives_the_bits_of_a_fresh_handle_and_set_columns_clears():
    name = "L40-N32-B5"
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    P0a, P0r = p0(cols)
    s, tau = handle(cols)
    fresh = solve_dev(s, tau, P0a, P0r)
    s.close()
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    I1 = run_first_order(s, tau, sigma_of(cols, "plane"), P0a, P0r)
    weighted = solve_dev(s, tau, P0a, P0r, I1)
    assert not np.array_equal(weighted[0], fresh[0])
    set_weights(s, None, None)
    again = solve_dev(s, tau, P0a, P0r)
    assert all(np.array_equal(a, b) for a, b in zip(again, fresh))
    # sosrt_set_columns clears: the plain solve runs, the profile stage has no weights
    set_weights(s, wa, wr)
    with pytest.raises(_lib.SosrtError, match="weights"):
        solve_dev(s, tau, P0a, P0r)
    set_cols(s, cols)
    again = solve_dev(s, tau, P0a, P0r)
    assert all(np.array_equal(a, b) for a, b in zip(again, fresh))
    with pytest.raises(_lib.SosrtError, match="no per-level weights"):
        run_first_order(s, tau, sigma_of(cols, "plane"), P0a, P0r)
    s.close()


def test_a_column_does_not_depend_on_its_batch_or_its_neighbours():
    name = "L40-N32-B5"
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    P0a, P0r = p0(cols)
    sig = sigma_of(cols, "plane")

    def run(idx, wa_, wr_):
        sub = [cols[i] for i in idx]
        s, tau = handle(sub, B_max=5)
        set_weights(s, wa_, wr_)
        I1 = run_first_order(s, tau, sig[idx], P0a[idx], P0r[idx])
        out = solve_dev(s, tau, P0a[idx], P0r[idx], I1)
        s.close()
        return out

    full = run([0, 1, 2, 3, 4], wa, wr)
    alone = run([2], wa[2:3], wr[2:3])
    assert all(np.array_equal(a[0], f[2]) for a, f in zip(alone, full))
    # other weights on the neighbours; and B = 3 of the five columns weighted, the rest left at one
    wa2, wr2 = wa.copy(), wr.copy()
    wa2[[0, 1, 3, 4]] = 0.5
    wr2[[0, 1, 3, 4]] = 0.9
    other = run([0, 1, 2, 3, 4], wa2, wr2)
    assert all(np.array_equal(o[2], f[2]) for o, f in zip(other, full))
    s, tau = handle(cols)
    set_weights(s, wa[:3], wr[:3], B=3)
    I1 = run_first_order(s, tau, sig, P0a, P0r)
    part = solve_dev(s, tau, P0a, P0r, I1)
    set_weights(s, np.concatenate((wa[:3], np.ones((2, 40)))), np.concatenate((wr[:3], np.ones((2, 40)))))
    I1b = run_first_order(s, tau, sig, P0a, P0r)
    whole = solve_dev(s, tau, P0a, P0r, I1b)
    s.close()
    assert np.array_equal(I1, I1b) and all(np.array_equal(a, b) for a, b in zip(part, whole))
    assert all(np.array_equal(a[:3], f[:3]) for a, f in zip(part, full))


def test_guarded_entries_return_state_errors_and_write_nothing():
    name = "L40-N32-B5"
    cols = shape_columns(name)
    wa, wr = shape_weights(name)
    P0a, P0r = p0(cols)
    s, tau = handle(cols)
    B, L, D = 5, 40, s.D
    d_tau, d_sig, d_P0a, d_P0r = dev(tau), dev(sigma_of(cols, "plane")), dev(P0a), dev(P0r)
    d_pl, d_bs = dev(np.ones((B, L))), dev(np.ones(B))
    d_I = dev(np.ones((B, L, D)))
    rows = dev(np.ones((2, D)))
    p0rows = dev(np.ones((B, 2)))
    mu_view, lev32 = np.array([0.5]), np.array([0, L - 1], dtype=np.int32)
    out = dfull((B + 2, L, D))                                 # sentinels around [1 : B + 1]
    o_n = _torch().full((B + 2,), -7, dtype=_torch().int32, device=out.device)
    set_weights(s, wa, wr)
    sync()
    o, on = out[1:].data_ptr(), o_n[1:].data_ptr()
    lev = [0, L - 1]
    calls = {
        "sosrt_first_order": lambda: s.first_order(tau, P0a, P0r),
        "sosrt_solve": lambda: s.solve(tau, P0a, P0r),
        "sosrt_solve_dev": lambda: s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), o, d_n_orders=on, d_status=on),
        "sosrt_first_order_beam_dev": lambda: s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), o),
        "sosrt_view_first_order_beam_dev": lambda: s.view_first_order_beam_device([0.5], d_tau.data_ptr(), d_sig.data_ptr(), p0rows.data_ptr(),
                                                                                  p0rows.data_ptr(), lev, o),
        "sosrt_view_radiance_dev": lambda: _lib.check(_lib.lib().sosrt_view_radiance_dev(
            s._h, B, 1, mu_view.ctypes.data, d_tau.data_ptr(), d_I.data_ptr(), rows.data_ptr(), rows.data_ptr(), p0rows.data_ptr(),
            p0rows.data_ptr(), 0, 2, lev32.ctypes.data, o, o)),
        "sosrt_emission_dev": lambda: s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), o),
        "sosrt_emission_view_dev": lambda: s.emission_view_device([0.5], d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), lev, o),
    }
    for what, call in calls.items():
        with pytest.raises(_lib.SosrtError) as ei:             # SOSRT_E_STATE (a ValueError would be SOSRT_E_INVALID)
            call()
        assert "weights" in str(ei.value), (what, str(ei.value))
        assert np.all(np.isnan(host(out, s))) and np.all(host(o_n, s) == -7), "%s wrote to an output" % what
    # the entries that stay open: the source step and the solve from a caller's first order
    assert np.all(np.isfinite(s.source(np.ones((B, L, D)))))
    # refusals of the new entries: ValueError (SOSRT_E_INVALID) with a message, nothing written
    d_w = dev(wa)
    for bad in (0, 6):
        with pytest.raises(ValueError, match="B="):
            s.set_row_weights_device(d_w.data_ptr(), d_w.data_ptr(), B=bad)
        with pytest.raises(ValueError, match="B="):
            s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), o, B=bad)
        with pytest.raises(ValueError, match="B="):
            s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), o, B=bad)
    with pytest.raises(ValueError, match="null"):
        s.first_order_profile_device(d_tau.data_ptr(), 0, d_P0a.data_ptr(), d_P0r.data_ptr(), o)
    with pytest.raises(ValueError, match="null"):
        s.emission_profile_device(d_tau.data_ptr(), 0, d_bs.data_ptr(), o)
    assert np.all(np.isnan(host(out, s)))
    s.close()
    # no columns; the single slab
    s = Solver(L, 32, max_batch=2)
    s.set_grid(cols[0].mu)
    with pytest.raises(_lib.SosrtError, match="sosrt_set_columns"):
        s.set_row_weights_device(d_w.data_ptr(), d_w.data_ptr(), B=1)
    s.set_columns_single_slab([0.5, 0.6], 0.9, 0.3)
    with pytest.raises(ValueError, match="single slab"):
        s.set_row_weights_device(d_w.data_ptr(), d_w.data_ptr())
    s.close()


# ---- 6. the drivers against the chain of calls they stand for -------------------------------------------------------------------------
GAS = np.concatenate(([0.0], np.cumsum(np.where((np.arange(1, DC.L) >= 4) & (np.arange(1, DC.L) <= 9), 0.01, 0.002))))
GAS3 = GAS[None, :] * np.array([1.0, 0.5, 2.0])[:, None]


def hand_chain(mu0, t_aer, rho, gas, t_atm=0.124, alb_atm=1.0, alb_aer=1.0, z=None, thermal=None, want=(), phases=(None,) * 4):
    """What a driver with gas_tau stands for, call by call on the cached handle: the columns on the total optical depth, the
    weights, the first order (or the emission) with them, the solve from it, the epilogue; the weights cleared."""
    from sosrt import main
    torch = _torch()
    ns = main._gas_args(gas, len(mu0), DC.L)
    s, tau, P0a, P0r, mu, iu, idn, N = main._prepare_batch(mu0, t_aer, rho, t_atm, alb_atm, alb_aer, 120, 25, 17, DC.L, DC.N, "rayleigh",
                                                           0.0, "hg", 0.7, None, None, *phases, "specular", 256, 0, gas=ns)
    B = tau.shape[0]
    out = {}
    with main._on_torch_stream(s, 0) as dv:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dv)
        d_tau, d_w = up(tau), up(ns.w)
        d_I1 = torch.empty((B, DC.L, s.D), dtype=torch.float64, device=dv)
        d_I = torch.empty_like(d_I1)
        d_n, d_st = torch.zeros(B, dtype=torch.int32, device=dv), torch.zeros(B, dtype=torch.int32, device=dv)
        d_e = {k: torch.empty((B,) if k == "net_toa" else (B, DC.L), dtype=torch.float64, device=dv) for k in want}
        e = lambda k: d_e[k].data_ptr() if k in d_e else 0
        epi = (e("flux_down"), e("flux_up"), 0, 0, e("net_toa"))
        try:
            s.set_row_weights_device(d_w.data_ptr(), d_w.data_ptr(), B=B)
            if thermal is not None:
                d_pl, d_bs = up(thermal[0]), up(thermal[1])
                s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I1.data_ptr(), B=B)
                p0a = p0r = 0
            else:
                d_P0a, d_P0r = up(P0a), up(P0r)
                p0a, p0r = d_P0a.data_ptr(), d_P0r.data_ptr()
                if z is None:
                    d_sig = up(tau / np.asarray(mu0, dtype=np.float64)[:, None])
                else:
                    d_z, d_sig = up(z), torch.empty((B, DC.L), dtype=torch.float64, device=dv)
                    s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), B=B)
                s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), p0a, p0r, d_I1.data_ptr(), B=B)
                out["beam_slant"] = d_sig
            s.solve_device(d_tau.data_ptr(), p0a, p0r, d_I.data_ptr(), d_I1=d_I1.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            if want:
                if thermal is not None:
                    s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), 0, *epi, B=B)
                elif z is None:
                    s.epilogue_device(d_tau.data_ptr(), d_I.data_ptr(), 0, "crit", *epi)
                else:
                    s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), 0, "crit", *epi, B=B)
            s.synchronize()
        finally:
            s.set_row_weights_device(0, 0)
        out.update(I=d_I, n=d_n, status=d_st, **d_e)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out["tau"], out["w"] = tau, ns.w
    return out


def test_batch_drivers_are_the_hand_chain():
    from sosrt.main import SOS_Aer, SOS_Aer_batch, solve_batch_device
    DC.fresh()
    kw = dict(DC.SHAPE, **DC.PHASE)
    ref = hand_chain(DC.MU0, DC.T_AER, DC.RHO, GAS3)
    r = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, raise_on_error=False, **kw)
    assert np.array_equal(r.I, ref["I"]) and np.array_equal(r.n, ref["n"]) and np.array_equal(r.status, ref["status"])
    assert np.array_equal(r.tau, ref["tau"]) and np.array_equal(r.row_weight, ref["w"]) and np.array_equal(r.gas_tau, GAS3)
    assert r.beam_slant is None and not np.array_equal(r.tau, SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, raise_on_error=False, **kw).tau)
    d, _ = solve_batch_device(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, **kw)
    assert np.array_equal(d["I"].cpu().numpy(), ref["I"]) and np.array_equal(d["n"].cpu().numpy(), ref["n"])
    assert np.array_equal(d["row_weight"], ref["w"]) and "beam_slant" not in d
    # one profile [L] for all columns
    r1 = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS, raise_on_error=False, **kw)
    assert np.array_equal(r1.I[0], r.I[0]) and np.array_equal(r1.I, hand_chain(DC.MU0, DC.T_AER, DC.RHO, np.tile(GAS, (3, 1)))["I"])
    # the single column
    c = SOS_Aer(mu0=DC.MU0[0], tauStar_aer=DC.T_AER[0], grd_alb=DC.RHO[0], tauStar_atm=0.124, gas_tau=GAS, **kw)
    one = hand_chain(DC.MU0[:1], DC.T_AER[:1], DC.RHO[:1], GAS[None, :])
    assert np.array_equal(c.I, one["I"][0]) and c.n == one["n"][0] and c.I_saved is None and np.array_equal(c.row_weight, one["w"][0])
    # the sphere: the slant path of the total optical depth
    z = np.linspace(120, 0, DC.L)
    ref = hand_chain(DC.MU0, DC.T_AER, DC.RHO, GAS3, z=z)
    r = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, beam="spherical", raise_on_error=False, **kw)
    assert np.array_equal(r.I, ref["I"]) and np.array_equal(r.n, ref["n"]) and np.array_equal(r.beam_slant, ref["beam_slant"])
    DC.fresh()


def test_flux_drivers_are_the_hand_chain():
    from sosrt.forcing import toa_net_flux
    from sosrt.thermal import thermal_toa_flux
    DC.fresh()
    alb = np.array([0.9, 0.95, 1.0])
    got = toa_net_flux(0.5, 0.124, DC.T_AER, 0.1, 1.0, alb, g_aer=0.7, gas_tau=GAS3, **DC.SHAPE)
    # (toa_net_flux takes its phase arrays from the host builders: the hand chain is given the same arrays)
    from sosrt.inputs import direction_grid, phase_function
    mu = direction_grid(DC.N)
    P0a, Pa = phase_function("rayleigh", DC.N, mu, 0.5, 0.0)
    P0r, Pr = phase_function("hg", DC.N, mu, 0.5, 0.7)
    ref = hand_chain(np.full(3, 0.5), DC.T_AER, np.full(3, 0.1), GAS3, alb_aer=alb, want=("net_toa",), phases=(Pa, Pr, P0a, P0r))
    assert np.array_equal(got, ref["net_toa"])
    assert not np.array_equal(got, toa_net_flux(0.5, 0.124, DC.T_AER, 0.1, 1.0, alb, g_aer=0.7, **DC.SHAPE))
    z = np.linspace(120, 0, DC.L)
    ref = hand_chain(np.full(3, 0.5), DC.T_AER, np.full(3, 0.1), GAS3, alb_aer=alb, z=z, want=("net_toa",), phases=(Pa, Pr, P0a, P0r))
    assert np.array_equal(toa_net_flux(0.5, 0.124, DC.T_AER, 0.1, 1.0, alb, g_aer=0.7, gas_tau=GAS3, beam="spherical", **DC.SHAPE),
                          ref["net_toa"])
    # the thermal flux: bit for bit the hand chain
    th = (DC.PLANCK, DC.THERMAL["planck_surface"])
    ref = hand_chain(np.full(3, 0.5), DC.GREY_T_AER, DC.RHO, GAS3, t_atm=0.125, alb_atm=0.5, alb_aer=0.8, thermal=th, want=("flux_up",))
    got = thermal_toa_flux(DC.GREY_T_AER, DC.RHO, DC.PLANCK, th[1], gas_tau=GAS3, **DC.GREY, **DC.SHAPE, **DC.PHASE)
    assert np.array_equal(got, ref["flux_up"][:, 0])
    plain = thermal_toa_flux(DC.GREY_T_AER, DC.RHO, DC.PLANCK, th[1], **DC.GREY, **DC.SHAPE, **DC.PHASE)
    assert not np.array_equal(got, plain)
    DC.fresh()


def band_thermal_hand_chain(edges, Tz, Ts, t_aer, rho, gas, grey):
    """What band_thermal(gas_tau=[K, L]) stands for, call by call on the cached handle, K points x C columns in one solve: the
    Planck stage, the columns on the total optical depth, the weights, the emission with them, the solve from it, the emission
    epilogue, the weighted sum over the points (weights one, the Planck stage's scales)."""
    from sosrt import main
    torch = _torch()
    lo, hi = edges
    K, C, L = len(lo), len(t_aer), DC.L
    B = K * C
    s = main.get_solver(L, DC.N, B, 256, 0)
    per_point = lambda a: np.tile(np.broadcast_to(np.asarray(a, dtype=np.float64), (C,)), K)
    ns = main._gas_args(np.repeat(gas, C, axis=0), B, L)
    _, tau, _, _, _, _, _, _ = main._prepare_batch(np.full(B, 0.5), per_point(t_aer), per_point(rho), per_point(grey["tauStar_atm"]),
                                                   per_point(grey["alb_atm"]), per_point(grey["alb_aer"]), 120, 25, 17, L, DC.N, "rayleigh",
                                                   0.0, "hg", 0.7, None, None, None, None, None, None, "specular", 256, 0, gas=ns)
    names = ("flux_down", "flux_up", "heating_rate", "net_toa")
    with main._on_torch_stream(s, 0) as dv:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dv)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dv)
        d_T, d_Ts = up(np.broadcast_to(Tz, (C, L))), up(np.broadcast_to(Ts, (C,)))
        d_pl, d_bs, d_scale = new(K, C, L), new(K, C), new(K, C)
        s.planck_bands_device(d_T.data_ptr(), d_Ts.data_ptr(), lo, hi, d_pl.data_ptr(), d_bs.data_ptr(), d_scale.data_ptr(), C=C)
        d_tau, d_w, d_z, d_ones = up(tau), up(ns.w), up(np.linspace(120, 0, L)), up(np.ones((K, C)))
        d_I0, d_I = new(B, L, s.D), new(B, L, s.D)
        d_n, d_st = torch.zeros(B, dtype=torch.int32, device=dv), torch.zeros(B, dtype=torch.int32, device=dv)
        buf = {k: new(B, 1 if k == "net_toa" else L) for k in names}
        out = {k: new(C, 1 if k == "net_toa" else L) for k in names}
        try:
            s.set_row_weights_device(d_w.data_ptr(), d_w.data_ptr(), B=B)
            s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr(), B=B)
            s.solve_device(d_tau.data_ptr(), 0, 0, d_I.data_ptr(), d_I1=d_I0.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), buf["flux_down"].data_ptr(), buf["flux_up"].data_ptr(),
                                       0, buf["heating_rate"].data_ptr(), buf["net_toa"].data_ptr(), B=B)
            for k in names:
                s.band_reduce_device(buf[k].data_ptr(), out[k].data_ptr(), C, K, out[k].shape[1], d_ones.data_ptr(), d_scale.data_ptr())
            s.synchronize()
        finally:
            s.set_row_weights_device(0, 0)
        r = {k: v.cpu().numpy() for k, v in out.items()}
        r["net_toa"] = r["net_toa"][:, 0]
        r["point_net_toa"] = buf["net_toa"].cpu().numpy().reshape(K, C) * d_scale.cpu().numpy()
        r["n"], r["status"] = d_n.cpu().numpy().reshape(K, C), d_st.cpu().numpy().reshape(K, C)
    return r


BAND_EDGES = (np.array([500.0, 700.0]), np.array([700.0, 900.0]))
BAND_T = np.maximum(288.0 - 6.5 * np.linspace(120, 0, DC.L), 216.5)
BAND_GAS = np.stack([GAS, 3 * GAS])


def test_band_thermal_with_a_profile_per_point():
    """K = 2 points, each its own gas profile, against the hand chain of Solver calls bit for bit: the summed outputs, every
    point's net flux, the order counts.  Then the driver against itself: the sum does not depend on how the points are chunked,
    a point is its own single-point call, [K, C, L] is [K, L] per column."""
    from sosrt.bands import band_thermal
    DC.fresh()
    kw = dict(DC.GREY, **DC.SHAPE, **DC.PHASE)
    ref = band_thermal_hand_chain(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER, DC.RHO, BAND_GAS, DC.GREY)
    assert np.all(ref["status"] == 0)
    DC.fresh()
    both = band_thermal(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO, gas_tau=BAND_GAS, per_point=True, **kw)
    for k in ("flux_up", "flux_down", "heating_rate", "net_toa", "point_net_toa", "n", "status"):
        assert np.array_equal(getattr(both, k), ref[k]), k
    one_by_one = band_thermal(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO, gas_tau=BAND_GAS, per_point=True, points_per_solve=1, **kw)
    for k in ("flux_up", "flux_down", "heating_rate", "net_toa", "point_net_toa", "n"):
        assert np.array_equal(getattr(both, k), getattr(one_by_one, k)), k
    for k in range(2):
        single = band_thermal((BAND_EDGES[0][k:k + 1], BAND_EDGES[1][k:k + 1]), BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO,
                              gas_tau=BAND_GAS[k:k + 1], per_point=True, **kw)
        assert np.array_equal(single.point_net_toa[0], both.point_net_toa[k]) and np.array_equal(single.n[0], both.n[k])
    full = band_thermal(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO, gas_tau=np.repeat(BAND_GAS[:, None, :], 3, axis=1), per_point=True, **kw)
    assert np.array_equal(full.flux_up, both.flux_up)
    plain = band_thermal(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO, per_point=True, **kw)
    assert not np.array_equal(plain.flux_up, both.flux_up)
    DC.fresh()


def test_band_solar_with_a_profile_per_point():
    """Every point's net flux is the hand chain's of the K C columns, bit for bit; the sum is their weighted sum."""
    from sosrt.bands import band_solar
    DC.fresh()
    K, C = 2, 3
    flux = np.array([1.5, 0.5])
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=1.0, **DC.SHAPE, **DC.PHASE)
    got = band_solar(flux, DC.MU0, DC.T_AER[None, :], DC.RHO, gas_tau=BAND_GAS, per_point=True, want=("net_toa", "flux_up"), **kw)
    ref = hand_chain(np.tile(DC.MU0, K), np.tile(DC.T_AER, K), np.tile(DC.RHO, K), np.repeat(BAND_GAS, C, axis=0), want=("net_toa", "flux_up"))
    assert np.array_equal(got.point_net_toa, ref["net_toa"].reshape(K, C)) and np.array_equal(got.n, ref["n"].reshape(K, C))
    fu = ref["flux_up"].reshape(K, C, DC.L)
    want = np.zeros((C, DC.L))
    for k in range(K):
        want = want + flux[k] * fu[k]
    assert _err(got.flux_up, want) <= 1e-14
    assert not np.array_equal(got.point_net_toa, band_solar(flux, DC.MU0, DC.T_AER[None, :], DC.RHO, per_point=True, want=("net_toa",), **kw).point_net_toa)
    DC.fresh()


def test_forcing_forms_pass_the_gas_on():
    """The four forcing forms are differences of the flux drivers above, which the hand chain pins: bit for bit those differences,
    the baseline column keeping the gas."""
    from sosrt.bands import band_solar, band_solar_forcing, band_thermal, band_thermal_forcing
    from sosrt.forcing import radiative_forcing, toa_net_flux
    from sosrt.thermal import thermal_forcing, thermal_toa_flux
    DC.fresh()
    alb = np.array([0.9, 0.95, 1.0])
    fk = dict(g_aer=0.7, **DC.SHAPE)
    flux = lambda t, a, g: toa_net_flux(0.5, 0.124, t, 0.1, 1.0, a, gas_tau=g, **fk)
    # one profile for all columns: one baseline; a profile per column: a baseline per column
    assert np.array_equal(radiative_forcing(0.5, 0.124, DC.T_AER, 0.1, 1.0, alb, gas_tau=GAS, **fk),
                          flux(DC.T_AER, alb, GAS) - flux([0.0], [1.0], GAS)[0])
    assert np.array_equal(radiative_forcing(0.5, 0.124, DC.T_AER, 0.1, 1.0, alb, gas_tau=GAS3, **fk),
                          flux(DC.T_AER, alb, GAS3) - flux(np.zeros(3), np.ones(3), GAS3))
    th = (DC.PLANCK, DC.THERMAL["planck_surface"])
    tk = dict(DC.GREY, **DC.SHAPE, **DC.PHASE)
    assert np.array_equal(thermal_forcing(DC.GREY_T_AER, DC.RHO, *th, gas_tau=GAS3, **tk),
                          thermal_toa_flux(np.zeros(3), DC.RHO, *th, gas_tau=GAS3, **tk) - thermal_toa_flux(DC.GREY_T_AER, DC.RHO, *th, gas_tau=GAS3, **tk))
    two = lambda a: np.concatenate((a, a), axis=-1)
    r = band_thermal(BAND_EDGES, BAND_T, 288.0, np.concatenate((DC.GREY_T_AER, np.zeros(3)))[None, :], two(DC.RHO),
                     gas_tau=np.repeat(BAND_GAS[:, None, :], 6, axis=1), want=("flux_up",), **tk)
    assert np.array_equal(band_thermal_forcing(BAND_EDGES, BAND_T, 288.0, DC.GREY_T_AER[None, :], DC.RHO, gas_tau=BAND_GAS, **tk),
                          r.flux_up[3:, 0] - r.flux_up[:3, 0])
    sk = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=1.0, **DC.SHAPE, **DC.PHASE)
    r = band_solar(np.array([1.5, 0.5]), two(DC.MU0), np.concatenate((DC.T_AER, np.zeros(3)))[None, :], two(DC.RHO),
                   gas_tau=np.repeat(BAND_GAS[:, None, :], 6, axis=1), want=("net_toa",), **sk)
    assert np.array_equal(band_solar_forcing(np.array([1.5, 0.5]), DC.MU0, DC.T_AER[None, :], DC.RHO, gas_tau=BAND_GAS, **sk),
                          r.net_toa[:3] - r.net_toa[3:])
    DC.fresh()


def test_thermal_batch_and_aerosol_sets_with_gas():
    """SOS_Aer_batch(source='thermal', gas_tau=) against the hand chain bit for bit; and several aerosols in one batch under gas --
    the two-pass contraction with phase sets, regrouped when the weights are set and restored when they are cleared: every column
    against the batch of its own aerosol alone (1e-10, equal n; bit-equality reported), and a plain aer_set call afterwards with
    the bits it had before."""
    from sosrt.main import SOS_Aer_batch
    DC.fresh()
    kw = dict(DC.SHAPE, **DC.PHASE)
    ref = hand_chain(DC.MU0, DC.GREY_T_AER, DC.RHO, GAS3, t_atm=0.125, alb_atm=0.5, alb_aer=0.8,
                     thermal=(DC.PLANCK, DC.THERMAL["planck_surface"]))
    r = SOS_Aer_batch(DC.MU0, DC.GREY_T_AER, DC.RHO, gas_tau=GAS3, raise_on_error=False, **DC.GREY, **DC.THERMAL, **kw)
    assert np.array_equal(r.I, ref["I"]) and np.array_equal(r.n, ref["n"]) and np.array_equal(r.status, ref["status"])
    DC.fresh()
    sets = np.array([0, 1, 0])
    two = dict(DC.SHAPE, **DC.TWO_AEROSOLS)
    before = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, aer_set=sets, raise_on_error=False, **two)
    mixed = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, aer_set=sets, gas_tau=GAS3, raise_on_error=False, **two)
    after = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, aer_set=sets, raise_on_error=False, **two)
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n)
    assert list(mixed.status) == [0, 0, 0] and not np.array_equal(mixed.I, before.I)
    for k, (name, g) in enumerate(zip(DC.TWO_AEROSOLS["aer_phase_fun"], DC.TWO_AEROSOLS["g_aer"])):
        c = np.flatnonzero(sets == k)
        DC.fresh()
        one = SOS_Aer_batch(DC.MU0[c], DC.T_AER[c], DC.RHO[c], gas_tau=GAS3[c], raise_on_error=False, atm_phase_fun="rayleigh",
                            aer_phase_fun=name, g_aer=g, **DC.SHAPE)
        e = max(rel_err(mixed.I[b], one.I[i]) for i, b in enumerate(c))
        print("aerosol %d (%s) under gas: the mixed batch against its own batch %.3e (bit-equal: %s)" % (k, name, e, np.array_equal(mixed.I[c], one.I)))
        assert np.array_equal(mixed.n[c], one.n) and e <= RTOL
    DC.fresh()


def test_no_gas_leaves_the_drivers_as_they_were():
    """gas_tau=None and a call after a gas call: I and n of the plain call, bit for bit (the weights were cleared, the grouping restored)."""
    from sosrt.main import SOS_Aer_batch
    DC.fresh()
    kw = dict(DC.SHAPE, **DC.PHASE)
    before = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, raise_on_error=False, **kw)
    SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, raise_on_error=False, **kw)
    after = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=None, raise_on_error=False, **kw)
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n) and np.array_equal(before.tau, after.tau)
    assert after.gas_tau is None and after.row_weight is None
    DC.fresh()
