"""Thermal emission on the device (csrc/emission.hip, csrc/api_emission.hip) through the C ABI: the emitted
field on the grid and at view cosines and the emission epilogue against the NumPy model of tests/thermal_np.py (which
tests/test_thermal_host.py pins to closed forms and runs through the oracle), whole solves against the oracle fed the model's
field, every refusal, the handle's state, and the drivers."""
import functools

import numpy as np
import pytest

import sos_oracle as O
import thermal_np as T
import view_np
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

SURFACES = ["specular", "lambertian", "lambertian_readme"]
RTOL = 1e-10


def _torch():
    return pytest.importorskip("torch")


def dev(a, dtype=np.float64):
    torch = _torch()
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(torch.device("cuda", 0))    # (a copy: cached references are read-only)


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


def handle(cols, phase=True, max_orders=64, mu0=None):
    """A handle with the oracle columns `cols` (one shape and surface, Rayleigh + HG) set: (solver, tau [B, L])."""
    c0 = cols[0]
    L, N, B = len(c0.tau), c0.N, len(cols)
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(c0.mu)
    if phase:
        s.set_phase(c0.P_atm, c0.P_aer)
    col = lambda f: [f(c) for c in cols]
    m0 = col(lambda c: c.mu0) if mu0 is None else [mu0] * B
    if c0.zone_table is None:
        s.set_columns(col(lambda c: c.idx_up), col(lambda c: c.idx_down), m0, col(lambda c: c.grd_alb),
                      col(lambda c: c.alb_atm), col(lambda c: c.alb_aer), col(lambda c: c.dtau_atm), col(lambda c: c.dtau_aer),
                      col(lambda c: c.tauStar_tot), surface=c0.surface)
    else:
        s.set_columns_zones(np.array([[z.r0 for z in c.zone_table] for c in cols]), [int(z.kind == "mix") for z in c0.zone_table],
                            m0, col(lambda c: c.grd_alb), col(lambda c: c.alb_atm), col(lambda c: c.dtau_atm),
                            np.array([[z.alb_aer for z in c.zone_table] for c in cols]),
                            np.array([[z.dtau_aer for z in c.zone_table] for c in cols]), col(lambda c: c.tauStar_tot),
                            surface=c0.surface)
    return s, np.stack([c.tau for c in cols])


def run_emission(s, tau, planck, bs, es=None, B=None):
    d = [dev(x) for x in (tau, planck, bs)]
    d_es = None if es is None else dev(es)
    d_I0 = dfull(tau.shape + (s.D,))
    sync()
    s.emission_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_I0.data_ptr(), 0 if d_es is None else d_es.data_ptr(), B=B)
    return host(d_I0, s)


def run_view(s, tau, planck, bs, mu_view, levels, es=None):
    d = [dev(x) for x in (tau, planck, bs)]
    d_es = None if es is None else dev(es)
    d_out = dfull((tau.shape[0], np.size(levels), 2 * np.size(mu_view)))
    sync()
    s.emission_view_device(mu_view, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), levels, d_out.data_ptr(),
                           0 if d_es is None else d_es.data_ptr())
    return host(d_out, s)


# ---- the columns of the kernel tests: per (shape, surface), shared by the tests and never changed ------------------------------
# (N, L, B, slabs): (96, 24, 2) is two waves per column: the Lambertian sum crosses waves; N = 33 is odd; B = 70 cycles
SHAPES = {"N32-L24-B3": (32, 24, 3, None), "N33-L24-B3": (33, 24, 3, None), "N64-L24-B3": (64, 24, 3, None),
          "N96-L24-B2": (96, 24, 2, None), "N32-L48-B3-2slabs": (32, 48, 3, T.TWO_SLABS), "N32-L24-B70": (32, 24, 70, None)}
# (rho, tauStar_atm, alb_atm, tauStar_aer, alb_aer): the second column has a black ground, the third an atmosphere of 1e-6, whose
# layers take the small-x branch of the weights on every lane
BASE = [(0.3, 1.0, 0.2, 0.3, 0.6), (0.0, 0.5, 0.0, 0.3, 0.9), (0.5, 1e-6, 0.3, 2e-6, 0.7)]


@functools.lru_cache(maxsize=None)
def shape_columns(name, surface):
    N, L, B, slabs = SHAPES[name]
    par = [BASE[b] if b < 3 else (0.1 * (b % 6), 0.05 + 0.03 * b, 0.01 * (b % 50), 0.02 * (b % 11), 0.1 * (b % 10)) for b in range(B)]
    if B == 2:
        par = [BASE[0], BASE[2]]
    return tuple(T.column(O, N, L, r, ta, wa, tr, wr, surface, slabs) for r, ta, wa, tr, wr in par)


@functools.lru_cache(maxsize=None)
def shape_sources(name):
    """(planck [B, L], planck_surface [B], an explicit emissivity [B])"""
    N, L, B, _ = SHAPES[name]
    b = np.arange(B)
    out = (T.planck_profile(L)[None, :] * (1 + 0.1 * b[:, None]), 1 + 0.05 * b, 0.95 - 0.01 * (b % 40))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shape_model(name, surface, explicit):
    cols = shape_columns(name, surface)
    pl, bs, es = shape_sources(name)
    I0 = np.stack([T.emission(c, pl[b], bs[b], es[b] if explicit else None) for b, c in enumerate(cols)])
    I0.setflags(write=False)
    return I0


# ---- a. the emission kernel against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_emission_kernel_against_the_model(name, surface):
    cols = shape_columns(name, surface)
    pl, bs, es = shape_sources(name)
    s, tau = handle(cols, phase=False)
    for explicit in (False, True):
        ref = shape_model(name, surface, explicit)
        got = run_emission(s, tau, pl, bs, es if explicit else None)
        assert np.all(np.isfinite(got))
        worst = max(_err(got[b], ref[b]) for b in range(len(cols)))
        print("%s %s emissivity %s: emission kernel vs model %.3e of the field maximum" %
              (name, surface, "given" if explicit else "1 - rho", worst))
        assert worst <= 1e-12
    if len(cols) > 2:
        assert np.array_equal(run_emission(s, tau[:2], pl[:2], bs[:2], B=2), run_emission(s, tau, pl, bs)[:2])   # the first columns alone
    s.close()


# ---- b. the two known answers on the device -------------------------------------------------------------------------------------------
def test_known_answers_on_the_device():
    N, L = 32, 24
    c = T.column(O, N, L, 0.0, 1.0, 0.0, 0.3, 0.0)           # omega = 0 everywhere, black ground
    s, tau = handle([c], phase=False)
    a = np.abs(c.mu[:N - 1])
    att = 1 - np.exp(-c.tau[:, None] / a)
    one = np.ones(1)
    got = run_emission(s, tau, np.ones((1, L)), one, one)[0]
    e_up, e_dn = np.max(np.abs(got[:, N:] - 1)), np.max(np.abs(got[:, :N - 1] - att))
    print("isothermal: upward lanes - 1: %.3e, downward lanes - (1 - e^{-tau/a}): %.3e" % (e_up, e_dn))
    assert e_up <= 1e-13 and e_dn <= 1e-13 and np.all(got[:, N - 1] == 1)
    got = run_emission(s, tau, (0.5 + 0.8 * c.tau)[None, :], one, one)[0]
    ref = 0.5 * att + 0.8 * (c.tau[:, None] - a * att)
    e = np.max(np.abs(got[:, :N - 1] - ref))
    print("b = 0.5 + 0.8 tau: downward lanes vs the closed form %.3e" % e)
    assert e <= 1e-13
    s.close()


# ---- c. whole solves ---------------------------------------------------------------------------------------------------------------------
def solve_dev(s, d_tau, d_P0a, d_P0r, d_I1=None):
    torch = _torch()
    B, L = d_tau.shape
    d_I = dfull((B, L, s.D))
    d_n = torch.zeros(B, dtype=torch.int32, device=d_tau.device)
    d_st = torch.zeros(B, dtype=torch.int32, device=d_tau.device)
    sync()
    s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_I1=0 if d_I1 is None else d_I1.data_ptr(),
                   d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
    s.synchronize()
    return d_I.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()


@functools.lru_cache(maxsize=None)
def whole_oracle(i):
    c = T.solve_column_case(O, T.SOLVE_CASES[i])
    L = len(c.tau)
    r = O.solve_column(c, literal=False, I1=T.emission(c, T.planck_profile(L), 1.0))
    r.I.setflags(write=False)
    return c, r


def thermal_dev(s, c, tau):
    L = len(c.tau)
    d_tau, d_pl, d_bs = dev(tau), dev(T.planck_profile(L)[None, :]), dev(np.ones(1))
    d_P0a, d_P0r = dev(c.P0_atm[None, :]), dev(c.P0_aer[None, :])
    d_I0 = dfull((1, L, s.D))
    sync()
    s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr())
    return solve_dev(s, d_tau, d_P0a, d_P0r, d_I0)


@pytest.mark.parametrize("i", range(len(T.SOLVE_CASES)), ids=lambda i: "N%d-L%d-%s%s" % (T.SOLVE_CASES[i][:2] + (T.SOLVE_CASES[i][7], "-2slabs" if T.SOLVE_CASES[i][8] else "")))
def test_whole_solves(i):
    c, ref = whole_oracle(i)
    assert ref.n == T.SOLVE_CASES[i][-1]
    s, tau = handle([c])
    I, n, st = thermal_dev(s, c, tau)
    e = _err(I[0], ref.I)
    print("%s: thermal solve n = %d (oracle %d), field %.3e of its maximum" % (T.SOLVE_CASES[i][:2], n[0], ref.n, e))
    assert st[0] == 0 and n[0] == ref.n
    assert e <= RTOL
    s.close()
    # the same column set with another mu0: the sun does not enter
    s, tau = handle([c], mu0=0.83)
    I2, n2, _ = thermal_dev(s, c, tau)
    e = _err(I2[0], I[0])
    print("%s: mu0 = 0.83 against mu0 = %g: %.3e" % (T.SOLVE_CASES[i][:2], c.mu0, e))
    assert n2[0] == n[0] and e <= 1e-13
    s.close()


# ---- d. the view kernel ------------------------------------------------------------------------------------------------------------------
def test_view_kernel_at_node_cosines_is_the_grid_kernel():
    name, N, L = "N33-L24-B3", 33, 24
    cols = shape_columns(name, "specular")
    pl, bs, es = shape_sources(name)
    s, tau = handle(cols, phase=False)
    k = np.array([1, 5, 16, 32])
    mu_view = cols[0].mu[N + k]
    lev = np.arange(L)
    for e_ in (None, es):
        grid = run_emission(s, tau, pl, bs, e_)
        got = run_view(s, tau, pl, bs, mu_view, lev, e_)
        ref = np.concatenate((grid[:, :, N - 1 - k], grid[:, :, N + k]), axis=2)
        e = _err(got, ref)
        print("view lanes at node cosines vs the grid kernel %.3e" % e)
        assert e <= 1e-12
    s.close()


VIEW_MU = {1: np.array([0.01]), 5: np.array([0.01, 0.123, 0.5, 0.77, 1.0]),
           17: np.concatenate(([0.01], 0.013 + 0.06 * np.arange(15), [1.0]))}


@pytest.mark.parametrize("name,V", [("N33-L24-B3", 5), ("N33-L24-B3", 17), ("N32-L24-B70", 1)])
def test_view_kernel_off_the_grid_against_the_model(name, V):
    cols = shape_columns(name, "specular")
    pl, bs, es = shape_sources(name)
    L = SHAPES[name][1]
    s, tau = handle(cols, phase=False)
    # V = 5: 300 levels (rows repeat), more than one launch of the sweeps takes
    lev = np.arange(300) % L if V == 5 else np.array([0, L // 2, L - 1])
    got = run_view(s, tau, pl, bs, VIEW_MU[V], lev, es)
    assert np.all(np.isfinite(got))
    ref = np.stack([T.emission_view(c, pl[b], bs[b], VIEW_MU[V], lev, es[b]) for b, c in enumerate(cols)])
    worst = max(_err(got[b], ref[b]) for b in range(len(cols)))
    print("%s V=%d: view kernel vs model %.3e" % (name, V, worst))
    assert worst <= 1e-12
    s.close()


def test_view_kernel_isothermal():
    c = T.column(O, 33, 24, 0.0, 1.0, 0.0, 0.3, 0.0)
    s, tau = handle([c], phase=False)
    got = run_view(s, tau, np.ones((1, 24)), np.ones(1), VIEW_MU[5], np.arange(24), np.ones(1))[0]
    e = np.max(np.abs(got[:, 5:] - 1))
    print("isothermal, view lanes: upward - 1: %.3e" % e)
    assert e <= 1e-13
    assert np.max(np.abs(got[:, :5] - (1 - np.exp(-c.tau[:, None] / VIEW_MU[5])))) <= 1e-13
    s.close()


# ---- e. the emission epilogue ---------------------------------------------------------------------------------------------------------
EPI = ("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")


def run_epilogue(s, tau, I, z, sigma=None):
    B, L = tau.shape
    d_tau, d_I, d_z = dev(tau), dev(I), dev(z)
    out = {k: dfull((B,) if k == "net_toa" else (B, L)) for k in EPI}
    sync()
    p = [out[k].data_ptr() for k in EPI]
    if sigma is None:
        s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), *p)
    else:
        d_sig = dev(sigma)
        s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), d_z.data_ptr(), "crit", *p)
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["N32-L24-B3", "N33-L24-B3", "N32-L48-B3-2slabs"])
def test_emission_epilogue(name):
    cols = shape_columns(name, "specular")
    I = shape_model(name, "specular", False)
    L = len(cols[0].tau)
    z = T.altitudes(L)
    s, tau = handle(cols, phase=False)
    got = run_epilogue(s, tau, I, z)
    for b, c in enumerate(cols):
        slabs = [(zn.r0, zn.r1) for zn in c.zones if zn.kind == "mix"]
        ref = T.epilogue_emission(I[b], c.mu, c.N, z_profile=z, slabs=slabs)
        for k in EPI:
            # The heating rate differences the flux between two levels.  Column 2's atmosphere has tau* = 3e-6: its fluxes differ
            # by 1e-6 of themselves from level to level, so 1e-10 of the heating rate would ask 1e-16 of a 32-term trapezoid sum --
            # below the rounding of double precision.  Its fluxes are checked, its heating rate is not.
            if k == "heating_rate" and c.tauStar_tot < 1e-3:
                continue
            e = _err(np.atleast_1d(got[k][b]), np.atleast_1d(ref[k]))
            print("%s column %d %s: emission epilogue vs NumPy %.3e" % (name, b, k, e))
            assert e <= 1e-10, (k, b, e)
    # the beam epilogue on a path of 1e300, where both beam terms vanish
    beam = run_epilogue(s, tau, I, z, np.full(tau.shape, 1e300))
    for k in EPI:
        e = _err(got[k], beam[k])
        print("%s %s: emission epilogue vs the beam epilogue at sigma = 1e300: %.3e" % (name, k, e))
        assert e <= 1e-12, k
    s.close()


# ---- f. refusals: SOSRT_E_INVALID, a message, outputs untouched ------------------------------------------------------------------------
def _refused(call, outputs, s, word=None):
    with pytest.raises(ValueError) as ei:
        call()
    assert str(ei.value), "a refusal carries a message"
    if word:
        assert word in str(ei.value), str(ei.value)
    for o in outputs:
        assert np.all(np.isnan(host(o, s))), "a refused call wrote to an output"


def test_refusals_leave_the_outputs_untouched():
    name, L = "N32-L24-B3", 24
    cols = shape_columns(name, "specular")
    pl, bs, es = shape_sources(name)
    I = shape_model(name, "specular", False)
    s, tau = handle(cols, phase=False)
    d_tau, d_pl, d_bs, d_I = dev(tau), dev(pl), dev(bs), dev(I)
    o_I0, o_v, o_f = dfull((3, L, s.D)), dfull((3, 2, 4)), dfull((3, L))
    outs = [o_I0, o_v, o_f]
    sync()
    emi = lambda **k: s.emission_device(k.get("tau", d_tau.data_ptr()), k.get("pl", d_pl.data_ptr()), k.get("bs", d_bs.data_ptr()),
                                        k.get("out", o_I0.data_ptr()), B=k.get("B"))
    view = lambda **k: s.emission_view_device(k.get("mu", [0.3, 0.7]), k.get("tau", d_tau.data_ptr()), k.get("pl", d_pl.data_ptr()),
                                              k.get("bs", d_bs.data_ptr()), k.get("lev", [0, L - 1]), k.get("out", o_v.data_ptr()),
                                              B=k.get("B"))
    epi = lambda **k: s.epilogue_emission_device(k.get("tau", d_tau.data_ptr()), k.get("I", d_I.data_ptr()), k.get("z", 0),
                                                 o_f.data_ptr(), d_heating_rate=k.get("hr", 0), B=k.get("B"))
    for B in (0, 4, -1):
        for call in (emi, view, epi):
            _refused(lambda: call(B=B), outs, s, "B=")
    for k in ("tau", "pl", "bs", "out"):
        _refused(lambda: emi(**{k: 0}), outs, s, "null")
        _refused(lambda: view(**{k: 0}), outs, s, "null")
    for k in ("tau", "I"):
        _refused(lambda: epi(**{k: 0}), outs, s, "null")
    _refused(lambda: epi(hr=o_f.data_ptr()), outs, s, "z_profile")
    # view cosines and levels outside the limits of the view stage
    _refused(lambda: view(mu=np.linspace(0.1, 1, 65)), outs, s, "V=")
    _refused(lambda: view(mu=[]), outs, s, "V=")
    for bad in (0.009, 1.01, -0.5, float("nan"), float("inf")):
        _refused(lambda: view(mu=[0.5, bad]), outs, s, "mu_view")
    for bad in ([-1], [L], [0, 99]):
        _refused(lambda: view(lev=bad), outs, s, "levels")
    _refused(lambda: view(lev=[]), outs, s, "levels")
    # the stage still works on this handle, and then writes
    emi()
    view()
    epi()
    assert all(np.all(np.isfinite(host(o, s))) for o in outs)
    s.close()
    # a Lambertian surface in the view call
    for surface in SURFACES[1:]:
        s, _ = handle(shape_columns(name, surface), phase=False)
        o = dfull((3, 2, 4))
        sync()
        _refused(lambda: s.emission_view_device([0.3, 0.7], d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), [0, L - 1], o.data_ptr()),
                 [o], s, "Lambertian")
        s.close()
    # single-slab geometry
    s = Solver(L, 32, max_batch=3)
    s.set_grid(O.make_mu(32))
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.4)
    outs = [dfull((3, L, s.D)), dfull((3, 2, 4)), dfull((3, L))]
    sync()
    _refused(lambda: s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), outs[0].data_ptr()), outs, s, "slab")
    _refused(lambda: s.emission_view_device([0.3, 0.7], d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), [0, L - 1], outs[1].data_ptr()),
             outs, s, "slab")
    _refused(lambda: s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), 0, outs[2].data_ptr()), outs, s, "slab")
    s.close()


def test_layers_beyond_the_lds_limit_are_refused():
    L = 2049
    iu, idn = O.slab_indices(T.Z0, 25, 17, L)
    s = Solver(L, 32, max_batch=1)
    s.set_grid(O.make_mu(32))
    s.set_columns([iu], [idn], 0.5, 0.3, 0.5, 0.6, 1.0 / L, 0.3 / (idn + 1 - iu), 1.3)
    d_tau, d_bs = dev(np.zeros((1, L))), dev(np.ones(1))
    outs = [dfull((1, L, s.D)), dfull((1, 1, 2)), dfull((1, L))]
    sync()
    _refused(lambda: s.emission_device(d_tau.data_ptr(), d_tau.data_ptr(), d_bs.data_ptr(), outs[0].data_ptr()), outs, s, "L=")
    _refused(lambda: s.emission_view_device([0.5], d_tau.data_ptr(), d_tau.data_ptr(), d_bs.data_ptr(), [0], outs[1].data_ptr()), outs, s, "L=")
    _refused(lambda: s.epilogue_emission_device(d_tau.data_ptr(), outs[0].data_ptr(), 0, outs[2].data_ptr()), outs, s, "L=")
    s.close()


# ---- g. the stage leaves the handle as it was --------------------------------------------------------------------------------------------
def test_the_stage_leaves_the_handle_untouched():
    c, _ = whole_oracle(0)
    c2 = T.column(O, 32, 24, 0.3, 1.0, 0.0, 0.3, 0.6)
    cols = [c, c2]
    L = 24
    z = T.altitudes(L)
    s, tau = handle(cols)
    P0a, P0r = np.stack([x.P0_atm for x in cols]), np.stack([x.P0_aer for x in cols])
    f0 = s.first_order(tau, P0a, P0r)
    r0 = s.solve(tau, P0a, P0r)
    assert np.all(r0.status == 0)
    e0 = s.epilogue(z_profile=z)                                # what the resident field and optical depths give
    # the whole stage on buffers of its own, with other optical depths than the resident ones
    tau2 = tau * 1.25
    pl = np.tile(T.planck_profile(L), (2, 1))
    I0 = run_emission(s, tau2, pl, np.ones(2))
    run_view(s, tau2, pl, np.ones(2), [0.3, 0.7], [0, L - 1])
    run_epilogue(s, tau2, I0, z)
    e1 = s.epilogue(z_profile=z)                                # the resident field and tau: same bytes
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    r1 = s.solve(tau, P0a, P0r)                                 # the columns and the phase state: the same solve, bit for bit
    assert np.array_equal(r0.I, r1.I) and np.array_equal(r0.n, r1.n)
    assert np.array_equal(s.first_order(tau, P0a, P0r), f0)
    # ... also with the README first order set: the stage is not refused there, and the mode stays
    s.set_first_order("readme")
    assert np.array_equal(run_emission(s, tau2, pl, np.ones(2)), I0)
    s.set_first_order("coded")
    s.close()


# ---- h. the drivers --------------------------------------------------------------------------------------------------------------------
DRV = dict(tauStar_atm=1.0, alb_atm=0.1, alb_aer=0.6, z0=T.Z0, nb_layers=24, nb_angles=32, atm_phase_fun="rayleigh",
           aer_phase_fun="hg", g_aer=T.G_AER)
DRV_COLS = [(0.3, 0.1, 1.0), (0.12, 0.3, 1.1), (0.3, 0.0, 0.9)]    # (tauStar_aer, rho, planck_surface)
DRV_MU0 = 0.5


@functools.lru_cache(maxsize=None)
def driver_oracle(t_aer, rho, bs):
    """(column, oracle solution from the model's emitted field)"""
    c = T.column(O, 32, 24, rho, 1.0, 0.1, t_aer, 0.6, mu0=DRV_MU0)
    r = O.solve_column(c, literal=False, I1=T.emission(c, T.planck_profile(24), bs))
    r.I.setflags(write=False)
    return c, r


def test_driver_on_three_columns(monkeypatch):
    from sosrt import main
    t_aer, rho, bs = (np.array([c[k] for c in DRV_COLS]) for k in range(3))
    pl = T.planck_profile(24)
    plain = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, **DRV)
    solar = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="solar", **DRV)
    assert np.array_equal(solar.I, plain.I) and np.array_equal(solar.n, plain.n)
    th = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="thermal", planck=pl, planck_surface=bs, **DRV)
    assert th.I.shape == plain.I.shape == (3, 24, 64) and th.n.shape == (3,) and th.beam_slant is None
    for b, col in enumerate(DRV_COLS):
        c, ref = driver_oracle(*col)
        e = _err(th.I[b], ref.I)
        print("driver column %s: n = %d (oracle %d), thermal field %.3e of its maximum" % (col, th.n[b], ref.n, e))
        assert th.n[b] == ref.n and th.status[b] == 0
        assert e <= RTOL
    # [B, L] sources and an explicit emissivity give the same field as their broadcast forms
    th2 = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="thermal", planck=np.tile(pl, (3, 1)), planck_surface=bs,
                             surface_emissivity=1 - rho, **DRV)
    assert np.array_equal(th2.I, th.I)
    # the cached handle solves a plain solar batch with its old bits afterwards, also after an error raised in between
    again = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, **DRV)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n)

    def boom(self, *a, **k):
        raise RuntimeError("raised in between")
    with monkeypatch.context() as mp:
        mp.setattr(Solver, "emission_device", boom)
        with pytest.raises(RuntimeError, match="in between"):
            main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="thermal", planck=pl, planck_surface=bs, **DRV)
    again = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, **DRV)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n)
    # the per-order fields of the one-column driver add up to its field
    one = main.SOS_Aer(source="thermal", planck=pl, planck_surface=1.1, mu0=DRV_MU0, grd_alb=0.3, tauStar_aer=0.12, **DRV)
    assert one.I_saved.shape[0] == one.n
    assert _err(one.I, th.I[1]) <= 1e-12 and _err(one.I_saved.sum(axis=0), one.I) <= 1e-12
    assert _err(one.I_saved[0], T.emission(driver_oracle(*DRV_COLS[1])[0], pl, 1.1)) <= 1e-12


def test_other_drivers_take_the_thermal_source():
    from sosrt import main
    t_aer, rho, bs = (np.array([c[k] for c in DRV_COLS]) for k in range(3))
    pl = T.planck_profile(24)
    th = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="thermal", planck=pl, planck_surface=bs, **DRV)
    d, _ = main.solve_batch_device(DRV_MU0, t_aer, rho, source="thermal", planck=pl, planck_surface=bs, **DRV)
    assert np.array_equal(d["I"].cpu().numpy(), th.I) and np.array_equal(d["n"].cpu().numpy(), th.n)
    # one layer through the zone-table driver: the same field to rounding (its columns are a zone table)
    kw = {k: v for k, v in DRV.items() if k != "alb_aer"}
    lay = main.SOS_Aer_layers([DRV_MU0] * 2, rho[[0, 2]], [(25, 17, 0.3, 0.6)], source="thermal", planck=pl, planck_surface=bs[[0, 2]], **kw)
    assert lay.I.shape == (2, 24, 64)
    assert _err(lay.I, th.I[[0, 2]]) <= 1e-12
    sun = main.SOS_Aer_layers([DRV_MU0] * 2, rho[[0, 2]], [(25, 17, 0.3, 0.6)], **kw)
    assert _err(lay.I, sun.I) > 1e-2


def test_driver_view_lanes_with_the_thermal_source():
    from sosrt import main
    t_aer, rho, bs = (np.array([c[k] for c in DRV_COLS]) for k in range(3))
    pl = T.planck_profile(24)
    vmu, lev = np.array([0.05, 0.33, 0.9, 1.0]), [0, 11, 23]
    for quad, qid in (("grid", view_np.QUAD_GRID), ("linear", view_np.QUAD_LINEAR)):
        th = main.SOS_Aer_batch(DRV_MU0, t_aer, rho, source="thermal", planck=pl, planck_surface=bs, view_mu=vmu, view_levels=lev,
                                view_quadrature=quad, **DRV)
        assert th.I_view.shape == th.I_view_first.shape == th.I_view_scattered.shape == (3, 3, 8)
        assert np.array_equal(th.I_view, th.I_view_first + th.I_view_scattered)
        sgn = view_np.signed(vmu)
        assert np.array_equal(th.view_mu_signed, sgn)
        for b, col in enumerate(DRV_COLS):
            c, ref = driver_oracle(*col)
            first = T.emission_view(c, pl, col[2], vmu, lev)
            rows_atm = view_np.phase_rows(view_np.phase_fn("rayleigh"), c.mu, sgn)
            rows_aer = view_np.phase_rows(view_np.phase_fn("hg", T.G_AER), c.mu, sgn)
            scat = view_np.transport(c, view_np.source(c, rows_atm, rows_aer, ref.I), vmu, qid)[lev]
            e1, e2 = _err(th.I_view_first[b], first), _err(th.I_view_scattered[b], scat)
            print("view lanes, %s, column %s: emission %.3e, scattered %.3e" % (quad, col, e1, e2))
            assert e1 <= 1e-12 and e2 <= RTOL


def test_thermal_forcing_against_numpy_on_the_oracle_fields():
    from sosrt import thermal
    t_aer, rho, bs = (np.array([c[k] for c in DRV_COLS]) for k in range(3))
    pl = T.planck_profile(24)
    kw = {k: v for k, v in DRV.items()}
    olr = lambda t, r, b: float(T.epilogue_emission(driver_oracle(t, r, b)[1].I, O.make_mu(32), 32)["flux_up"][0])
    ref = np.array([olr(*c) for c in DRV_COLS])
    ref0 = np.array([olr(0.0, c[1], c[2]) for c in DRV_COLS])
    got = thermal.thermal_toa_flux(t_aer, rho, pl, bs, **kw)
    print("outgoing flux: device %s, NumPy on the oracle fields %s" % (got, ref))
    assert got.shape == (3,) and np.max(np.abs(got - ref)) <= RTOL * np.max(np.abs(ref))
    f = thermal.thermal_forcing(t_aer, rho, pl, bs, **kw)
    print("longwave forcing: device %s, NumPy %s" % (f, ref0 - ref))
    # (a difference of two fluxes each good to 1e-10 of itself: the bar is in units of the flux)
    assert np.max(np.abs(f - (ref0 - ref))) <= 2 * RTOL * np.max(np.abs(ref))
    assert np.all(f > 0)
