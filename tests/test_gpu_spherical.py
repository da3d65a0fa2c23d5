"""Pseudo-spherical direct beam on the device (csrc/beam.hip, csrc/api_beam.hip) through the C ABI: the slant
path, the layer-by-layer first order and the beam epilogue against the NumPy model of tests/spherical_np.py (which
tests/test_spherical_host.py pins to the oracle), the plane path against the coded first order and the plain solve, whole
solves against the oracle fed the model's first order, every refusal, and the drivers."""
import functools

import numpy as np
import pytest

import sos_oracle as O
import spherical_np as S
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

SURFACES = ["specular", "lambertian", "lambertian_readme"]


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


def handle(cols, surface="specular", phase=True, max_orders=64, P_aer_sets=None):
    """A handle with the oracle columns `cols` (one shape, Rayleigh + HG) set: (solver, tau [B, L], P0_atm, P0_aer [B, 2N])."""
    c0 = cols[0]
    L, N, B = len(c0.tau), c0.N, len(cols)
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(c0.mu)
    if P_aer_sets is not None:
        s.set_phase_sets(c0.P_atm, P_aer_sets)
    elif phase:
        s.set_phase(c0.P_atm, c0.P_aer)
    col = lambda f: [f(c) for c in cols]
    if c0.zone_table is None:
        s.set_columns(col(lambda c: c.idx_up), col(lambda c: c.idx_down), col(lambda c: c.mu0), col(lambda c: c.grd_alb),
                      col(lambda c: c.alb_atm), col(lambda c: c.alb_aer), col(lambda c: c.dtau_atm), col(lambda c: c.dtau_aer),
                      col(lambda c: c.tauStar_tot), surface=surface)
    else:
        s.set_columns_zones(np.array([[z.r0 for z in c.zone_table] for c in cols]), [int(z.kind == "mix") for z in c0.zone_table],
                            col(lambda c: c.mu0), col(lambda c: c.grd_alb), col(lambda c: c.alb_atm), col(lambda c: c.dtau_atm),
                            np.array([[z.alb_aer for z in c.zone_table] for c in cols]),
                            np.array([[z.dtau_aer for z in c.zone_table] for c in cols]), col(lambda c: c.tauStar_tot), surface=surface)
    return s, np.stack([c.tau for c in cols]), np.stack([c.P0_atm for c in cols]), np.stack([c.P0_aer for c in cols])


def run_slant(s, tau, z, R=S.EARTH_RADIUS_KM, mu0=None, B=None):
    d_tau, d_z, d_sig = dev(tau), dev(z), dfull(tau.shape)
    d_mu0 = None if mu0 is None else dev(mu0)
    sync()
    s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), R, 0 if d_mu0 is None else d_mu0.data_ptr(), B=B)
    return host(d_sig, s)


def run_first_order(s, tau, sigma, P0a, P0r):
    d = [dev(x) for x in (tau, sigma, P0a, P0r)]
    d_I1 = dfull(tau.shape + (s.D,))
    sync()
    s.first_order_beam_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_I1.data_ptr(), B=tau.shape[0])
    return host(d_I1, s)


# ---- the columns of the kernel tests: per shape, shared by the tests and never changed ----------------------------------------
MU0S = [0.05, 0.21, 0.6, 1.0]
# (N, L, B, slabs): a column at mu0 = 0.05, one with rho = 0, one at a higher sun; B = 70 cycles through sun angles and albedos
SHAPES = {"N32-L24-B3": (32, 24, 3, None), "N33-L24-B3": (33, 24, 3, None), "N64-L24-B3": (64, 24, 3, None),
          "N32-L48-B3-2slabs": (32, 48, 3, S.TWO_SLABS), "N32-L24-B70": (32, 24, 70, None)}


@functools.lru_cache(maxsize=None)
def shape_columns(name):
    N, L, B, slabs = SHAPES[name]
    base = [(0.05, 0.3), (0.6, 0.0), (0.21, 0.5)]
    par = [base[b] if b < 3 else (0.05 + 0.9 * ((7 * b) % 70) / 70.0, 0.1 * (b % 6)) for b in range(B)]
    return tuple(S.column(O, N, L, m, r, slabs) for m, r in par)


@functools.lru_cache(maxsize=None)
def shape_model(name):
    """(sigma [B, L] on the sphere, I1 [B, L, 2N] of the model on it)"""
    cols = shape_columns(name)
    z = S.altitudes(len(cols[0].tau))
    sig = np.stack([S.slant_path(c.tau, z, c.mu0) for c in cols])
    I1 = np.stack([S.first_order_beam(c, sg) for c, sg in zip(cols, sig)])
    sig.setflags(write=False)
    I1.setflags(write=False)
    return sig, I1


# ---- a. the slant kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [S.EARTH_RADIUS_KM, 1e15])
@pytest.mark.parametrize("L,B", [(24, 3), (48, 70), (200, 2)])
def test_slant_kernel_against_the_model(L, B, R):
    # the columns' own sun angles, and a second set handed in as d_mu0: between them every shape sees all of MU0S
    own, other = (np.array([MU0S[(b + k) % 4] for b in range(B)]) for k in (0, 2))
    iu, idn = O.slab_indices(S.Z0, 25, 17, L)
    t_aer = 0.05 + 0.01 * np.arange(B)
    tau = np.stack([O.tau_profile(S.T_ATM, t, S.Z0, 25, 17, L) for t in t_aer])
    z = S.altitudes(L)
    s = Solver(L, 32, max_batch=B)
    s.set_grid(O.make_mu(32))
    s.set_columns(np.full(B, iu), np.full(B, idn), own, 0.3, 1.0, 0.97, S.T_ATM / L, t_aer / (idn + 1 - iu), S.T_ATM + t_aer)
    got = run_slant(s, tau, z, R)
    assert np.array_equal(run_slant(s, tau, z, R, mu0=own), got)
    if B > 2:
        assert np.array_equal(run_slant(s, tau[:2], z, R, B=2), got[:2])    # the first columns alone: the same bits
    for mu0, sig in ((own, got), (other, run_slant(s, tau, z, R, mu0=other))):
        assert np.all(np.isfinite(sig)) and np.all(sig[:, 0] == 0)
        worst = 0.0
        for b in range(B):
            worst = max(worst, _err(sig[b], S.slant_path(tau[b], z, mu0[b], R)))
            if mu0[b] == 1.0:
                assert np.max(np.abs(sig[b] - tau[b])) <= 1e-15, "mu0 = 1 must give tau"
        print("L=%d B=%d R=%g: slant kernel vs model %.3e of max sigma" % (L, B, R, worst))
        assert worst <= 1e-12
        if R == 1e15:
            assert _err(sig, tau / mu0[:, None]) <= 1e-10
    s.close()


# ---- b. the first-order kernel on the sphere's path ------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_first_order_kernel_against_the_model(name, surface):
    cols = shape_columns(name)
    sig, ref = shape_model(name)
    s, tau, P0a, P0r = handle(cols, surface)
    got = run_first_order(s, tau, sig, P0a, P0r)
    assert np.all(np.isfinite(got))
    worst = max(_err(got[b], ref[b]) for b in range(len(cols)))
    print("%s %s: first-order kernel vs model %.3e of the field maximum" % (name, surface, worst))
    assert worst <= 1e-12
    s.close()


# ---- c. the plane path is the coded first order ---------------------------------------------------------------------------------
PIN_GROUPS = {"N32-L24": [c for c in S.FIRST_ORDER_CASES if c[:2] == (32, 24) and len(c) == 4],
              "N33-L24": [c for c in S.FIRST_ORDER_CASES if c[0] == 33], "N32-L48-2slabs": [c for c in S.FIRST_ORDER_CASES if len(c) > 4]}


@pytest.mark.parametrize("group", list(PIN_GROUPS))
def test_plane_path_is_the_coded_first_order(group):
    assert sum(len(v) for v in PIN_GROUPS.values()) == len(S.FIRST_ORDER_CASES)
    cols = [S.column(O, *case) for case in PIN_GROUPS[group]]
    s, tau, P0a, P0r = handle(cols)
    coded = s.first_order(tau, P0a, P0r)
    sig = np.stack([S.plane_path(c.tau, c.mu0) for c in cols])
    got = run_first_order(s, tau, sig, P0a, P0r)
    for b, c in enumerate(cols):
        e = _err(got[b], coded[b])
        print("%s mu0=%g rho=%g: plane path vs sosrt_first_order %.3e" % (group, c.mu0, c.grd_alb, e))
        assert e <= 1e-10
    s.close()


# ---- d. singular lanes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 33])
def test_singular_lanes_are_finite_and_exact(N):
    """sigma = tau / mu_j for a node mu_j makes (1 / a - s) Delta vanish on that lane in every layer; a column whose mu0 IS the
    node also has (1 / a - 1 / mu0) Delta = 0 on the upward lane."""
    mu = O.make_mu(N)
    j, k = N + N // 2, N + 5
    cols = [S.column(O, N, 24, float(mu[j]), 0.3), S.column(O, N, 24, 0.6, 0.3)]
    sig = np.stack([cols[0].tau / mu[j], cols[1].tau / mu[k]])
    ref = np.stack([S.first_order_beam(c, sg) for c, sg in zip(cols, sig)])
    s, tau, P0a, P0r = handle(cols)
    got = run_first_order(s, tau, sig, P0a, P0r)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    for b in range(2):
        assert _err(got[b], ref[b]) <= 1e-12
    s.close()


# ---- e. the per-zone P0_aer layout ------------------------------------------------------------------------------------------------
def test_per_zone_p0_layout_on_a_two_aerosol_column():
    N, L = 32, 48
    mu = O.make_mu(N)
    cols = [S.column(O, N, L, m, r, S.TWO_SLABS) for m, r in ((0.6, 0.3), (0.21, 0.0), (0.83, 0.5))]
    P_sets = np.stack([O.phase_hg(N, mu, 0.6, 0.7)[1], O.phase_hg(N, mu, 0.6, 0.3)[1]])
    s, tau, P0a, _ = handle(cols, P_aer_sets=P_sets)
    nz = len(cols[0].zone_table)
    assert nz == 5
    zset = np.array([0, 0, 0, 1, 0], dtype=np.int32)
    s.set_aerosol_sets(np.tile(zset, (3, 1)))
    P0z = np.zeros((3, nz, 2 * N))
    for b, c in enumerate(cols):
        P0z[b, 1] = O.phase_hg(N, mu, c.mu0, 0.7)[0]
        P0z[b, 3] = O.phase_hg(N, mu, c.mu0, 0.3)[0]
        P0z[b, [0, 2, 4]] = np.nan                           # rows of clear zones are not read
    z = S.altitudes(L)
    sig = np.stack([S.slant_path(c.tau, z, c.mu0) for c in cols])
    ref = np.stack([S.first_order_beam(c, sg, P0_aer_zone=P0z[b]) for b, (c, sg) in enumerate(zip(cols, sig))])
    got = run_first_order(s, tau, sig, P0a, P0z)
    assert np.all(np.isfinite(got))
    for b in range(3):
        assert _err(got[b], ref[b]) <= 1e-12
    # and the two aerosols differ: the one-aerosol model is far from it
    assert _err(S.first_order_beam(cols[0], sig[0]), ref[0]) > 1e-3
    s.close()


# ---- f. whole solves --------------------------------------------------------------------------------------------------------------
WHOLE = [S.SOLVE_CASES[0], S.SOLVE_CASES[3], S.SOLVE_CASES[6]]


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


@pytest.mark.parametrize("case", WHOLE, ids=lambda c: "N%d-L%d-mu0_%g%s" % (c[:3] + ("-2slabs" if len(c) > 4 else "",)))
def test_whole_solves(case):
    c = S.column(O, *case)
    L = len(c.tau)
    z = S.altitudes(L)
    s, tau, P0a, P0r = handle([c])
    d_tau, d_z, d_P0a, d_P0r = dev(tau), dev(z), dev(P0a), dev(P0r)
    d_sig, d_I1 = dfull((1, L)), dfull((1, L, s.D))
    sync()
    # the device's own stage: slant path, first order on it, the order loop fed that first order
    s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr())
    s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr())
    I, n, st = solve_dev(s, d_tau, d_P0a, d_P0r, d_I1)
    ref = O.solve_column(c, literal=False, I1=S.first_order_beam(c, S.slant_path(c.tau, z, c.mu0)))
    e = _err(I[0], ref.I)
    print("%s: spherical solve n = %d (oracle %d), field %.3e" % (case[:4], n[0], ref.n, e))
    assert st[0] == 0 and n[0] == ref.n
    assert e <= 1e-10
    # the plane path through d_I1_in against the plain solve
    d_plane = dev(tau / c.mu0)
    s.first_order_beam_device(d_tau.data_ptr(), d_plane.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr())
    Ip, n_p, _ = solve_dev(s, d_tau, d_P0a, d_P0r, d_I1)
    I0, n0, _ = solve_dev(s, d_tau, d_P0a, d_P0r)
    e = _err(Ip[0], I0[0])
    print("%s: plane path through d_I1_in vs the plain solve %.3e" % (case[:4], e))
    assert n_p[0] == n0[0]
    assert e <= 1e-10
    s.close()


# ---- g. the beam epilogue -----------------------------------------------------------------------------------------------------------
EPI = ("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")


def run_epilogue(s, tau, I, z, sigma=None, beam_norm="crit"):
    B, L = tau.shape
    d_tau, d_I, d_z = dev(tau), dev(I), dev(z)
    out = {k: dfull((B,) if k == "net_toa" else (B, L)) for k in EPI}
    sync()
    p = [out[k].data_ptr() for k in EPI]
    if sigma is None:
        s.epilogue_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), beam_norm, *p)
    else:
        d_sig = dev(sigma)
        s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), d_z.data_ptr(), beam_norm, *p)
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["N32-L24-B3", "N33-L24-B3", "N32-L48-B3-2slabs"])
def test_beam_epilogue(name):
    cols = shape_columns(name)
    sig, I = shape_model(name)
    L = len(cols[0].tau)
    z = S.altitudes(L)
    s, tau, _, _ = handle(cols, phase=False)
    for norm in ("crit", "graphe"):
        got = run_epilogue(s, tau, I, z, sig, norm)
        for b, c in enumerate(cols):
            slabs = [(zn.r0, zn.r1) for zn in c.zones if zn.kind == "mix"]
            ref = S.epilogue_beam(I[b], c.mu, c.tau, sig[b], c.N, c.mu0, c.grd_alb, z_profile=z, slabs=slabs, beam_norm=norm)
            for k in EPI:
                e = _err(np.atleast_1d(got[k][b]), np.atleast_1d(ref[k]))
                assert e <= 1e-10, (k, b, e)
        # on the plane path it is sosrt_epilogue_dev
        plane = np.stack([S.plane_path(c.tau, c.mu0) for c in cols])
        a, b_ = run_epilogue(s, tau, I, z, plane, norm), run_epilogue(s, tau, I, z, None, norm)
        for k in EPI:
            assert _err(a[k], b_[k]) <= 1e-12, k
    s.close()


# ---- h. refusals: SOSRT_E_INVALID, a message, outputs untouched -------------------------------------------------------------------
def _refused(call, outputs, s, word=None):
    with pytest.raises(ValueError) as ei:
        call()
    assert str(ei.value), "a refusal carries a message"
    if word:
        assert word in str(ei.value), str(ei.value)
    for o in outputs:
        assert np.all(np.isnan(host(o, s))), "a refused call wrote to an output"


def test_refusals_leave_the_outputs_untouched():
    cols = shape_columns("N32-L24-B3")
    sig, I = shape_model("N32-L24-B3")
    L = 24
    z = S.altitudes(L)
    s, tau, P0a, P0r = handle(cols)
    d_tau, d_z, d_P0a, d_P0r, d_sig, d_I = dev(tau), dev(z), dev(P0a), dev(P0r), dev(sig), dev(I)
    o_sig, o_I1, o_f = dfull((3, L)), dfull((3, L, s.D)), dfull((3, L))
    outs = [o_sig, o_I1, o_f]
    sync()
    slant = lambda **k: s.beam_slant_device(k.get("tau", d_tau.data_ptr()), k.get("z", d_z.data_ptr()), k.get("out", o_sig.data_ptr()),
                                            k.get("R", 6371.0), B=k.get("B"))
    first = lambda **k: s.first_order_beam_device(k.get("tau", d_tau.data_ptr()), k.get("sig", d_sig.data_ptr()),
                                                  k.get("p0a", d_P0a.data_ptr()), k.get("p0r", d_P0r.data_ptr()),
                                                  k.get("out", o_I1.data_ptr()), B=k.get("B"))
    epi = lambda **k: s.epilogue_beam_device(k.get("tau", d_tau.data_ptr()), k.get("I", d_I.data_ptr()), k.get("sig", d_sig.data_ptr()),
                                             k.get("z", 0), "crit", o_f.data_ptr(), d_heating_rate=k.get("hr", 0), B=k.get("B"))
    # earth radius
    for R in (0.0, -6371.0, float("nan"), float("inf")):
        _refused(lambda: slant(R=R), outs, s, "earth_radius")
    # altitudes: not strictly descending, not finite
    for bad in (z[::-1].copy(), np.where(np.arange(L) == 5, z[4], z), np.where(np.arange(L) == 7, np.nan, z), np.where(np.arange(L) == 0, np.inf, z)):
        d_bad = dev(bad)
        sync()
        _refused(lambda: slant(z=d_bad.data_ptr()), outs, s, "z")
    # B outside the current columns
    for B in (0, 4, -1):
        for call in (slant, first, epi):
            _refused(lambda: call(B=B), outs, s, "B=")
    # null pointers
    for k in ("tau", "z", "out"):
        _refused(lambda: slant(**{k: 0}), outs, s, "null")
    for k in ("tau", "sig", "p0a", "p0r", "out"):
        _refused(lambda: first(**{k: 0}), outs, s, "null")
    for k in ("tau", "I", "sig"):
        _refused(lambda: epi(**{k: 0}), outs, s, "null")
    _refused(lambda: epi(hr=o_f.data_ptr()), outs, s, "z_profile")
    # a caller's mu0 outside (0, 1]
    d_mu0 = dev(np.array([0.5, 0.0, 0.3]))
    sync()
    _refused(lambda: s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), o_sig.data_ptr(), 6371.0, d_mu0.data_ptr()), outs, s, "mu0")
    # the README first order
    s.set_first_order("readme")
    for call in (slant, first, epi):
        _refused(call, outs, s, "README")
    s.set_first_order("coded")
    # the stage still works on this handle, and then writes
    slant()
    first()
    epi()
    assert all(np.all(np.isfinite(host(o, s))) for o in outs)
    s.close()
    # single-slab geometry
    s = Solver(L, 32, max_batch=3)
    s.set_grid(O.make_mu(32))
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.4)
    outs = [dfull((3, L)), dfull((3, L, s.D)), dfull((3, L))]
    sync()
    _refused(lambda: s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), outs[0].data_ptr()), outs, s, "slab")
    _refused(lambda: s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), outs[1].data_ptr()),
             outs, s, "slab")
    _refused(lambda: s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), 0, "crit", outs[2].data_ptr()), outs, s, "slab")
    s.close()


# ---- i. the stage leaves the handle as it was -----------------------------------------------------------------------------------------
def test_the_stage_leaves_the_handle_untouched():
    cols = [S.column(O, *S.SOLVE_CASES[0]), S.column(O, *S.SOLVE_CASES[1])]     # (columns the plain solve converges on)
    L = 24
    z = S.altitudes(L)
    s, tau, P0a, P0r = handle(cols)
    f0 = s.first_order(tau, P0a, P0r)
    r0 = s.solve(tau, P0a, P0r)
    assert np.all(r0.status == 0)
    e0 = s.epilogue(z_profile=z)                                # what the resident field and optical depths give
    # the whole stage on buffers of its own, with other optical depths than the resident ones
    tau2 = tau * 1.25
    sig = run_slant(s, tau2, z)
    I1 = run_first_order(s, tau2, sig, P0a, P0r)
    run_epilogue(s, tau2, I1, z, sig)
    e1 = s.epilogue(z_profile=z)                                # the resident field and tau: same bytes
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    r1 = s.solve(tau, P0a, P0r)                                 # the columns and the phase state: the same solve, bit for bit
    assert np.array_equal(r0.I, r1.I) and np.array_equal(r0.n, r1.n)
    assert np.array_equal(s.first_order(tau, P0a, P0r), f0)
    s.close()


# ---- j. the drivers ------------------------------------------------------------------------------------------------------------------
DRV = dict(tauStar_atm=S.T_ATM, alb_atm=1.0, alb_aer=0.97, z0=S.Z0, nb_layers=24, nb_angles=64, atm_phase_fun="rayleigh",
           aer_phase_fun="hg", g_aer=0.7)
DRV_COLS = [(0.3, 0.3), (0.21, 0.3), (0.15, 0.1)]              # (mu0, rho) of S.SOLVE_CASES at N = 64, L = 24


@functools.lru_cache(maxsize=None)
def driver_oracle():
    """[(column, sigma, oracle solution from the model's spherical first order)] of the driver's three columns"""
    out = []
    z = S.altitudes(24)
    for m, r in DRV_COLS:
        c = S.column(O, 64, 24, m, r)
        sg = S.slant_path(c.tau, z, m)
        out.append((c, sg, O.solve_column(c, literal=False, I1=S.first_order_beam(c, sg))))
    return out


def test_driver_on_three_columns(monkeypatch):
    from sosrt import main
    mu0, rho = np.array([c[0] for c in DRV_COLS]), np.array([c[1] for c in DRV_COLS])
    plain = main.SOS_Aer_batch(mu0, S.T_AER, rho, **DRV)
    assert plain.beam_slant is None
    plane = main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="plane", **DRV)
    assert np.array_equal(plane.I, plain.I) and np.array_equal(plane.n, plain.n) and plane.beam_slant is None
    sph = main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="spherical", **DRV)
    assert sph.I.shape == plain.I.shape == (3, 24, 128) and sph.beam_slant.shape == (3, 24) and sph.n.shape == (3,)
    for b, (c, sg, ref) in enumerate(driver_oracle()):
        assert _err(sph.beam_slant[b], sg) <= 1e-12
        e = _err(sph.I[b], ref.I)
        print("driver column mu0=%g: n = %d (oracle %d), field %.3e; the sphere moves it by %.3e" %
              (c.mu0, sph.n[b], ref.n, e, _err(sph.I[b], plain.I[b])))
        assert sph.n[b] == ref.n and sph.status[b] == 0
        assert e <= 1e-10
        assert _err(sph.I[b], plain.I[b]) > 1e-2                # (low sun: the sphere's effect is percent-sized)
    flat = main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="spherical", earth_radius=1e15, **DRV)
    assert np.array_equal(flat.n, plain.n)
    assert _err(flat.I, plain.I) <= 1e-10
    # the cached handle solves a plain batch with its old bits afterwards, also after an error raised in between
    again = main.SOS_Aer_batch(mu0, S.T_AER, rho, **DRV)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n)

    def boom(self, *a, **k):
        raise RuntimeError("raised in between")
    with monkeypatch.context() as mp:
        mp.setattr(Solver, "first_order_beam_device", boom)
        with pytest.raises(RuntimeError, match="in between"):
            main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="spherical", **DRV)
    with pytest.raises(ValueError):                             # (refused by the library: the altitudes do not descend)
        main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="spherical", **dict(DRV, z0=-120.0))
    again = main.SOS_Aer_batch(mu0, S.T_AER, rho, **DRV)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n)
    # the per-order fields of the one-column driver add up to its field
    one = main.SOS_Aer(beam="spherical", mu0=0.21, grd_alb=0.3, tauStar_aer=S.T_AER, **DRV)
    assert one.beam_slant.shape == (24,) and one.I_saved.shape[0] == one.n
    assert _err(one.I, sph.I[1]) <= 1e-12 and _err(one.I_saved.sum(axis=0), one.I) <= 1e-12


def test_other_drivers_take_the_sphere():
    from sosrt import main
    mu0, rho = np.array([0.3, 0.21]), np.array([0.3, 0.3])
    sph = main.SOS_Aer_batch(mu0, S.T_AER, rho, beam="spherical", **DRV)
    d, _ = main.solve_batch_device(mu0, S.T_AER, rho, beam="spherical", **DRV)
    assert np.array_equal(d["I"].cpu().numpy(), sph.I) and np.array_equal(d["beam_slant"].cpu().numpy(), sph.beam_slant)
    # one layer through the zone-table driver: the same field to rounding (its columns are a zone table)
    lay = main.SOS_Aer_layers(mu0, rho, [(25, 17, S.T_AER, 0.97)], beam="spherical", **{k: v for k, v in DRV.items() if k != "alb_aer"})
    assert lay.beam_slant.shape == (2, 24)
    assert _err(lay.I, sph.I) <= 1e-12
    plane = main.SOS_Aer_layers(mu0, rho, [(25, 17, S.T_AER, 0.97)], **{k: v for k, v in DRV.items() if k != "alb_aer"})
    assert plane.beam_slant is None and _err(lay.I, plane.I) > 1e-2


def test_forcing_functions_on_the_sphere():
    from sosrt import forcing
    kw = dict(z0=S.Z0, nb_layers=24, nb_angles=64, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
    mu0, rho, N, L = 0.3, 0.3, 64, 24
    z = S.altitudes(L)

    @functools.lru_cache(maxsize=None)
    def net(t_aer, w_aer):
        mu = O.make_mu(N)
        P0a, Pa = O.phase_rayleigh(N, mu, mu0)
        P0r, Pr = O.phase_hg(N, mu, mu0, 0.7)
        c = O.make_column(mu0, S.Z0, 25, 17, L, S.T_ATM, t_aer, rho, 1.0, w_aer, N, P0a, Pa, P0r, Pr)
        sg = S.slant_path(c.tau, z, mu0)
        r = O.solve_column(c, literal=False, I1=S.first_order_beam(c, sg))
        return float(S.epilogue_beam(r.I, c.mu, c.tau, sg, N, mu0, rho)["net_toa"])

    t_aer, w_aer = np.array([0.3, 0.15]), np.array([0.97, 0.9])
    ref = np.array([net(float(t), float(w)) for t, w in zip(t_aer, w_aer)])
    got = forcing.toa_net_flux(mu0, S.T_ATM, t_aer, rho, 1.0, w_aer, beam="spherical", **kw)
    plane = forcing.toa_net_flux(mu0, S.T_ATM, t_aer, rho, 1.0, w_aer, **kw)
    print("TOA net flux: sphere %s, plane %s, NumPy on the oracle field %s" % (got, plane, ref))
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))
    assert np.all(np.abs(got - plane) > 1e-3)                   # (0.5975 -> 0.5932 at mu0 = 0.3)
    rf = forcing.radiative_forcing(mu0, S.T_ATM, t_aer, rho, 1.0, w_aer, beam="spherical", **kw)
    assert np.max(np.abs(rf - (ref - net(0.0, 1.0)))) <= 1e-10 * np.max(np.abs(ref))
    ca = forcing.critical_albedo(mu0, S.T_ATM, t_aer, rho, 1.0, beam="spherical", **kw)
    want = [O.critical_albedo(lambda w, t=float(t): net(t, float(w)) - net(0.0, 1.0)) for t in t_aer]
    assert np.array_equal(ca, np.array(want))
    flat = forcing.toa_net_flux(mu0, S.T_ATM, t_aer, rho, 1.0, w_aer, beam="spherical", earth_radius=1e15, **kw)
    assert np.max(np.abs(flat - plane)) <= 1e-10 * np.max(np.abs(plane))
