"""The view-radiance stage on the device (csrc/view.hip, csrc/api_view.hip) through the C ABI: the builders of
phase rows off the grid (csrc/phase.hip), the source contraction, the two sweeps in both quadratures and the closed-form first order, against
the NumPy model of tests/view_np.py (which tests/test_view_host.py pins to the oracle), against the device's own field at the
nodes of the direction grid, and against a known answer."""
import ctypes
import functools

import numpy as np
import pytest

import sos_oracle as O
import view_np as VN
from sosrt import _lib, inputs
from sosrt.solver import Solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu


def _torch():
    return pytest.importorskip("torch")


def dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def dzeros(shape, fill=0.0):
    torch = _torch()
    return torch.full(tuple(shape), fill, dtype=torch.float64, device=torch.device("cuda", 0))


def host(t, s):
    s.synchronize()
    return t.cpu().numpy()


KINDS = [("iso", 0.0), ("rayleigh", 0.0), ("hg", 0.7), ("table", 0.0)]


def fn_of(kind, g):
    return VN.phase_fn(kind, g, table=inputs.fwc_table() if kind == "table" else None)


def build_rows(s, kind, g, sgn, mu0):
    """(rows [V2, 2N], p0rows [B, V2]) from the device builders."""
    if kind == "table":
        s.set_phase_table(*inputs.fwc_table())
    d_rows, d_p0, d_mu0 = dzeros((len(sgn), s.D)), dzeros((len(mu0), len(sgn))), dev(np.asarray(mu0, dtype=np.float64))
    _torch().cuda.synchronize()
    s.phase_rows_device(kind, sgn, d_rows.data_ptr(), g)
    s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, d_p0.data_ptr(), len(mu0), g)
    return d_rows, d_p0


# ---- a. builders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V2", [10, 34])
@pytest.mark.parametrize("N", [32, 33])
def test_builders(N, V2):
    mu = O.make_mu(N)
    mu0 = np.array([0.3, 0.6, 0.95])
    s = Solver(4, N, max_batch=3)
    s.set_grid(mu)
    s.set_phase_table(*inputs.fwc_table())
    nodes = np.unique(np.round(np.linspace(0, 2 * N - 1, V2)).astype(int))
    nodes = np.union1d(nodes, [N - 1, N])[:V2]                       # (both mu = 0 nodes among them)
    rng = np.random.default_rng(5)
    off = np.concatenate(([-1.0, 1.0, 0.01, -0.01], rng.uniform(-1, 1, V2 - 4)))
    for kind, g in KINDS:
        fn = fn_of(kind, g)
        P, P0 = s.phase_matrix(kind, g), s.phase_p0(kind, mu0, g)
        d_rows, d_p0 = build_rows(s, kind, g, mu[nodes], mu0)
        assert_close(host(d_rows, s), P[nodes], 1e-12, "%s rows at nodes" % kind)
        assert_close(host(d_p0, s), P0[:, nodes], 1e-12, "%s P0 rows at nodes" % kind)
        d_rows, d_p0 = build_rows(s, kind, g, off, mu0)
        assert_close(host(d_rows, s), VN.phase_rows(fn, mu, off), 1e-12, "%s rows off the grid" % kind)
        assert_close(host(d_p0, s), VN.phase_p0_rows(fn, mu, mu0, off), 1e-12, "%s P0 rows off the grid" % kind)
    s.close()


# ---- columns of the tests ----------------------------------------------------------------------------------------------------
def three_zone_solver(cols, g, max_orders=64):
    """A handle with the oracle columns `cols` (same shape and phase functions: Rayleigh + HG g) set, and their inputs."""
    c0 = cols[0]
    L, N, B = len(c0.tau), c0.N, len(cols)
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(c0.mu)
    s.set_phase(c0.P_atm, c0.P_aer)
    if c0.zone_table is None:
        s.set_columns([c.idx_up for c in cols], [c.idx_down for c in cols], [c.mu0 for c in cols], [c.grd_alb for c in cols],
                      [c.alb_atm for c in cols], [c.alb_aer for c in cols], [c.dtau_atm for c in cols], [c.dtau_aer for c in cols],
                      [c.tauStar_tot for c in cols])
    else:
        zt = c0.zone_table
        s.set_columns_zones(np.array([[z.r0 for z in c.zone_table] for c in cols]), [int(z.kind == "mix") for z in zt],
                            [c.mu0 for c in cols], [c.grd_alb for c in cols], [c.alb_atm for c in cols], [c.dtau_atm for c in cols],
                            np.array([[z.alb_aer for z in c.zone_table] for c in cols]),
                            np.array([[z.dtau_aer for z in c.zone_table] for c in cols]), [c.tauStar_tot for c in cols])
    tau = np.stack([c.tau for c in cols])
    return s, tau, np.stack([c.P0_atm for c in cols]), np.stack([c.P0_aer for c in cols])


NODE_CASES = {"A": (VN.case_A, [(0.6, 0.3, 0.15), (0.35, 0.1, 0.4), (0.85, 0.6, 0.0)], 0.7),
              "B": (VN.case_B, [(0.6, 0.15, 1.0), (0.4, 0.3, 0.5), (0.9, 0.05, 2.0)], 0.6)}


def run_view(s, mv, d_tau, d_src, rows, p0rows, levels, quadrature="grid", B=None, scat=True, first=False):
    B = s.B if B is None else B
    V2 = 2 * len(mv)
    d_scat = dzeros((B, len(levels), V2), np.nan) if scat else None
    d_first = dzeros((B, len(levels), V2), np.nan) if first else None
    _torch().cuda.synchronize()
    s.view_radiance_device(mv, d_tau.data_ptr(), d_src.data_ptr() if d_src is not None else 0, rows[0].data_ptr() if rows else 0,
                           rows[1].data_ptr() if rows and rows[1] is not None else 0, levels,
                           d_scat_out=d_scat.data_ptr() if scat else 0, d_first_out=d_first.data_ptr() if first else 0,
                           d_p0rows_atm=p0rows[0].data_ptr() if p0rows else 0,
                           d_p0rows_aer=p0rows[1].data_ptr() if p0rows and p0rows[1] is not None else 0, quadrature=quadrature, B=B)
    return (host(d_scat, s) if scat else None), (host(d_first, s) if first else None)


# ---- b. the device's own field at the nodes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_grid_quadrature_reproduces_the_device_field_at_nodes(name):
    case, params, g = NODE_CASES[name]
    cols = [case(*p) for p in params]
    s, tau, P0a, P0r = three_zone_solver(cols, g)
    r = s.solve(tau, P0a, P0r, save_orders=True)
    L, N = tau.shape[1], cols[0].N
    mv, lanes = VN.node_views(cols[0].mu, N)
    V = len(mv)
    src = np.stack([r.I[b] - r.I_saved[b, r.n[b] - 1] for b in range(len(cols))])
    sgn = VN.signed(mv)
    ra, _ = build_rows(s, "rayleigh", 0.0, sgn, [c.mu0 for c in cols])
    rr, _ = build_rows(s, "hg", g, sgn, [c.mu0 for c in cols])
    scat, _ = run_view(s, mv, dev(tau), dev(src), (ra, rr), None, np.arange(L))
    for b, p in enumerate(params):
        # the lanes the host test calls untouched, from the oracle's solve of this column
        c, sol = VN.solved(case, *p)
        assert sol.n == r.n[b]
        err_h, rewritten = VN.node_errors(c, sol)
        keep = np.concatenate((~rewritten, np.broadcast_to(VN.untouched_up(err_h), (L, V))), axis=1)
        ref = (r.I[b] - r.I_saved[b, 0])[:, lanes]
        err = np.where(keep, np.abs(scat[b] - ref), 0.0) / np.max(np.abs(ref))
        print("%s column %d: %d upward lanes, max error %.3e of the field maximum" % (name, b, keep[0, V:].sum(), err.max()))
        assert keep[0, V:].sum() >= 30 and not np.any(np.isnan(scat[b]))
        assert err.max() <= RTOL
    s.close()


def test_grid_quadrature_reproduces_the_device_field_at_nodes_single_slab():
    N, L, g = 64, 30, 0.3
    mu = O.make_mu(N)
    params = [(0.45, 0.9, 0.5), (0.8, 1.0, 0.2), (0.3, 0.7, 1.0)]          # (mu0, albedo, tauStar), black surface
    tau = np.stack([np.linspace(0, p[2], L) for p in params])
    P = O.phase_hg(N, mu, 0.5, g)[1]
    P0 = np.stack([O.phase_hg(N, mu, p[0], g)[0] for p in params])
    s = Solver(L, N, max_batch=3)
    s.set_grid(mu)
    s.set_phase(P, None)
    s.set_columns_single_slab([p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    r = s.solve(tau, P0, None, save_orders=True)
    mv, lanes = VN.node_views(mu, N)
    V = len(mv)
    src = np.stack([r.I[b] - r.I_saved[b, r.n[b] - 1] for b in range(3)])
    rr, _ = build_rows(s, "hg", g, VN.signed(mv), [p[0] for p in params])
    scat, _ = run_view(s, mv, dev(tau), dev(src), (rr, None), None, np.arange(L))
    for b, (mu0, alb, tauStar) in enumerate(params):
        c = VN.single_slab_column(tau[b], mu, N, mu0, alb, tauStar)
        c.P_atm = P
        sol = O.solve_single_slab(tau[b], mu, tauStar, mu0, P0[b], P, alb, N, literal=False)
        assert sol.n == r.n[b]
        err_h, rewritten = VN.node_errors(c, sol, surface=None)
        assert np.where(rewritten, 0.0, err_h[:, :V]).max() < 1e-12          # (the model is pinned on this geometry too)
        keep = np.concatenate((~rewritten, np.broadcast_to(VN.untouched_up(err_h), (L, V))), axis=1)
        ref = (r.I[b] - r.I_saved[b, 0])[:, lanes]
        err = np.where(keep, np.abs(scat[b] - ref), 0.0) / np.max(np.abs(ref))
        print("single slab column %d: %d upward lanes, max error %.3e" % (b, keep[0, V:].sum(), err.max()))
        assert keep[0, V:].sum() >= 30 and err.max() <= RTOL
    s.close()


# ---- c. off the grid, both quadratures, against the model ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def off_grid_columns(N, L, B, g=0.7):
    mu = O.make_mu(N)
    Pa, Pr = O.phase_rayleigh(N, mu, 0.5)[1], O.phase_hg(N, mu, 0.5, g)[1]
    mu0 = np.linspace(0.25, 0.95, B)
    taer = 0.05 + 0.9 * ((np.arange(B) * 7) % 11) / 11
    rho = ((np.arange(B) * 3) % 5) / 5
    fa, fr = VN.phase_fn("rayleigh"), VN.phase_fn("hg", g)
    P0a, P0r = VN.phase_p0_rows(fa, mu, mu0, mu), VN.phase_p0_rows(fr, mu, mu0, mu)
    return tuple(O.make_column(mu0[b], VN.Z0, 25, 17, L, 0.124 + 0.4 * (b % 3), taer[b], rho[b], 0.98, 0.9, N, P0a[b], Pa, P0r[b], Pr)
                 for b in range(B))


@pytest.mark.parametrize("N,B,V", [(33, 3, 5), (33, 3, 17), (32, 70, 1)])
def test_off_grid_against_the_model(N, B, V):
    L, g = 24, 0.7
    cols = off_grid_columns(N, L, B)
    s, tau, _, _ = three_zone_solver(cols, g)
    rng = np.random.default_rng(11)
    # one view cosine inside the |mu - mu0| < 1e-4 limit branch of a column (spec:111,204) and one at the lower end
    mv = np.concatenate(([cols[B // 2].mu0 + 5e-5, 0.01], rng.uniform(0.02, 1.0, V)))[:V] if V > 1 else np.array([cols[B // 2].mu0 - 5e-5])
    src = rng.uniform(0.1, 1.0, (B, L, 2 * N)) * np.exp(-np.linspace(0, 2, L))[None, :, None]
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    ra, pa = build_rows(s, "rayleigh", 0.0, sgn, mu0)
    rr, pr = build_rows(s, "hg", g, sgn, mu0)
    levels = [0, L - 1, 7, cols[0].idx_up, cols[0].idx_down, 7]
    fa, fr = VN.phase_fn("rayleigh"), VN.phase_fn("hg", g)
    mu = cols[0].mu
    Ra, Rr = VN.phase_rows(fa, mu, sgn), VN.phase_rows(fr, mu, sgn)
    P0a, P0r = VN.phase_p0_rows(fa, mu, mu0, sgn), VN.phase_p0_rows(fr, mu, mu0, sgn)
    d_tau, d_src = dev(tau), dev(src)
    want_first = np.stack([VN.first_order(c, P0a[b], P0r[b], mv)[levels] for b, c in enumerate(cols)])
    S = [VN.source(c, Ra, Rr, src[b]) for b, c in enumerate(cols)]
    for quad, qid in (("grid", VN.QUAD_GRID), ("linear", VN.QUAD_LINEAR)):
        scat, first = run_view(s, mv, d_tau, d_src, (ra, rr), (pa, pr), levels, quad, first=True)
        want = np.stack([VN.transport(c, S[b], mv, qid)[levels] for b, c in enumerate(cols)])
        e1 = assert_close(scat, want, RTOL, "%s scattered radiance" % quad)
        e2 = assert_close(first, want_first, RTOL, "first order")
        print("N=%d B=%d V=%d %s: scattered %.2e, first order %.2e" % (N, B, V, quad, e1, e2))
    s.close()


# ---- d. known answer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("three_zone", [True, False], ids=["three_zone", "single_slab"])
def test_linear_quadrature_known_answer(three_zone):
    """Isotropic, conservative, I_src = 1: S = 1 and TOA-up = surface-down = 1 - exp(-tauStar / mu).  The single slab has
    SOSRT_SURFACE_NONE; the three-zone geometry (which the library only takes with a surface) a specular ground of albedo 0."""
    L, N = 24, 16
    mu = O.make_mu(N)
    P0, P = O.phase_isotropic(N, mu)
    mv = np.array([0.011, 0.05, 0.33, 1.0])
    V = len(mv)
    s = Solver(L, N, max_batch=1)
    s.set_grid(mu)
    if three_zone:
        c = O.make_column(0.5, VN.Z0, 25, 17, L, 0.5, 0.5, 0.0, 1.0, 1.0, N, P0, P, P0, P)
        s.set_phase(P, P)
        s.set_columns(c.idx_up, c.idx_down, 0.5, 0.0, 1.0, 1.0, c.dtau_atm, c.dtau_aer, c.tauStar_tot)
        tau = c.tau[None]
    else:
        tau = np.linspace(0, 1.0, L)[None]
        s.set_phase(P, None)
        s.set_columns_single_slab(0.5, 1.0, 1.0)
    rows, _ = build_rows(s, "iso", 0.0, VN.signed(mv), [0.5])
    exact = 1 - np.exp(-tau[0, -1] / mv)
    lin, _ = run_view(s, mv, dev(tau), dev(np.ones((1, L, 2 * N))), (rows, rows if three_zone else None), None, [0, L - 1], "linear")
    print("LINEAR: TOA-up %.2e, surface-down %.2e" % (np.max(np.abs(lin[0, 0, V:] - exact)), np.max(np.abs(lin[0, 1, :V] - exact))))
    assert np.max(np.abs(lin[0, 0, V:] - exact)) < 1e-12 and np.max(np.abs(lin[0, 1, :V] - exact)) < 1e-12
    assert np.all(lin[0, 0, :V] == 0) and np.all(lin[0, 1, V:] == 0)
    if three_zone:
        grid, _ = run_view(s, mv, dev(tau), dev(np.ones((1, L, 2 * N))), (rows, rows), None, [0, L - 1], "grid")
        assert abs(grid[0, 0, V + 2] - exact[2]) > 1e-2                   # (the modes are not swapped)
    s.close()


# ---- e. first order at the nodes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_first_order_at_nodes_matches_the_device_first_order(name):
    case, _, g = NODE_CASES[name]
    N = 64
    # mu0 half-way between two nodes, >= 5e-3 from each: clear of the amplification `first_order_extended` documents
    mu0s = [37.5 / (N - 1), 20.5 / (N - 1), 55.5 / (N - 1)]
    cols = [case(m, 0.3, 0.15) if name == "A" else case(m, 0.15) for m in mu0s]
    s, tau, _, _ = three_zone_solver(cols, g)
    L = tau.shape[1]
    mv, lanes = VN.node_views(cols[0].mu, N)
    P0a, P0r = s.phase_p0("rayleigh", mu0s), s.phase_p0("hg", mu0s, g)
    I1 = s.first_order(tau, P0a, P0r)
    _, pa = build_rows(s, "rayleigh", 0.0, VN.signed(mv), mu0s)
    _, pr = build_rows(s, "hg", g, VN.signed(mv), mu0s)
    _, first = run_view(s, mv, dev(tau), None, None, (pa, pr), np.arange(L), scat=False, first=True)
    e = assert_close(first, I1[:, :, lanes], RTOL, "first order at the nodes")
    print("%s: first order at the nodes %.2e" % (name, e))
    s.close()


def test_first_order_at_nodes_single_slab():
    N, L, g = 32, 30, 0.6
    mu = O.make_mu(N)
    mu0s, alb, tauStar = [14.5 / (N - 1), 25.5 / (N - 1)], [0.9, 1.0], [1.5, 0.3]
    tau = np.stack([np.linspace(0, t, L) for t in tauStar])
    s = Solver(L, N, max_batch=2)
    s.set_grid(mu)
    s.set_phase(O.phase_hg(N, mu, 0.5, g)[1], None)
    s.set_columns_single_slab(mu0s, alb, tauStar)
    mv, lanes = VN.node_views(mu, N)
    I1 = s.first_order(tau, s.phase_p0("hg", mu0s, g))
    _, p0 = build_rows(s, "hg", g, VN.signed(mv), mu0s)
    _, first = run_view(s, mv, dev(tau), None, None, (p0, None), np.arange(L), scat=False, first=True)
    assert_close(first, I1[:, :, lanes], RTOL, "single-slab first order at the nodes")
    want = np.stack([VN.first_order_single_slab(tau[b], tauStar[b], mu0s[b], alb[b], host(p0, s)[b], mv) for b in range(2)])
    assert_close(first, want, RTOL, "single-slab first order against the model")
    s.close()


# ---- f. the field and the handle are left as they were ----------------------------------------------------------------------------------
def test_field_and_handle_untouched():
    torch = _torch()
    cols = [VN.case_A(*p) for p in NODE_CASES["A"][1]]
    s, tau, P0a, P0r = three_zone_solver(cols, 0.7)
    r1 = s.solve(tau, P0a, P0r)
    mv = np.array([0.05, 0.4, 0.77])
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    ra, pa = build_rows(s, "rayleigh", 0.0, sgn, mu0)
    rr, pr = build_rows(s, "hg", 0.7, sgn, mu0)
    d_I, d_tau = dev(r1.I), dev(tau)
    before_I, before_tau = d_I.clone(), d_tau.clone()
    for quad in ("grid", "linear"):
        scat, first = run_view(s, mv, d_tau, d_I, (ra, rr), (pa, pr), [0, len(cols[0].tau) - 1], quad, first=True)
        assert np.all(np.isfinite(scat)) and np.all(np.isfinite(first))
    assert torch.equal(d_I, before_I) and torch.equal(d_tau, before_tau)
    r2 = s.solve(tau, P0a, P0r)
    assert np.array_equal(r1.I, r2.I) and np.array_equal(r1.n, r2.n) and np.array_equal(r1.status, r2.status)
    s.close()


# ---- g. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = 40
    cols = [VN.case_A(*p) for p in NODE_CASES["A"][1]]
    s, tau, P0a, P0r = three_zone_solver(cols, 0.7)
    c0 = cols[0]
    mv = np.array([0.2, 0.9])
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    ra, pa = build_rows(s, "rayleigh", 0.0, sgn, mu0)
    rr, pr = build_rows(s, "hg", 0.7, sgn, mu0)
    d_tau, d_I = dev(tau), dev(np.ones((3, L, 2 * c0.N)))
    d_scat, d_first = dzeros((3, 2, 4), -7.0), dzeros((3, 2, 4), -7.0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(B=3, V=None, mu=mv, quad=0, levels=(0, L - 1), p0=(pa, pr), first=True):
        m = np.ascontiguousarray(mu, dtype=np.float64)
        lev = np.ascontiguousarray(levels, dtype=np.int32)
        _torch().cuda.synchronize()
        return _lib.lib().sosrt_view_radiance_dev(s._h, B, m.size if V is None else V, m.ctypes.data_as(ctypes.c_void_p), vp(d_tau), vp(d_I),
                                                  vp(ra), vp(rr), vp(p0[0]), vp(p0[1]), quad, lev.size, lev.ctypes.data_as(ctypes.c_void_p),
                                                  vp(d_scat), vp(d_first) if first else None)

    def refused(what, **kw):
        rc = call(**kw)
        msg = _lib.lib().sosrt_last_error().decode()
        assert rc == _lib.E_INVALID and msg, "%s: rc %d, message %r" % (what, rc, msg)
        assert np.all(host(d_scat, s) == -7.0) and np.all(host(d_first, s) == -7.0), "%s: an output was written" % what

    assert call() == 0                                                   # (the same call with nothing wrong is served)
    assert not np.any(host(d_scat, s) == -7.0) and not np.any(host(d_first, s) == -7.0)
    d_scat.fill_(-7.0)
    d_first.fill_(-7.0)
    refused("V = 0", V=0)
    refused("V = 65", mu=np.linspace(0.1, 1, 65))
    refused("NaN view cosine", mu=[0.3, np.nan])
    refused("view cosine below 0.01", mu=[0.3, 0.005])
    refused("view cosine above 1", mu=[1.5, 0.3])
    refused("infinite view cosine", mu=[np.inf, 0.3])
    refused("level -1", levels=(0, -1))
    refused("level L", levels=(L, 0))
    refused("B above the current columns", B=4)
    refused("unknown quadrature", quad=2)
    refused("first order without the aerosol's p0rows", p0=(pa, None))
    refused("first order without the atmosphere's p0rows", p0=(None, pr))
    # Lambertian surfaces
    args = ([c.idx_up for c in cols], [c.idx_down for c in cols], mu0, [c.grd_alb for c in cols], 1.0, 0.95, c0.dtau_atm,
            [c.dtau_aer for c in cols], [c.tauStar_tot for c in cols])
    for surface in ("lambertian", "lambertian_readme"):
        s.set_columns(*args, surface=surface)
        refused(surface)
    s.set_columns(*args)
    # the README's first order, with d_first_out only
    s.set_first_order("readme")
    refused("SOSRT_FIRST_ORDER_README")
    assert call(first=False) == 0
    d_scat.fill_(-7.0)
    s.set_first_order("coded")
    # a column off aerosol set 0, a column off atmosphere set 0
    s.set_phase_sets(c0.P_atm, np.stack([c0.P_aer, c0.P_aer]))
    s.set_columns(*args)
    s.set_aerosol_sets([0, 1, 0])
    refused("aerosol sets")
    s.set_columns(*args)
    s.set_phase(c0.P_atm, c0.P_aer)
    s.set_atm_phase_sets(np.stack([c0.P_atm, c0.P_atm]))
    s.set_atmosphere_sets([0, 0, 1])
    refused("atmosphere sets")
    s.set_columns(*args)
    assert call() == 0
    s.close()


# ---- h. the driver -------------------------------------------------------------------------------------------------------------------------
def test_sos_aer_batch_view_mu():
    from sosrt.main import SOS_Aer_batch
    params = NODE_CASES["A"][1][:2]
    L, N, tol = 40, 64, 1e-4
    mu = O.make_mu(N)
    mv_nodes, lanes = VN.node_views(mu, N)
    pick = np.arange(0, len(mv_nodes), 2)                                # every other node ...
    off = np.array([0.0123, 0.31, 0.905])                                # ... and cosines that are not nodes
    view_mu = np.concatenate((mv_nodes[pick], off))
    V, Vn = len(view_mu), len(pick)
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.95, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg",
              g_aer=0.7, tol=tol)
    a = [np.array([p[i] for p in params]) for i in range(3)]
    plain = SOS_Aer_batch(*a, **kw)
    for quad in ("grid", "linear"):
        r = SOS_Aer_batch(*a, view_mu=view_mu, view_quadrature=quad, **kw)
        assert np.array_equal(r.I, plain.I) and np.array_equal(r.n, plain.n) and np.array_equal(r.status, plain.status)
        assert r.view_mu_signed.shape == (2 * V,) and np.array_equal(r.view_mu_signed, np.concatenate((-view_mu, view_mu)))
        assert r.I_view.shape == r.I_view_first.shape == r.I_view_scattered.shape == (2, 2, 2 * V)
        assert np.array_equal(r.I_view, r.I_view_first + r.I_view_scattered) and np.all(np.isfinite(r.I_view))
    r = SOS_Aer_batch(*a, view_mu=view_mu, **kw)                          # the default is 'grid'
    assert plain.I_view is None and plain.view_mu_signed is None
    for b, p in enumerate(params):
        c, sol = VN.solved(VN.case_A, *p)
        err_h, rewritten = VN.node_errors(c, sol)
        ok_up = VN.untouched_up(err_h)[pick]
        assert ok_up.sum() >= 15
        up, down = lanes[len(mv_nodes):][pick], lanes[:len(mv_nodes)][pick]
        # TOA, upward: the view radiance carries the series' next term, which the stopping rule bounds by tol I
        d_up = np.abs(r.I_view[b, 0, V:V + Vn] - r.I[b, 0, up])[ok_up]
        print("column %d TOA-up: max |I_view - I| / I = %.2e" % (b, np.max(d_up / r.I[b, 0, up][ok_up])))
        assert np.all(d_up <= tol * r.I[b, 0, up][ok_up])
        ok_dn = ~rewritten[L - 1][pick]
        d_dn = np.abs(r.I_view[b, 1, :Vn] - r.I[b, L - 1, down])[ok_dn]
        print("column %d surface-down: max |I_view - I| / I = %.2e" % (b, np.max(d_dn / r.I[b, L - 1, down][ok_dn])))
        assert np.all(d_dn <= tol * r.I[b, L - 1, down][ok_dn])
