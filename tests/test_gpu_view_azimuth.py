"""Azimuth-resolved view radiance on the device (csrc/view.hip, csrc/api_view.hip) through the C ABI: the mode
rows and first-order phase values at view lanes (csrc/phase.hip), the view stage on the field of a Fourier mode, the synthesis over the view
lanes and the driver SOS_Aer_batch(..., view_mu=, view_azimuths=), against the NumPy model of tests/view_azimuth_np.py (which
tests/test_view_azimuth_host.py pins to the mode builders and to a direct view radiance) and against the device's own mode
fields at the nodes of the direction grid.

Norms.  Quantities of a mode m >= 1 cross zero, so they are compared as the mode tests of tests/test_gpu_azimuth.py compare
them: the largest difference over the largest reference value (`_close`); the builders against the mode-0 maximum of the same
phase function, as `test_higher_modes_match_numpy` does.  Positive quantities (mode 0, the exact first order) keep
`util.assert_close`."""
import ctypes
import functools
import types

import numpy as np
import pytest

import azimuth_np as A
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import _lib, inputs
from sosrt.solver import Solver
from test_gpu_azimuth import _close, _oracle_fixed
from test_gpu_view import KINDS, NODE_CASES, build_rows, dev, dzeros, fn_of, host, off_grid_columns, run_view, three_zone_solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu


def _torch():
    return pytest.importorskip("torch")


def mode_rows_dev(s, kind, g, sgn, mf, mc, nphi, sign_odd, mu0=None):
    """(rows [mc, V2, 2N], p0rows [mc, B, V2] or None) from the device builders, as torch tensors."""
    d_rows = dzeros((mc, len(sgn), s.D), np.nan)
    _torch().cuda.synchronize()
    s.phase_rows_modes_device(kind, sgn, d_rows.data_ptr(), mf, mc, nphi, g, sign_odd=sign_odd)
    d_p0 = None
    if mu0 is not None:
        d_mu0 = dev(np.asarray(mu0, dtype=np.float64))
        d_p0 = dzeros((mc, len(mu0), len(sgn)), np.nan)
        _torch().cuda.synchronize()
        s.phase_p0_rows_modes_device(kind, d_mu0.data_ptr(), sgn, d_p0.data_ptr(), len(mu0), mf, mc, nphi, g)
        s.synchronize()
    return d_rows, d_p0


def p0_exact_dev(s, kind, g, sgn, mu0, phi):
    d_mu0, d_phi = dev(np.asarray(mu0, dtype=np.float64)), dev(np.asarray(phi, dtype=np.float64))
    d_out = dzeros((len(phi), len(mu0), len(sgn)), np.nan)
    _torch().cuda.synchronize()
    s.phase_p0_rows_azimuth_device(kind, d_mu0.data_ptr(), sgn, d_phi.data_ptr(), len(phi), d_out.data_ptr(), len(mu0), g)
    s.synchronize()
    return d_out


def accumulate_dev(s, vals, phi, B):
    """sosrt_view_azimuth_accumulate_dev over vals [M + 1][B, nlev, V2] in ascending m: [B, nlev, V2, len(phi)]."""
    _, nlev, V2 = vals[0].shape
    d_phi = dev(np.asarray(phi, dtype=np.float64))
    d_out = dzeros((B, nlev, V2, len(phi)), np.nan)
    d_vals = [dev(v) for v in vals]
    _torch().cuda.synchronize()
    for m, d in enumerate(d_vals):
        s.view_azimuth_accumulate_device(m, d.data_ptr(), nlev, V2, d_phi.data_ptr(), len(phi), d_out.data_ptr(), B=B)
    return host(d_out, s)


# ---- a. builders -------------------------------------------------------------------------------------------------------------
MODE_SETS = [(1, 3, 25), (1, 9, 25), (5, 17, 41), (1, 33, 71)]       # 4, 10, 18 and 34 accumulators: every compiled bound


@pytest.mark.parametrize("V2", [10, 34])
@pytest.mark.parametrize("N", [32, 33])
def test_mode_builders(N, V2):
    torch = _torch()
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
        for mf, mc, nphi in MODE_SETS:
            ms = list(range(mf, mf + mc))
            odd = (np.array(ms) & 1).astype(bool)
            what = "%s modes %d..%d on %d nodes" % (kind, mf, mf + mc - 1, nphi)
            # off the grid: the two signs, the model
            r0, p0 = mode_rows_dev(s, kind, g, off, mf, mc, nphi, False, mu0)
            r1, _ = mode_rows_dev(s, kind, g, off, mf, mc, nphi, True)
            r0, r1, p0 = host(r0, s), host(r1, s), host(p0, s)
            assert not np.isnan(r0).any() and not np.isnan(r1).any() and not np.isnan(p0).any(), what
            assert np.array_equal(r1[odd], -1.0 * r0[odd]) and np.array_equal(r1[~odd], r0[~odd]), what + ": sign_odd"
            if kind == "iso":
                assert not np.any(r0) and not np.any(p0), what
                continue
            scale = np.max(np.abs(VN.phase_rows(fn, mu, off)))
            scale0 = np.max(np.abs(VN.phase_p0_rows(fn, mu, mu0, off)))
            e = np.max(np.abs(r0 - VA.mode_rows(fn, mu, off, ms, nphi))) / scale
            e0 = np.max(np.abs(p0 - VA.mode_p0_rows(fn, mu, mu0, off, ms, nphi))) / scale0
            assert e <= 1e-12 and e0 <= 1e-12, "%s: rows %.2e, p0 rows %.2e of the mode-0 maximum" % (what, e, e0)
            if kind == "rayleigh":
                z = np.array(ms) >= 3
                assert not np.any(r0[z]) and not np.any(p0[z]), what + ": modes m >= 3 are exact zeros"
                assert mf >= 3 or np.max(np.abs(r0[~z])) > 1e-3 * scale
            # at node lanes: the rows of sosrt_phase_modes_dev, bit for bit
            rn, pn = mode_rows_dev(s, kind, g, mu[nodes], mf, mc, nphi, False, mu0)
            d_P = dzeros((mc, 2 * N, 2 * N), np.nan)
            torch.cuda.synchronize()
            s.phase_modes_device(kind, d_P.data_ptr(), mf, mc, nphi, g)
            assert np.array_equal(host(rn, s), host(d_P, s)[:, nodes, :]), what + ": rows at nodes"
            P0 = s.phase_p0_modes(kind, mu0, mf, mc, nphi, g)
            e0 = np.max(np.abs(host(pn, s) - P0[:, :, nodes])) / scale0
            assert e0 <= 1e-12, "%s: p0 rows at nodes %.2e" % (what, e0)
    s.close()


@pytest.mark.parametrize("N,V2", [(32, 10), (33, 34)])
def test_exact_p0_builder(N, V2):
    mu = O.make_mu(N)
    mu0 = np.array([0.3, 0.6, 0.95])
    s = Solver(4, N, max_batch=3)
    s.set_grid(mu)
    rng = np.random.default_rng(6)
    off = np.concatenate(([-1.0, 1.0, 0.01, -0.01], rng.uniform(-1, 1, V2 - 4)))
    phi = np.array([0.0, 0.3, np.pi / 2, np.pi, 4.0, -1.0])
    phi48 = 2 * np.pi * np.arange(48) / 48
    for kind, g in KINDS:
        fn = fn_of(kind, g)
        if kind == "table":
            s.set_phase_table(*inputs.fwc_table())
        got = host(p0_exact_dev(s, kind, g, off, mu0, phi), s)
        if kind == "iso":
            assert np.all(got == 1.0)
            continue
        assert_close(got, VA.p0_exact(fn, mu, mu0, off, phi), 1e-12, "%s exact p0" % kind)
        # the mean over the 48 uniform azimuths is the 25-node ring: sosrt_phase_p0_rows_dev
        mean = host(p0_exact_dev(s, kind, g, off, mu0, phi48), s).mean(axis=0)
        _, d_p0 = build_rows(s, kind, g, off, mu0)
        assert_close(mean, host(d_p0, s), 1e-12, "%s mean of the exact p0 over 48 azimuths" % kind)
    s.close()


# ---- b. a node pin per mode: the device's own mode fields ----------------------------------------------------------------------
NPHI_PIN = 25


@functools.lru_cache(maxsize=None)
def oracle_mode(params, m):
    """Case A column `params` solved by the oracle in mode m with the order count of its mode-0 solve: (column with the mode's
    matrices, result with I and I_saved)."""
    import dataclasses
    c, sol = VN.solved(VN.case_A, *params)
    if m == 0:
        return c, sol
    ray, hg = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7)
    cm = dataclasses.replace(c, P_atm=A.solve_modes(ray, c.mu, [m], NPHI_PIN)[0], P_aer=A.solve_modes(hg, c.mu, [m], NPHI_PIN)[0],
                             P0_atm=A.phase_p0_modes(ray, c.mu, c.mu0, [m], NPHI_PIN)[0],
                             P0_aer=A.phase_p0_modes(hg, c.mu, c.mu0, [m], NPHI_PIN)[0])
    In = O.first_order(cm)
    saved, I = [In], In.copy()
    for _ in range(2, sol.n + 1):
        In = O.transport(cm, O.source_function(cm, In), literal=False)
        saved.append(In)
        I = I + In
    return cm, types.SimpleNamespace(I=I, I_saved=np.stack(saved), n=sol.n)


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_grid_quadrature_reproduces_the_device_mode_field_at_nodes(m):
    """DESIGN section 15's case A (Rayleigh + HG g = 0.7, L = 40, N = 64, its three columns), mode m solved on the device with
    the order counts of mode 0 and saved orders: GRID on I^m - I^m_last with the mode's rows at the node cosines reproduces
    I^m - I1^m on the lanes the mu -> 0 treatments left alone in that mode (the oracle's solve of the mode says which)."""
    torch = _torch()
    case, params, g = NODE_CASES["A"]
    cols = [case(*p) for p in params]
    s, tau, P0a, P0r = three_zone_solver(cols, g)
    mu0 = [c.mu0 for c in cols]
    L, N = tau.shape[1], cols[0].N
    r0 = s.solve(tau, P0a, P0r, save_orders=m == 0)
    mv, lanes = VN.node_views(cols[0].mu, N)
    V = len(mv)
    sgn = VN.signed(mv)
    if m == 0:
        r = r0
        ra, _ = build_rows(s, "rayleigh", 0.0, sgn, mu0)
        rr, _ = build_rows(s, "hg", g, sgn, mu0)
    else:
        sg = (-1.0) ** m
        s.set_phase(sg * s.phase_modes("rayleigh", m, 1, NPHI_PIN)[0], sg * s.phase_modes("hg", m, 1, NPHI_PIN, g)[0])
        d_target = dev(np.ascontiguousarray(r0.n, dtype=np.int32))
        torch.cuda.synchronize()
        s.set_order_targets(d_target.data_ptr())
        try:
            r = s.solve(tau, s.phase_p0_modes("rayleigh", mu0, m, 1, NPHI_PIN)[0], s.phase_p0_modes("hg", mu0, m, 1, NPHI_PIN, g)[0],
                        save_orders=True)
        finally:
            s.set_order_targets(None)
        assert np.array_equal(r.n, r0.n)
        ra = mode_rows_dev(s, "rayleigh", 0.0, sgn, m, 1, NPHI_PIN, True)[0][0]
        rr = mode_rows_dev(s, "hg", g, sgn, m, 1, NPHI_PIN, True)[0][0]
    src = np.stack([r.I[b] - r.I_saved[b, r.n[b] - 1] for b in range(len(cols))])
    scat, _ = run_view(s, mv, dev(tau), dev(src), (ra, rr), None, np.arange(L))
    for b, p in enumerate(params):
        cm, sol = oracle_mode(p, m)
        assert sol.n == r.n[b]
        err_h, rewritten = VN.node_errors(cm, sol)
        keep = np.concatenate((~rewritten, np.broadcast_to(VN.untouched_up(err_h), (L, V))), axis=1)
        ref = (r.I[b] - r.I_saved[b, 0])[:, lanes]
        err = np.where(keep, np.abs(scat[b] - ref), 0.0) / np.max(np.abs(ref))
        print("mode %d column %d: %d upward lanes, max error %.3e of the field maximum" % (m, b, keep[0, V:].sum(), err.max()))
        assert keep[0, V:].sum() >= 30 and not np.any(np.isnan(scat[b]))
        assert err.max() <= RTOL
    s.close()


# ---- c. off the grid, both quadratures, against the model ------------------------------------------------------------------------
PHI_OFF = np.array([0.0, 0.3, np.pi / 2, np.pi])


@pytest.mark.parametrize("N,B,V,M", [(33, 3, 5, 3), (33, 3, 17, 9), (32, 70, 1, 2)])
def test_off_grid_against_the_model(N, B, V, M):
    L, g = 24, 0.7
    nphi = max(25, 2 * M + 1)
    cols = off_grid_columns(N, L, B)
    s, tau, _, _ = three_zone_solver(cols, g)
    rng = np.random.default_rng(12)
    # one view cosine inside the |mu - mu0| < 1e-4 limit branch of a column (spec:111,204) and one at the lower end
    mv = np.concatenate(([cols[B // 2].mu0 + 5e-5, 0.01], rng.uniform(0.02, 1.0, V)))[:V] if V > 1 else np.array([cols[B // 2].mu0 - 5e-5])
    # fields of the modes: mode 0 positive, modes m >= 1 of either sign
    src = rng.uniform(0.1, 1.0, (M + 1, B, L, 2 * N)) * np.exp(-np.linspace(0, 2, L))[None, None, :, None]
    src[1:] *= rng.choice([-1.0, 1.0], (M, B, 1, 2 * N)) / np.arange(1, M + 1)[:, None, None, None]
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    mu = cols[0].mu
    ms = list(range(1, M + 1))
    levels = [0, L - 1, 7, cols[0].idx_up, cols[0].idx_down, 7]
    fa, fr = VN.phase_fn("rayleigh"), VN.phase_fn("hg", g)
    # device rows: mode 0 from the stored matrix's builders, modes m >= 1 as (-1)^m rows^m
    ra0, pa0 = build_rows(s, "rayleigh", 0.0, sgn, mu0)
    rr0, pr0 = build_rows(s, "hg", g, sgn, mu0)
    ram, pam = mode_rows_dev(s, "rayleigh", 0.0, sgn, 1, M, nphi, True, mu0)
    rrm, prm = mode_rows_dev(s, "hg", g, sgn, 1, M, nphi, True, mu0)
    rows = [(ra0, rr0)] + [(ram[m - 1], rrm[m - 1]) for m in ms]
    p0rows = [(pa0, pr0)] + [(pam[m - 1], prm[m - 1]) for m in ms]
    # model rows
    Ra = [VN.phase_rows(fa, mu, sgn)] + list(VA.solve_rows(fa, mu, sgn, ms, nphi))
    Rr = [VN.phase_rows(fr, mu, sgn)] + list(VA.solve_rows(fr, mu, sgn, ms, nphi))
    P0a = [VN.phase_p0_rows(fa, mu, mu0, sgn)] + list(VA.mode_p0_rows(fa, mu, mu0, sgn, ms, nphi))
    P0r = [VN.phase_p0_rows(fr, mu, mu0, sgn)] + list(VA.mode_p0_rows(fr, mu, mu0, sgn, ms, nphi))
    d_tau = dev(tau)
    d_src = [dev(src[m]) for m in range(M + 1)]
    want_first = [np.stack([VN.first_order(c, P0a[m][b], P0r[m][b], mv)[levels] for b, c in enumerate(cols)]) for m in range(M + 1)]
    S = [[VN.source(c, Ra[m], Rr[m], src[m, b]) for b, c in enumerate(cols)] for m in range(M + 1)]
    for quad, qid in (("grid", VN.QUAD_GRID), ("linear", VN.QUAD_LINEAR)):
        scat, first, wants, worst = [], [], [], 0.0
        for m in range(M + 1):
            sc, fi = run_view(s, mv, d_tau, d_src[m], rows[m], p0rows[m], levels, quad, first=True)
            want = np.stack([VN.transport(c, S[m][b], mv, qid)[levels] for b, c in enumerate(cols)])
            wants.append(want)
            if m == 0:
                assert_close(sc, want, RTOL, "%s scattered radiance, mode 0" % quad)
                assert_close(fi, want_first[0], RTOL, "first order, mode 0")
            else:
                _close(sc, want, RTOL, "%s scattered radiance, mode %d" % (quad, m))
                _close(fi, want_first[m], RTOL, "first order, mode %d" % m)
                worst = max(worst, np.max(np.abs(sc - want)) / np.max(np.abs(want)), np.max(np.abs(fi - want_first[m])) / np.max(np.abs(want_first[m])))
            scat.append(sc)
            first.append(fi)
        # their synthesis, from the device's own per-mode values
        got_s, got_f = accumulate_dev(s, scat, PHI_OFF, B), accumulate_dev(s, first, PHI_OFF, B)
        _close(got_s, VA.synthesize(np.stack(wants), PHI_OFF), RTOL, "%s synthesis of the scattered part" % quad)
        _close(got_f, VA.synthesize(np.stack(want_first), PHI_OFF), RTOL, "synthesis of the first order")
        print("N=%d B=%d V=%d M=%d %s: modes m >= 1 within %.2e of their maximum" % (N, B, V, M, quad, worst))
    # the exact first order: one closed-form evaluation per azimuth from p(c(lane, mu0, phi)) / Z0
    ea, er = p0_exact_dev(s, "rayleigh", 0.0, sgn, mu0, PHI_OFF), p0_exact_dev(s, "hg", g, sgn, mu0, PHI_OFF)
    Ea, Er = VA.p0_exact(fa, mu, mu0, sgn, PHI_OFF), VA.p0_exact(fr, mu, mu0, sgn, PHI_OFF)
    for i in range(len(PHI_OFF)):
        _, fi = run_view(s, mv, d_tau, None, None, (ea[i], er[i]), levels, scat=False, first=True)
        want = np.stack([VN.first_order(c, Ea[i, b], Er[i, b], mv)[levels] for b, c in enumerate(cols)])
        assert_close(fi, want, RTOL, "exact first order at phi = %g" % PHI_OFF[i])
    s.close()


# ---- d. accumulate ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c with one rounding (exact rational arithmetic, then the correctly rounded conversion)."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_accumulate_writes_then_adds_in_ascending_order():
    """Mode 0 writes (over NaN), modes m >= 1 add 2 v cos(m phi) in the order of the calls.  Two statements.
    (1) The bits: `azimuth_term` compiles to one fused multiply-add, acc <- fma(2 v, cos(m phi), acc) (2 v is exact), so with the
    device's own cos(m phi) -- read back through the kernel itself: mode 0 writes 0, mode m adds 2 * 0.5 * cos -- the output is
    that recurrence evaluated exactly, bit for bit, in ascending m.
    (2) Against the plain host loop `out = out + 2 * v * np.cos(m * phi)` (two roundings per term, the host's cos): within one
    ulp per term, the ulp of the running magnitude at that term (the larger of the sum before, the term and the sum after).
    Which holds, measured on gfx950: (1) holds; the host loop's bits do not (largest difference 8.9e-16 = 0.62 of the bound of
    (2)), and the device's cos(m phi) equals NumPy's on these 42 arguments."""
    B, nlev, V2, M = 3, 5, 14, 6
    phi = np.array([0.0, 0.3, 1.0, np.pi / 2, np.pi, 5.5, -2.0])
    rng = np.random.default_rng(3)
    vals = [rng.uniform(-1, 1, (B, nlev, V2)) for _ in range(M + 1)]
    s = Solver(4, 8, max_batch=B)
    got = accumulate_dev(s, vals, phi, B)
    assert got.shape == (B, nlev, V2, len(phi)) and not np.isnan(got).any()
    # the device's cos(m phi): 0 + fma(2 * 0.5, cos, 0) is cos itself
    zero, half = np.zeros((1, 1, 1)), np.full((1, 1, 1), 0.5)
    cos_d = np.stack([accumulate_dev(s, [zero] * m + [half], phi, 1)[0, 0, 0] for m in range(1, M + 1)])
    cos_h = np.stack([np.cos(m * phi) for m in range(1, M + 1)])
    cos_ulp = np.max(np.abs(cos_d - cos_h) / np.spacing(np.abs(cos_h)))
    # (1) the recurrence with one rounding per term and the device's cos: the bits
    model = np.repeat(vals[0][..., None], len(phi), axis=-1)
    # (2) the host loop and its allowance of one ulp of the running magnitude per term
    want, allow = model.copy(), np.zeros_like(model)
    for m in range(1, M + 1):
        two_v = np.broadcast_to(2 * vals[m][..., None], model.shape)
        model = np.vectorize(_fma)(two_v, np.broadcast_to(cos_d[m - 1], model.shape), model)
        term = 2 * vals[m][..., None] * np.cos(m * phi)
        new = want + term
        allow = allow + np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(term)), np.abs(new)))
        want = new
    d = np.abs(got - want)
    print("accumulate: bits of the fma recurrence %s; bits of the host loop %s, max difference %.2e = %.2f of one ulp per term; "
          "device cos against NumPy %.2f ulp" % (np.array_equal(got, model), np.array_equal(got, want), d.max(), np.max(d / allow), cos_ulp))
    assert np.array_equal(got, model)
    assert np.all(d <= allow)
    # mode 0 alone writes the values themselves, at every azimuth
    assert np.array_equal(accumulate_dev(s, vals[:1], phi, B), np.repeat(vals[0][..., None], len(phi), axis=-1))
    s.close()


# ---- e. the handle, the field and the targets are left as they were ------------------------------------------------------------------
def test_field_handle_and_targets_untouched():
    torch = _torch()
    cols = [VN.case_A(*p) for p in NODE_CASES["A"][1]]
    s, tau, P0a, P0r = three_zone_solver(cols, 0.7)
    mu0 = [c.mu0 for c in cols]
    plain = s.solve(tau, P0a, P0r)
    m, nphi = 1, 25
    s.set_phase(-s.phase_modes("rayleigh", m, 1, nphi)[0], -s.phase_modes("hg", m, 1, nphi, 0.7)[0])
    p0a, p0r = s.phase_p0_modes("rayleigh", mu0, m, 1, nphi)[0], s.phase_p0_modes("hg", mu0, m, 1, nphi, 0.7)[0]
    d_target = dev(np.ascontiguousarray(plain.n, dtype=np.int32))
    torch.cuda.synchronize()
    s.set_order_targets(d_target.data_ptr())
    try:
        r1 = s.solve(tau, p0a, p0r)
        mv = np.array([0.05, 0.4, 0.77])
        sgn = VN.signed(mv)
        d_I, d_tau = dev(r1.I), dev(tau)
        before_I, before_tau, before_t = d_I.clone(), d_tau.clone(), d_target.clone()
        ra, pa = mode_rows_dev(s, "rayleigh", 0.0, sgn, 1, 2, nphi, True, mu0)
        rr, pr = mode_rows_dev(s, "hg", 0.7, sgn, 1, 2, nphi, True, mu0)
        ea = p0_exact_dev(s, "hg", 0.7, sgn, mu0, [0.0, 1.0])
        for quad in ("grid", "linear"):
            scat, first = run_view(s, mv, d_tau, d_I, (ra[0], rr[0]), (pa[0], pr[0]), [0, len(cols[0].tau) - 1], quad, first=True)
            assert np.all(np.isfinite(scat)) and np.all(np.isfinite(first))
            assert np.all(np.isfinite(accumulate_dev(s, [scat, first], [0.0, 2.0], 3)))
        assert np.all(np.isfinite(host(ea, s)))
        assert torch.equal(d_I, before_I) and torch.equal(d_tau, before_tau) and torch.equal(d_target, before_t)
        r2 = s.solve(tau, p0a, p0r)                                    # (the targets are still in force: the same orders, the same bits)
        assert np.array_equal(r1.I, r2.I) and np.array_equal(r1.n, r2.n) and np.array_equal(r2.n, plain.n)
    finally:
        s.set_order_targets(None)
    s.set_phase(cols[0].P_atm, cols[0].P_aer)
    again = s.solve(tau, P0a, P0r)
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n) and np.array_equal(again.status, plain.status)
    s.close()


# ---- f. refusals of the C ABI -----------------------------------------------------------------------------------------------------------
def test_refusals():
    cols = [VN.case_A(*p) for p in NODE_CASES["A"][1]]
    s, tau, P0a, P0r = three_zone_solver(cols, 0.7)
    L_ = _lib.lib()
    D = s.D
    sgn = VN.signed(np.array([0.2, 0.9]))
    d_mu0, d_phi = dev(np.array([c.mu0 for c in cols])), dev(np.array([0.0, 1.0]))
    d_rows, d_p0, d_ex = dzeros((2, 4, D), -7.0), dzeros((2, 4, 4), -7.0), dzeros((2, 4, 4), -7.0)      # (p0 outputs sized for B = 4)
    d_val, d_out = dzeros((4, 2, 4), 1.0), dzeros((4, 2, 4, 2), -7.0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    HG = s._KINDS["hg"]

    def lanes(x):
        a = np.ascontiguousarray(x, dtype=np.float64)
        return a, a.size

    def rows(mu=sgn, V2=None, mf=1, mc=2, nphi=25):
        a, n = lanes(mu)
        return L_.sosrt_phase_rows_modes_dev(s._h, HG, 0.7, mf, mc, nphi, 1, n if V2 is None else V2, a.ctypes.data_as(ctypes.c_void_p), vp(d_rows))

    def p0(mu=sgn, V2=None, mf=1, mc=2, nphi=25, B=3):
        a, n = lanes(mu)
        return L_.sosrt_phase_p0_rows_modes_dev(s._h, B, HG, 0.7, mf, mc, nphi, vp(d_mu0), n if V2 is None else V2,
                                                a.ctypes.data_as(ctypes.c_void_p), vp(d_p0))

    def exact(mu=sgn, V2=None, nout=2, B=3):
        a, n = lanes(mu)
        return L_.sosrt_phase_p0_rows_azimuth_dev(s._h, B, HG, 0.7, vp(d_mu0), n if V2 is None else V2, a.ctypes.data_as(ctypes.c_void_p),
                                                  nout, vp(d_phi), vp(d_ex))

    def acc(B=3, V2=4, nout=2, m=1):
        return L_.sosrt_view_azimuth_accumulate_dev(s._h, B, m, 2, V2, vp(d_val), nout, vp(d_phi), vp(d_out))

    outs = (d_rows, d_p0, d_ex, d_out)

    def refused(what, rc):
        _torch().cuda.synchronize()
        msg = L_.sosrt_last_error().decode()
        assert rc == _lib.E_INVALID and msg, "%s: rc %d, message %r" % (what, rc, msg)
        assert all(np.all(host(t, s) == -7.0) for t in outs), "%s: an output was written" % what

    _torch().cuda.synchronize()
    assert rows() == 0 and p0() == 0 and exact() == 0 and acc(m=0) == 0 and acc(m=1) == 0      # (the same calls with nothing wrong are served)
    assert not np.any(host(d_rows, s) == -7.0) and not np.any(host(d_out[:3], s) == -7.0)
    assert not np.any(host(d_p0, s).reshape(-1)[:2 * 3 * 4] == -7.0) and not np.any(host(d_ex, s).reshape(-1)[:2 * 3 * 4] == -7.0)
    for t in outs:
        t.fill_(-7.0)
    too_many = np.linspace(-1, 1, 2 * _lib.MAX_VIEWS + 1)
    for name, f in (("rows", rows), ("p0 rows", p0), ("exact p0", exact)):
        refused(name + ": V2 = 0", f(V2=0))
        refused(name + ": V2 = 129", f(mu=too_many))
        refused(name + ": lane above 1", f(mu=[0.3, 1.5, -0.3, -1.0]))
        refused(name + ": lane below -1", f(mu=[0.3, 0.5, -0.3, -1.0000001]))
        refused(name + ": NaN lane", f(mu=[0.3, np.nan, -0.3, -1.0]))
        refused(name + ": infinite lane", f(mu=[0.3, np.inf, -0.3, -1.0]))
    for name, f in (("rows", rows), ("p0 rows", p0)):
        refused(name + ": mode 0", f(mf=0))
        refused(name + ": no mode", f(mc=0))
        refused(name + ": mode 24 on 25 nodes", f(mf=23, mc=2))
        refused(name + ": above SOSRT_MAX_MODES", f(mf=60, mc=6, nphi=201))
    refused("p0 rows: B above the current columns", p0(B=4))
    refused("exact p0: B above the current columns", exact(B=4))
    refused("exact p0: nphi_out = 0", exact(nout=0))
    refused("accumulate: B above the current columns", acc(B=4))
    refused("accumulate: nphi_out = 0", acc(nout=0))
    refused("accumulate: V2 = 0", acc(V2=0))
    refused("accumulate: V2 = 129", acc(V2=129))
    refused("accumulate: mode -1", acc(m=-1))
    refused("accumulate: mode 65", acc(m=65))
    assert rows() == 0 and p0() == 0 and exact() == 0 and acc(m=0) == 0
    s.close()


# ---- g. the driver -------------------------------------------------------------------------------------------------------------------------
DRIVER = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.95, nb_layers=24, nb_angles=32, atm_phase_fun="rayleigh", aer_phase_fun="hg",
              g_aer=0.7, max_orders=64)
DRIVER_COLS = (np.array([0.35, 0.6, 0.85]), np.array([0.1, 0.3, 0.6]), np.array([0.4, 0.15, 0.0]))
VIEW = dict(view_mu=[0.2, 0.55, 0.9], view_azimuths=[0, 1.0, np.pi], n_modes=4)


def test_sos_aer_batch_view_azimuths():
    from sosrt.main import SOS_Aer_batch
    L, N, M, nphi = 24, 32, 4, 25
    mu0, taer, rho = DRIVER_COLS
    vmu, phi = np.array(VIEW["view_mu"]), np.array(VIEW["view_azimuths"], dtype=np.float64)
    V = len(vmu)
    sgn = VN.signed(vmu)
    plain = SOS_Aer_batch(mu0, taer, rho, **DRIVER)
    base = SOS_Aer_batch(mu0, taer, rho, view_mu=vmu, **DRIVER)
    r = SOS_Aer_batch(mu0, taer, rho, **VIEW, **DRIVER)
    rm = SOS_Aer_batch(mu0, taer, rho, view_first_order="modes", **VIEW, **DRIVER)
    for x in (r, rm):
        assert x.I_view_azimuth.shape == x.I_view_azimuth_first.shape == x.I_view_azimuth_scattered.shape == (3, 2, 2 * V, len(phi))
        assert x.view_mode_status.shape == (M + 1, 3) and x.view_mode_status.dtype == np.int32 and not x.view_mode_status.any()
        assert np.array_equal(x.I_view_azimuth, x.I_view_azimuth_first + x.I_view_azimuth_scattered) and np.all(np.isfinite(x.I_view_azimuth))
        assert np.array_equal(x.I, plain.I) and np.array_equal(x.n, plain.n) and np.array_equal(x.status, plain.status)
        assert np.array_equal(x.I_view, base.I_view) and np.array_equal(x.I_view_first, base.I_view_first)
        assert np.array_equal(x.I_view_scattered, base.I_view_scattered) and np.array_equal(x.view_mu_signed, base.view_mu_signed)
        assert x.I_azimuth is None and x.mode_status is None
    assert np.array_equal(r.I_view_azimuth_scattered, rm.I_view_azimuth_scattered)
    assert base.I_view_azimuth is None and base.view_mode_status is None
    # against the model: the oracle's mode fields (mode m solved with (-1)^m P^m for the orders of mode 0), the view stage per mode
    mu = inputs.direction_grid(N)
    ray, hg = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7)
    Pa, Pr = A.solve_modes(ray, mu, range(1, M + 1), nphi), A.solve_modes(hg, mu, range(1, M + 1), nphi)
    Ea, Er = VA.p0_exact(ray, mu, mu0, sgn, phi), VA.p0_exact(hg, mu, mu0, sgn, phi)
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    rows = [0, L - 1]
    for b in range(3):
        c = O.make_column(mu0[b], 120, 25, 17, L, 0.124, taer[b], rho[b], 1.0, 0.95, N, Z1, Z2, Z1, Z2)
        P0a, P0r = A.phase_p0_modes(ray, mu, mu0[b], range(1, M + 1), nphi), A.phase_p0_modes(hg, mu, mu0[b], range(1, M + 1), nphi)
        scat = [VA.mode_scattered(c, ray, hg, r.I[b], 0, vmu, VN.QUAD_GRID, nphi)[rows]]
        first = [VN.first_order(c, VA.mode_p0(ray, mu, mu0[b], vmu, 0, nphi), VA.mode_p0(hg, mu, mu0[b], vmu, 0, nphi), vmu)[rows]]
        for m in range(1, M + 1):
            cm = O.make_column(mu0[b], 120, 25, 17, L, 0.124, taer[b], rho[b], 1.0, 0.95, N, P0a[m - 1], Pa[m - 1], P0r[m - 1], Pr[m - 1])
            scat.append(VA.mode_scattered(c, ray, hg, _oracle_fixed(cm, int(r.n[b])), m, vmu, VN.QUAD_GRID, nphi)[rows])
            first.append(VN.first_order(c, VA.mode_p0(ray, mu, mu0[b], vmu, m, nphi), VA.mode_p0(hg, mu, mu0[b], vmu, m, nphi), vmu)[rows])
        want_s, want_fm = VA.synthesize(np.stack(scat), phi), VA.synthesize(np.stack(first), phi)
        want_fe = np.moveaxis(np.stack([VN.first_order(c, Ea[i, b], Er[i, b], vmu)[rows] for i in range(len(phi))]), 0, -1)
        _close(r.I_view_azimuth_scattered[b], want_s, RTOL, "scattered, column %d" % b)
        assert_close(r.I_view_azimuth_first[b], want_fe, RTOL, "exact first order, column %d" % b)
        _close(rm.I_view_azimuth_first[b], want_fm, RTOL, "modes' first order, column %d" % b)
        _close(r.I_view_azimuth[b], want_fe + want_s, RTOL, "I_view_azimuth, column %d" % b)
        print("column %d (n = %d): modes' first order misses the exact one by %.2e of its maximum at M = %d"
              % (b, r.n[b], np.max(np.abs(want_fm - want_fe)) / np.max(np.abs(want_fe)), M))


def test_cached_handle_is_left_as_it_was(monkeypatch):
    from sosrt.main import SOS_Aer_batch
    mu0, taer, rho = DRIVER_COLS
    plain = SOS_Aer_batch(mu0, taer, rho, **DRIVER)
    tight = SOS_Aer_batch(mu0, taer, rho, tol=1e-7, **DRIVER)
    assert (tight.n > plain.n).all()
    SOS_Aer_batch(mu0, taer, rho, **VIEW, **DRIVER)

    def check():
        again = SOS_Aer_batch(mu0, taer, rho, **DRIVER)                   # the phase matrices are back
        assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n) and np.array_equal(again.status, plain.status)
        t2 = SOS_Aer_batch(mu0, taer, rho, tol=1e-7, **DRIVER)            # and the targets cleared: another tolerance runs its own orders
        assert np.array_equal(t2.n, tight.n) and np.array_equal(t2.I, tight.I)
    check()
    # an error raised inside the loop, after the solve of mode 2
    real = Solver.view_azimuth_accumulate_device

    def failing(self, m, *a, **k):
        if m == 2:
            raise RuntimeError("stop in mode 2")
        return real(self, m, *a, **k)
    monkeypatch.setattr(Solver, "view_azimuth_accumulate_device", failing)
    with pytest.raises(RuntimeError, match="stop in mode 2"):
        SOS_Aer_batch(mu0, taer, rho, **VIEW, **DRIVER)
    monkeypatch.undo()
    check()
