"""Per-level weights in the view stage on the device (csrc/profile_view.hip, csrc/api_profile_view.hip, the shared body of
csrc/api_view.hip) through the C ABI: the three entries against the NumPy models of tests/profile_view_np.py
at the shapes of tests/profile_view_cases.py, their unit-weight bits against the entries they generalise, the node consistency
with the device's own weighted grid solve, rows of weight zero, the handle's state with every refusal, and the drivers against
the chain of Solver calls they stand for.

Bars: 1e-12 of a column's field maximum for an entry against its model (DESIGN section 29's bar for stage kernels; float64 NumPy
itself stays below 1e-13 of it at L = 1024, profile_view_cases.float64_gaps); bit-equality with unit weights; 1e-10, the project's
parity bar, for the constant-weight identity through the driver."""
import numpy as np
import pytest

import driver_cases as DC
import profile_np as P
import profile_view_cases as C
import profile_view_np as PV
import sos_oracle as O
import spherical_np as S
import thermal_np as T
import view_np as VN
from sosrt import _lib
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

RTOL = 1e-10                                                   # the project's parity bar
KERNEL_BAR = 1e-12                                             # an entry against its model, of the column's field maximum
QUADS = {"grid": VN.QUAD_GRID, "linear": VN.QUAD_LINEAR}


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


def handle(cols, phase=False, max_orders=64, B_max=None):
    c0 = cols[0]
    s = Solver(len(c0.tau), c0.N, max_batch=B_max or len(cols), max_orders=max_orders)
    s.set_grid(c0.mu)
    if phase:
        s.set_phase(c0.P_atm, c0.P_aer)
    set_cols(s, cols)
    return s, np.stack([c.tau for c in cols])


def set_weights(s, wa, wr, B=None):
    d_wa, d_wr = None if wa is None else dev(wa), None if wr is None else dev(wr)
    sync()
    s.set_row_weights_device(0 if d_wa is None else d_wa.data_ptr(), 0 if d_wr is None else d_wr.data_ptr(), B=B)
    s.synchronize()


def run_first(s, mv, tau, sig, p0a, p0r, lev, profile=True, B=None):
    """[nset][B][nlev][2V] from p0 rows [nset][B][2V]."""
    nset, B_ = p0a.shape[0], tau.shape[0] if B is None else B
    d = [dev(x) for x in (tau, sig, p0a, p0r)]
    out = dfull((nset, B_, len(lev), 2 * len(mv)))
    sync()
    f = s.view_first_order_profile_device if profile else s.view_first_order_beam_device
    f(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), lev, out.data_ptr(), nset=nset, B=B_)
    return host(out, s)


def run_emission(s, mv, tau, pl, bs, es, lev, profile=True, B=None):
    B_ = tau.shape[0] if B is None else B
    d = [dev(x) for x in (tau, pl, bs)]
    d_es = None if es is None else dev(es)
    out = dfull((B_, len(lev), 2 * len(mv)))
    sync()
    f = s.emission_view_profile_device if profile else s.emission_view_device
    f(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), lev, out.data_ptr(), 0 if d_es is None else d_es.data_ptr(), B=B_)
    return host(out, s)


def run_scattered(s, mv, tau, src, ra, rr, lev, quad, profile=True, B=None):
    B_ = tau.shape[0] if B is None else B
    d = [dev(x) for x in (tau, src, ra, rr)]
    out = dfull((B_, len(lev), 2 * len(mv)))
    sync()
    if profile:
        s.view_radiance_profile_device(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), lev, out.data_ptr(),
                                       quadrature=quad, B=B_)
    else:
        s.view_radiance_device(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), lev, d_scat_out=out.data_ptr(),
                               quadrature=quad, B=B_)
    return host(out, s)


# ---- 1. each new entry against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plane", "slant"])
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_first_order_entry_against_the_model(name, path):
    cols = C.columns(name)
    wa, wr = C.weights(name)
    mv, lev = C.view_mu(name), C.levels(name)
    sig = C.sigma_of(cols, path)
    p0a, p0r = C.p0_rows(name)
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    ref = C.model_first(name, path)
    for nset in (1, C.NSETS):
        got = run_first(s, mv, tau, sig, p0a[:nset], p0r[:nset], lev)
        assert np.all(np.isfinite(got))
        worst = max(C.col_err(got[k], ref[k][:, lev]) for k in range(nset))
        print("gas-view %s %s nset=%d: sosrt_view_first_order_profile_dev vs the model %.3e of the field maximum" % (name, path, nset, worst))
        assert worst <= KERNEL_BAR
    s.close()


@pytest.mark.parametrize("name", list(C.SHAPES))
def test_emission_entry_against_the_model(name):
    """Specular ground; column 1 (mod 5) has rho = 0, the same arithmetic as SOSRT_SURFACE_NONE, which the three-zone geometry has
    no code for (a Lambertian ground is refused: test_state_and_refusals)."""
    cols = C.columns(name)
    wa, wr = C.weights(name)
    mv, lev = C.view_mu(name), C.levels(name)
    pl, bs, es = C.planck_of(name)
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    for explicit in (False, True):
        got = run_emission(s, mv, tau, pl, bs, es if explicit else None, lev)
        assert np.all(np.isfinite(got))
        worst = C.col_err(got, C.model_emission(name, explicit)[:, lev])
        print("gas-view %s emissivity %s: sosrt_emission_view_profile_dev vs the model %.3e of the field maximum"
              % (name, "given" if explicit else "1 - rho", worst))
        assert worst <= KERNEL_BAR
    s.close()


@pytest.mark.parametrize("quad", list(QUADS))
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_scattered_entry_against_the_model(name, quad):
    cols = C.columns(name)
    wa, wr = C.weights(name)
    mv, lev = C.view_mu(name), C.levels(name)
    ra, rr = C.phase_rows(name)
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    got = run_scattered(s, mv, tau, C.source_field(name), ra, rr, lev, quad)
    assert np.all(np.isfinite(got))
    worst = C.col_err(got, C.model_scattered(name, QUADS[quad])[:, lev])
    print("gas-view %s %s: sosrt_view_radiance_profile_dev vs the model %.3e of the field maximum" % (name, quad, worst))
    assert worst <= KERNEL_BAR
    s.close()


# ---- 2. unit weights are bit-equal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_unit_weights_have_the_bits_of_the_unweighted_entries(name):
    cols = C.columns(name)
    mv, lev = C.view_mu(name), C.levels(name)
    p0a, p0r = C.p0_rows(name)
    ra, rr = C.phase_rows(name)
    pl, bs, es = C.planck_of(name)
    src = C.source_field(name)
    ones = np.ones_like(C.weights(name)[0])
    s, tau = handle(cols)
    plain = {}
    for path in ("plane", "slant"):
        plain[path] = run_first(s, mv, tau, C.sigma_of(cols, path), p0a, p0r, lev, profile=False)
    for explicit in (False, True):
        plain[explicit] = run_emission(s, mv, tau, pl, bs, es if explicit else None, lev, profile=False)
    for quad in QUADS:
        plain[quad] = run_scattered(s, mv, tau, src, ra, rr, lev, quad, profile=False)
    set_weights(s, ones, None)                                 # (ones by value, ones by the NULL pointer)
    for path in ("plane", "slant"):
        assert np.array_equal(run_first(s, mv, tau, C.sigma_of(cols, path), p0a, p0r, lev), plain[path]), "first order, %s" % path
    for explicit in (False, True):
        assert np.array_equal(run_emission(s, mv, tau, pl, bs, es if explicit else None, lev), plain[explicit]), "emission"
    for quad in QUADS:
        assert np.array_equal(run_scattered(s, mv, tau, src, ra, rr, lev, quad), plain[quad]), "scattered, %s" % quad
    s.close()


# ---- 3. node consistency on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slabs", [None, S.TWO_SLABS], ids=["L40-N64-B2", "L48-N64-B2-2slabs"])
def test_node_consistency_with_the_weighted_grid_solve(slabs):
    """A weighted solve_device(d_I1=...) from first_order_profile_device, every order stored; then the profile view entries at
    view_np.node_views.  Scattered (GRID, on I - I_last): I - I1 of the device's own field on the lanes rewritten_down /
    untouched_up leave; first term: the grid's profile first order; emission: emission_profile_device at the nodes.  1e-12."""
    torch = _torch()
    L, N = (48 if slabs else 40), 64
    cols = tuple(P.column(O, N, L, p[0], p[1], slabs, "specular", C.G_AER, p[2], p[3]) for p in C.PAR[:2])
    w = [P.random_weights(c, 300 + b) for b, c in enumerate(cols)]
    wa, wr = np.stack([x[0] for x in w]), np.stack([x[1] for x in w])
    B, D = 2, 2 * N
    s, tau = handle(cols, phase=True)
    set_weights(s, wa, wr)
    sig = C.sigma_of(cols, "plane")
    d_tau, d_sig = dev(tau), dev(sig)
    d_P0a, d_P0r = dev(np.stack([c.P0_atm for c in cols])), dev(np.stack([c.P0_aer for c in cols]))
    d_I1, d_I = dfull((B, L, D)), dfull((B, L, D))
    d_sv = torch.zeros((B, 64, L, D), dtype=torch.float64, device=d_tau.device)
    d_n = torch.zeros(B, dtype=torch.int32, device=d_tau.device)
    sync()
    s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr())
    s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_I1=d_I1.data_ptr(),
                   d_I_saved=d_sv.data_ptr(), d_n_orders=d_n.data_ptr())
    I, I1, sv, n = host(d_I, s), host(d_I1, s), host(d_sv, s), host(d_n, s)
    assert np.all(n >= 3) and np.array_equal(sv[:, 0], I1)
    src = np.stack([I[b] - sv[b, n[b] - 1] for b in range(B)])
    mv, lanes = VN.node_views(cols[0].mu, N)
    V, lev = len(mv), np.arange(L, dtype=np.int32)
    # rows at the nodes' cosines are the stored matrices' rows; p0 rows are P0 there
    scat = run_scattered(s, mv, tau, src, cols[0].P_atm[lanes], cols[0].P_aer[lanes], lev, "grid")
    p0a, p0r = np.stack([c.P0_atm[lanes] for c in cols])[None], np.stack([c.P0_aer[lanes] for c in cols])[None]
    first = run_first(s, mv, tau, sig, p0a, p0r, lev)[0]
    pl, bs = np.stack([T.planck_profile(L), 1.2 * T.planck_profile(L)]), np.array([1.0, 1.1])
    d_pl, d_bs, d_I0 = dev(pl), dev(bs), dfull((B, L, D))
    sync()
    s.emission_profile_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr())
    I0 = host(d_I0, s)
    emis = run_emission(s, mv, tau, pl, bs, None, lev)
    for b, c in enumerate(cols):
        ref = (I[b] - I1[b])[:, lanes]
        err = np.abs(scat[b] - ref) / np.max(np.abs(ref))
        # the lanes the model's own comparison leaves: profile_view_np on the oracle's weighted loop from the device's first order
        Im, Im_last, nm = PV.solve_column_last(O, c, wa[b], wr[b], I1[b])
        assert nm == n[b]
        Sm = PV.view_source_profile(c, c.P_atm[lanes], c.P_aer[lanes], Im - Im_last, wa[b], wr[b])
        refm = (Im - I1[b])[:, lanes]
        up = VN.untouched_up(np.abs(VN.transport(c, Sm, mv, VN.QUAD_GRID) - refm) / np.max(np.abs(refm)))
        rew = VN.rewritten_down(c, lanes[:V])
        e_s = max(err[:, :V][~rew].max(), err[:, V:][:, up].max())
        e_f = float(np.max(np.abs(first[b] - I1[b][:, lanes])) / np.max(np.abs(I1[b])))
        e_e = float(np.max(np.abs(emis[b] - I0[b][:, lanes])) / np.max(np.abs(I0[b])))
        print("gas-view node consistency L=%d column %d: scattered %.3e (%d upward lanes), first term %.3e, emission %.3e"
              % (L, b, e_s, up.sum(), e_f, e_e))
        assert up.sum() >= V // 2
        assert e_s <= KERNEL_BAR and e_f <= KERNEL_BAR and e_e <= KERNEL_BAR
    s.close()


# ---- 4. rows of weight zero; a column's bits do not depend on its batch ----------------------------------------------------------
def test_a_row_of_weight_zero_contributes_exactly_nothing():
    """One level, a column whose weights are all 0: the scattered source of every row is +0, so the scattered term and the first
    order are exactly +0 on every lane (the sweeps add and multiply zeros), while its neighbour keeps its values."""
    name = "L40-N32-B5-V3"
    cols = C.columns(name)[:2]
    wa, wr = (x[:2].copy() for x in C.weights(name))
    wa[0], wr[0] = 0.0, 0.0
    mv = C.view_mu(name)
    ra, rr = C.phase_rows(name)
    p0a, p0r = (x[:1, :2] for x in C.p0_rows(name))
    s, tau = handle(cols)
    set_weights(s, wa, wr)
    for lev in ([17], [39], [0]):
        for quad in QUADS:
            got = run_scattered(s, mv, tau, C.source_field(name)[:2], ra, rr, lev, quad)
            assert np.all(got[0] == 0) and not np.any(np.signbit(got[0])), (lev, quad)
            assert lev == [0] or np.all(got[1, :, :len(mv)] > 0)
        got = run_first(s, mv, tau, C.sigma_of(cols, "plane"), p0a, p0r, lev)[0]
        assert np.all(got[0] == 0) and not np.any(np.signbit(got[0]))
    s.close()


def test_a_column_does_not_depend_on_its_batch_or_its_neighbours():
    name = "L40-N32-B5-V3"
    cols = C.columns(name)
    wa, wr = C.weights(name)
    mv, lev = C.view_mu(name), C.levels(name)
    ra, rr = C.phase_rows(name)
    p0a, p0r = C.p0_rows(name)
    pl, bs, es = C.planck_of(name)
    src = C.source_field(name)
    sig = C.sigma_of(cols, "slant")

    def run(s, idx, B=None):
        tau = np.stack([cols[i].tau for i in idx])
        return (run_first(s, mv, tau, sig[idx], p0a[:, idx], p0r[:, idx], lev, B=B),
                run_emission(s, mv, tau, pl[idx], bs[idx], es[idx], lev, B=B),
                run_scattered(s, mv, tau, src[idx], ra, rr, lev, "linear", B=B))

    all5 = [0, 1, 2, 3, 4]
    s, _ = handle(cols)
    set_weights(s, wa, wr)
    full = run(s, all5)
    # B = 2 of the five columns: the first two, bit for bit
    first2 = run(s, [0, 1], B=2)
    assert np.array_equal(first2[0], full[0][:, :2]) and all(np.array_equal(a, f[:2]) for a, f in zip(first2[1:], full[1:]))
    # other weights on the neighbours
    wa2, wr2 = wa.copy(), wr.copy()
    wa2[[0, 1, 3, 4]], wr2[[0, 1, 3, 4]] = 0.5, 0.9
    set_weights(s, wa2, wr2)
    other = run(s, all5)
    assert np.array_equal(other[0][:, 2], full[0][:, 2]) and all(np.array_equal(o[2], f[2]) for o, f in zip(other[1:], full[1:]))
    # the first three weighted, the columns beyond B left at one: as if they had been given ones
    set_weights(s, wa[:3], wr[:3], B=3)
    part = run(s, all5)
    set_weights(s, np.concatenate((wa[:3], np.ones((2, 40)))), np.concatenate((wr[:3], np.ones((2, 40)))))
    whole = run(s, all5)
    assert all(np.array_equal(a, b) for a, b in zip(part, whole))
    assert np.array_equal(part[0][:, :3], full[0][:, :3]) and all(np.array_equal(a[:3], f[:3]) for a, f in zip(part[1:], full[1:]))
    s.close()
    # alone on a handle of its own
    s, _ = handle([cols[2]], B_max=5)
    set_weights(s, wa[2:3], wr[2:3])
    alone = run(s, [2])
    assert np.array_equal(alone[0][:, 0], full[0][:, 2]) and all(np.array_equal(a[0], f[2]) for a, f in zip(alone[1:], full[1:]))
    s.close()


# ---- 5. state ------------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals():
    name = "L40-N32-B5-V3"
    cols = C.columns(name)
    wa, wr = C.weights(name)
    mv, lev = C.view_mu(name), C.levels(name)
    p0a, p0r = (x[:1] for x in C.p0_rows(name))
    ra, rr = C.phase_rows(name)
    pl, bs, _ = C.planck_of(name)
    B, L, V2, nl = 5, 40, 2 * len(mv), len(lev)
    s, tau = handle(cols)
    d_tau, d_sig, d_src = dev(tau), dev(C.sigma_of(cols, "plane")), dev(C.source_field(name))
    d_p0a, d_p0r, d_ra, d_rr, d_pl, d_bs = dev(p0a), dev(p0r), dev(ra), dev(rr), dev(pl), dev(bs)
    out = dfull((B * nl * V2 + 2 * 64,))                       # sentinels before and behind the output
    sync()
    o = out[64:].data_ptr()
    t, sg, sr = d_tau.data_ptr(), d_sig.data_ptr(), d_src.data_ptr()
    first = lambda mv=mv, t=t, sg=sg, a=d_p0a.data_ptr(), r=d_p0r.data_ptr(), lev=lev, o=o, nset=1, B=None: \
        s.view_first_order_profile_device(mv, t, sg, a, r, lev, o, nset=nset, B=B)
    emis = lambda mv=mv, t=t, p=d_pl.data_ptr(), b=d_bs.data_ptr(), lev=lev, o=o, B=None: \
        s.emission_view_profile_device(mv, t, p, b, lev, o, B=B)
    scat = lambda mv=mv, t=t, sr=sr, a=d_ra.data_ptr(), r=d_rr.data_ptr(), lev=lev, o=o, quad="grid", B=None: \
        s.view_radiance_profile_device(mv, t, sr, a, r, lev, o, quadrature=quad, B=B)
    untouched = lambda: np.all(np.isnan(host(out, s)))
    # without weights: SOSRT_E_STATE (SosrtError; a ValueError would be SOSRT_E_INVALID), nothing written
    for call in (first, emis, scat):
        with pytest.raises(_lib.SosrtError, match="no per-level weights"):
            call()
        assert untouched()
    set_weights(s, wa, wr)
    # what the unweighted models refuse, each with nothing written
    for call in (first, emis, scat):
        for bad in (dict(B=0), dict(B=6), dict(mv=[]), dict(mv=np.full(65, 0.5)), dict(mv=[0.5, 0.009]), dict(mv=[1.0001]),
                    dict(mv=[np.nan]), dict(lev=[]), dict(lev=[0, 40]), dict(lev=[-1]), dict(t=0), dict(o=0)):
            with pytest.raises(ValueError):
                call(**bad)
            assert untouched(), (call, bad)
    for bad in (dict(sg=0), dict(a=0), dict(r=0), dict(nset=0)):
        with pytest.raises(ValueError):
            first(**bad)
    for bad in (dict(p=0), dict(b=0)):
        with pytest.raises(ValueError):
            emis(**bad)
    for bad in (dict(sr=0), dict(a=0), dict(r=0)):
        with pytest.raises(ValueError):
            scat(**bad)
    with pytest.raises(ValueError, match="quadrature"):
        _lib.check(_lib.lib().sosrt_view_radiance_profile_dev(s._h, B, len(mv), mv.ctypes.data, t, sr, d_ra.data_ptr(), d_rr.data_ptr(), 7,
                                                              nl, lev.ctypes.data, o))
    assert untouched()
    # after clearing, the guarded unweighted entries work again with the bits of a fresh handle
    set_weights(s, None, None)
    again = (run_first(s, mv, tau, C.sigma_of(cols, "plane"), p0a, p0r, lev, profile=False),
             run_emission(s, mv, tau, pl, bs, None, lev, profile=False),
             run_scattered(s, mv, tau, C.source_field(name), ra, rr, lev, "grid", profile=False))
    s.close()
    s, _ = handle(cols)
    fresh = (run_first(s, mv, tau, C.sigma_of(cols, "plane"), p0a, p0r, lev, profile=False),
             run_emission(s, mv, tau, pl, bs, None, lev, profile=False),
             run_scattered(s, mv, tau, C.source_field(name), ra, rr, lev, "grid", profile=False))
    assert all(np.array_equal(a, f) for a, f in zip(again, fresh))
    s.close()
    # a Lambertian ground
    s, _ = handle(C.columns(name, "lambertian"))
    set_weights(s, wa, wr)
    for call in (first, emis, scat):
        with pytest.raises(ValueError, match="Lambertian"):
            call()
        assert untouched()
    s.close()
    # several aerosol phase sets: the two entries that take phase rows
    c3 = C.columns(name)[:3]
    s = Solver(L, 32, max_batch=3)
    s.set_grid(c3[0].mu)
    s.set_phase_sets(c3[0].P_atm, np.stack([c3[0].P_aer, O.phase_hg(32, c3[0].mu, 0.5, 0.3)[1]]))
    set_cols(s, c3)
    s.set_aerosol_sets(np.array([0, 1, 0], dtype=np.int32))
    set_weights(s, wa[:3], wr[:3])
    for call in (first, scat):
        with pytest.raises(ValueError, match="phase sets"):
            call(B=3)
        assert untouched()
    s.close()
    # the single slab; L = 1025
    s = Solver(L, 32, max_batch=2)
    s.set_grid(cols[0].mu)
    s.set_columns_single_slab([0.5, 0.6], 0.9, 0.3)
    for call in (first, emis, scat):
        with pytest.raises(ValueError, match="single slab"):
            call(B=2)
        assert untouched()
    s.close()
    # L = 1025: one row past the stage's LDS budget, refused before the weights are asked for
    s, _ = handle((P.column(O, 32, 1025, 0.6, 0.3),))
    for call in (first, emis, scat):
        with pytest.raises(ValueError, match="at most 1024"):
            call(B=1)
        assert untouched()
    s.close()


# ---- 6. the drivers --------------------------------------------------------------------------------------------------------------------
GAS = np.concatenate(([0.0], np.cumsum(np.where((np.arange(1, DC.L) >= 4) & (np.arange(1, DC.L) <= 9), 0.01, 0.002))))
GAS3 = GAS[None, :] * np.array([1.0, 0.5, 2.0])[:, None]
VIEW = dict(view_mu=np.array([0.3, 0.9, 1.0]), view_levels=[0, 7, -1])


def hand_chain(mu0, t_aer, rho, gas, quad="grid", t_atm=0.124, alb_atm=1.0, alb_aer=1.0, z=None, thermal=None):
    """What SOS_Aer_batch(gas_tau, view_mu, gas_view=True) stands for, call by call on the cached handle: the columns on the total
    optical depth, the weights, the first order (or the emission) with them, the solve from it, the rows at the lanes, the three
    profile view entries on the resident field; the weights cleared."""
    from sosrt import main
    torch = _torch()
    ns = main._gas_args(gas, len(mu0), DC.L)
    s, tau, P0a, P0r, mu, iu, idn, N = main._prepare_batch(mu0, t_aer, rho, t_atm, alb_atm, alb_aer, 120, 25, 17, DC.L, DC.N, "rayleigh",
                                                           0.0, "hg", 0.7, None, None, None, None, None, None, "specular", 256, 0, gas=ns)
    B = tau.shape[0]
    mv = VIEW["view_mu"]
    lev = [x % DC.L for x in VIEW["view_levels"]]
    sgn = np.concatenate((-mv, mv))
    V2 = len(sgn)
    with main._on_torch_stream(s, 0) as dv:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dv)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dv)
        d_tau, d_w, d_mu0 = up(tau), up(ns.w), up(mu0)
        d_I1, d_I = new(B, DC.L, s.D), new(B, DC.L, s.D)
        d_n, d_st = torch.zeros(B, dtype=torch.int32, device=dv), torch.zeros(B, dtype=torch.int32, device=dv)
        d_first, d_scat = new(B, len(lev), V2), new(B, len(lev), V2)
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
                    d_z, d_sig = up(z), new(B, DC.L)
                    s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), B=B)
                s.first_order_profile_device(d_tau.data_ptr(), d_sig.data_ptr(), p0a, p0r, d_I1.data_ptr(), B=B)
            s.solve_device(d_tau.data_ptr(), p0a, p0r, d_I.data_ptr(), d_I1=d_I1.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
            rows, p0rows = [], []
            for kind, g in (("rayleigh", 0.0), ("hg", 0.7)):
                rw, p0 = new(V2, s.D), new(B, V2)
                torch.cuda.current_stream(dv).synchronize()
                s.phase_rows_device(kind, sgn, rw.data_ptr(), g)
                s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p0.data_ptr(), B, g)
                rows.append(rw); p0rows.append(p0)
            if thermal is not None:
                s.emission_view_profile_device(mv, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), lev, d_first.data_ptr(), B=B)
            else:
                s.view_first_order_profile_device(mv, d_tau.data_ptr(), d_sig.data_ptr(), p0rows[0].data_ptr(), p0rows[1].data_ptr(), lev,
                                                  d_first.data_ptr(), B=B)
            s.view_radiance_profile_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), lev,
                                           d_scat.data_ptr(), quadrature=quad, B=B)
            s.synchronize()
        finally:
            s.set_row_weights_device(0, 0)
        out = {k: v.cpu().numpy() for k, v in dict(I=d_I, n=d_n, first=d_first, scat=d_scat).items()}
    return out


def _same(r, ref):
    assert np.array_equal(r.I, ref["I"]) and np.array_equal(r.n, ref["n"])
    assert np.array_equal(r.I_view_first, ref["first"]) and np.array_equal(r.I_view_scattered, ref["scat"])
    assert np.array_equal(r.I_view, ref["first"] + ref["scat"])
    assert np.array_equal(r.view_mu_signed, np.concatenate((-VIEW["view_mu"], VIEW["view_mu"])))


def test_batch_driver_is_the_hand_chain():
    from sosrt.main import SOS_Aer_batch
    DC.fresh()
    kw = dict(DC.SHAPE, **DC.PHASE, raise_on_error=False)
    before = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, **VIEW, **kw)
    for quad in ("grid", "linear"):
        ref = hand_chain(DC.MU0, DC.T_AER, DC.RHO, GAS3, quad)
        r = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, gas_view=True, view_quadrature=quad, **VIEW, **kw)
        _same(r, ref)
        assert list(r.status) == [0, 0, 0] and np.all(np.isfinite(r.I_view)) and np.all(r.I_view[:, 0, 3:] > 0)
    # I and n of a gas_tau call do not depend on the view stage
    plain = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, **kw)
    assert np.array_equal(plain.I, r.I) and np.array_equal(plain.n, r.n) and plain.I_view is None
    # the sphere: the first term on the slant path of the total optical depth
    z = np.linspace(120, 0, DC.L)
    ref = hand_chain(DC.MU0, DC.T_AER, DC.RHO, GAS3, z=z)
    r = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, gas_tau=GAS3, gas_view=True, beam="spherical", beam_stages=True, **VIEW, **kw)
    _same(r, ref)
    assert r.beam_slant is not None
    # the thermal source: the weighted emission at the lanes
    th = (DC.PLANCK, DC.THERMAL["planck_surface"])
    ref = hand_chain(DC.MU0, DC.GREY_T_AER, DC.RHO, GAS3, t_atm=0.125, alb_atm=0.5, alb_aer=0.8, thermal=th)
    r = SOS_Aer_batch(DC.MU0, DC.GREY_T_AER, DC.RHO, gas_tau=GAS3, gas_view=True, **VIEW, **DC.GREY, **DC.THERMAL, **kw)
    _same(r, ref)
    # a call without gas after the gas-view calls has its old bits
    after = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, **VIEW, **kw)
    for k in ("I", "n", "I_view_first", "I_view_scattered", "I_view"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    DC.fresh()


def test_constant_weight_through_the_driver():
    """gas_tau = tau0 (1 / w - 1) gives w == 0.8: the scaled-albedo columns through the existing unweighted view_mu call.
    Scattered term: 1e-10 (the parity bar).  First term: against the layer-by-layer unweighted entry fed tau / mu0, at 1e-12 --
    the closed form of the unweighted call differs from the layer-by-layer form at the 1e-14 level, which is printed."""
    from sosrt import main
    from sosrt.inputs import tau_profile
    torch = _torch()
    DC.fresh()
    w, L, N = 0.8, 40, 32
    mu0, t_aer, t_atm = np.array([0.6, 0.45]), np.array([0.05, 0.1]), 0.124
    tau0 = np.stack([tau_profile(t_atm, t, 120, 25, 17, L) for t in t_aer])
    kw = dict(nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7, view_mu=[0.05, 0.6, 1.0],
              view_levels=[0, 20, -1])
    got = main.SOS_Aer_batch(mu0, t_aer, 0.3, tauStar_atm=t_atm, alb_atm=1.0, alb_aer=0.9, gas_tau=tau0 * (1 / w - 1), gas_view=True, **kw)
    ref = main.SOS_Aer_batch(mu0, t_aer / w, 0.3, tauStar_atm=t_atm / w, alb_atm=w, alb_aer=0.9 * w, **kw)
    assert list(got.n) == list(ref.n) and list(got.status) == [0, 0]
    e_s = C.col_err(got.I_view_scattered, ref.I_view_scattered)
    e_closed = C.col_err(got.I_view_first, ref.I_view_first)
    # the layer-by-layer unweighted first order on the handle the reference call left (its columns are the scaled ones)
    s = main.get_solver(L, N, 2, 256, 0)
    mv, lev = np.array(kw["view_mu"]), [0, 20, L - 1]
    sgn = np.concatenate((-mv, mv))
    d_tau, d_mu0 = dev(ref.tau), dev(mu0)
    d_sig = dev(ref.tau / mu0[:, None])
    p0 = [dfull((2, 6)), dfull((2, 6))]
    d_first = dfull((2, 3, 6))
    sync()
    s.phase_p0_rows_device("rayleigh", d_mu0.data_ptr(), sgn, p0[0].data_ptr(), 2, 0.0)
    s.phase_p0_rows_device("hg", d_mu0.data_ptr(), sgn, p0[1].data_ptr(), 2, 0.7)
    s.view_first_order_beam_device(mv, d_tau.data_ptr(), d_sig.data_ptr(), p0[0].data_ptr(), p0[1].data_ptr(), lev, d_first.data_ptr(), B=2)
    e_f = C.col_err(got.I_view_first, host(d_first, s))
    print("gas-view constant w = %g through SOS_Aer_batch: scattered %.3e, first term vs the layer-by-layer entry %.3e "
          "(vs the closed form %.3e)" % (w, e_s, e_f, e_closed))
    assert e_s <= RTOL and e_f <= KERNEL_BAR and e_closed <= RTOL
    DC.fresh()


def test_band_depth_at_nadir():
    """The physical figure of DESIGN section 30: TOA I_view at view_mu = 1 with a stepped gas_tau against the gas-free column, on
    the plane beam and at mu0 = 0.21 on the sphere.  Asserted: the band is darker than the continuum by more than a tenth, and
    positive; the figures are printed."""
    from sosrt.main import SOS_Aer_batch
    DC.fresh()
    L, N = 40, 32
    kw = dict(nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7, view_mu=[1.0], view_levels=[0])
    gas = np.concatenate(([0.0], np.cumsum(np.where(np.arange(1, L) >= 30, 0.05, 0.002))))      # 0.56 in all, most of it in the lowest rows
    for mu0, sphere in ((0.6, {}), (0.21, dict(beam="spherical", beam_stages=True))):
        clear = SOS_Aer_batch([mu0], 0.1, 0.3, **sphere, **kw)
        band = SOS_Aer_batch([mu0], 0.1, 0.3, gas_tau=gas, gas_view=True, **sphere, **kw)
        up0, up1 = clear.I_view[0, 0, 1], band.I_view[0, 0, 1]
        print("gas-view band depth at nadir, mu0 = %.2f %s: I_view %.6f without gas, %.6f with (ratio %.4f)"
              % (mu0, "sphere" if sphere else "plane", up0, up1, up1 / up0))
        assert 0 < up1 < 0.9 * up0
    DC.fresh()
