"""Pseudo-spherical beam in the azimuth and view stages on the device (csrc/beam_view.hip, sosrt_view_first_order_beam_dev;
beam='spherical' with beam_stages=True): the new entry against the NumPy model of tests/spherical_view_np.py
(which tests/test_spherical_views_host.py pins to the grid's model), its plane pin against the view stage's closed form, its node
pin against the grid's beam kernel, every refusal, the handle left as it was, the per-mode chain against a direct
azimuth-resolved solve on the sphere's path, and the drivers.  None passes without the symbol and the keyword."""
import functools

import numpy as np
import pytest

import azimuth_direct as AD
import sos_oracle as O
import spherical_np as S
import spherical_view_np as SV
import view_azimuth_np as VA
import view_np as VN
from sosrt import inputs
from sosrt.solver import Solver
from test_gpu_spherical import _err, _torch, dev, dfull, handle, host, run_first_order, solve_dev, sync

pytestmark = pytest.mark.gpu

FN_ATM, FN_AER = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7)


def run_view_beam(s, mu_view, tau, sigma, p0a, p0r, levels, nset=1, B=None):
    """sosrt_view_first_order_beam_dev: p0a, p0r [nset, B, 2V] (or [B, 2V]) -> [nset, B, nlev, 2V], with guard elements around
    the output (checked: untouched)."""
    B = tau.shape[0] if B is None else B
    V2 = 2 * len(mu_view)
    d = [dev(x) for x in (tau, sigma, p0a, p0r)]
    n = nset * B * len(levels) * V2
    buf = dfull((n + 32,))
    sync()
    s.view_first_order_beam_device(mu_view, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), levels,
                                   buf.data_ptr() + 16 * 8, nset=nset, B=B)
    out = host(buf, s)
    assert np.all(np.isnan(out[:16])) and np.all(np.isnan(out[-16:])), "the call wrote outside its output"
    return out[16:-16].reshape(nset, B, len(levels), V2)


# ---- the columns of the kernel tests: per shape, shared by the tests and never changed ---------------------------------------------
# (N, L, B, V, slabs): a column at mu0 = 0.05, one with rho = 0 at mu0 = 0.6, one at mu0 = 0.21; B = 70 cycles through sun angles
SHAPES = {"N32-L24-B3-V1": (32, 24, 3, 1, None), "N33-L24-B3-V5": (33, 24, 3, 5, None), "N32-L48-B3-V5-2slabs": (32, 48, 3, 5, S.TWO_SLABS),
          "N32-L24-B70-V3": (32, 24, 70, 3, None), "N32-L24-B2-V64": (32, 24, 2, 64, None)}
PHI_SETS = [0.3, 2.0]                                          # the azimuths of the sets 1 and 2 (set 0: the azimuth mean)


def view_cosines(V):
    """0.01, 1.0, mu0 = 0.6 exactly and 0.6 -+ 1e-5 (0.6 is the sun of column 1), as many of them as V holds."""
    if V == 1:
        return np.array([0.6])
    if V == 3:
        return np.array([0.01, 0.6, 1.0])
    if V == 5:
        return np.array([0.01, 1.0, 0.6, 0.6 - 1e-5, 0.6 + 1e-5])
    mv = np.linspace(0.01, 1.0, V)
    mv[[7, 20, 21, 22]] = [0.05, 0.6 - 1e-5, 0.6, 0.6 + 1e-5]   # (0.05 is the sun of column 0)
    return mv


def interior_levels(c):
    """Interior rows: the first and last row of every aerosol zone and their neighbours, out of order and one of them twice."""
    L = len(c.tau)
    rows = set()
    for z in c.zones:
        if z.kind == "mix":
            rows |= {z.r0 - 1, z.r0, z.r0 + 1, z.r1 - 1, z.r1, z.r1 + 1}
    rows = sorted(r for r in rows if 0 < r < L - 1)
    return rows[::-1] + [0, L - 1, rows[0]]


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(columns, mu_view, sigma [B, L] on the sphere, p0a, p0r [3, B, 2V], model [3, B, L, 2V])"""
    N, L, B, V, slabs = SHAPES[name]
    base = [(0.05, 0.3), (0.6, 0.0), (0.21, 0.5)]
    par = [base[b] if b < 3 else (0.05 + 0.9 * ((7 * b) % 70) / 70.0, 0.1 * (b % 6)) for b in range(B)]
    cols = tuple(S.column(O, N, L, m, r, slabs) for m, r in par)
    mv = view_cosines(V)
    sgn = VN.signed(mv)
    mu, mu0 = cols[0].mu, np.array([c.mu0 for c in cols])
    z = S.altitudes(L)
    sig = np.stack([S.slant_path(c.tau, z, c.mu0) for c in cols])
    p0 = [np.concatenate((VN.phase_p0_rows(fn, mu, mu0, sgn)[None], VA.p0_exact(fn, mu, mu0, sgn, PHI_SETS))) for fn in (FN_ATM, FN_AER)]
    ref = np.stack([[SV.view_first_order_beam(c, sig[b], p0[0][i, b], p0[1][i, b], mv) for b, c in enumerate(cols)] for i in range(3)])
    for a in (sig, p0[0], p0[1], ref):
        a.setflags(write=False)
    return cols, mv, sig, p0[0], p0[1], ref


# ---- a. the new entry against the model on the sphere's path ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_view_beam_kernel_against_the_model(name):
    cols, mv, sig, p0a, p0r, ref = shape_case(name)
    L, B = len(cols[0].tau), len(cols)
    s, tau, _, _ = handle(cols, phase=False)
    top = np.max(np.abs(ref), axis=(2, 3))                     # the field maximum per (set, column)
    for levels in ([0, L - 1], interior_levels(cols[0])):
        three = run_view_beam(s, mv, tau, sig, p0a, p0r, levels, nset=3)
        assert np.all(np.isfinite(three))
        worst = float(np.max(np.abs(three - ref[:, :, levels]) / top[:, :, None, None]))
        print("%s levels %s: view beam kernel vs model %.3e of the field maximum" % (name, levels, worst))
        assert worst <= 1e-12
        for i in range(3):
            one = run_view_beam(s, mv, tau, sig, p0a[i], p0r[i], levels, nset=1)
            assert np.array_equal(one[0], three[i]), "block %d of nset = 3 is not the nset = 1 call on set %d" % (i, i)
    if B > 2:                                                  # the first columns alone: the same bits
        part = run_view_beam(s, mv, tau[:2], sig[:2], p0a[0, :2], p0r[0, :2], [0, L - 1], B=2)
        assert np.array_equal(part[0], run_view_beam(s, mv, tau, sig, p0a[0], p0r[0], [0, L - 1])[0, :2])
    s.close()


def test_more_levels_than_one_launch_takes():
    """300 levels: two launches (256 per launch, as the view stage chunks them), every row more than once."""
    cols, mv, sig, p0a, p0r, ref = shape_case("N33-L24-B3-V5")
    L = 24
    levels = [(7 * i) % L for i in range(300)]
    s, tau, _, _ = handle(cols, phase=False)
    got = run_view_beam(s, mv, tau, sig, p0a[0], p0r[0], levels)[0]
    all_rows = run_view_beam(s, mv, tau, sig, p0a[0], p0r[0], list(range(L)))[0]
    assert np.array_equal(got, all_rows[:, levels])
    s.close()


# ---- b. the plane pin: on sigma = tau / mu0 it is the view stage's closed form -----------------------------------------------------------------
def run_view_closed_form(s, mu_view, tau, p0a, p0r, levels):
    B, V2 = tau.shape[0], 2 * len(mu_view)
    d_tau, d_a, d_r = dev(tau), dev(p0a), dev(p0r)
    out = dfull((B, len(levels), V2))
    sync()
    s.view_radiance_device(mu_view, d_tau.data_ptr(), 0, 0, 0, levels, d_first_out=out.data_ptr(), d_p0rows_atm=d_a.data_ptr(),
                           d_p0rows_aer=d_r.data_ptr(), quadrature="grid", B=B)
    return host(out, s)


@pytest.mark.parametrize("group", ["N32-L24", "N33-L24", "N32-L48-2slabs"])
def test_plane_path_is_the_view_stage_closed_form(group):
    cases = {"N32-L24": [c for c in S.FIRST_ORDER_CASES if c[:2] == (32, 24) and len(c) == 4],
             "N33-L24": [c for c in S.FIRST_ORDER_CASES if c[0] == 33], "N32-L48-2slabs": [c for c in S.FIRST_ORDER_CASES if len(c) > 4]}[group]
    cols = [S.column(O, *case) for case in cases]
    L = len(cols[0].tau)
    mu0 = np.array([c.mu0 for c in cols])
    far = np.array([0.01, 0.0123, 0.31, 0.5, 0.905, 1.0])     # every lane >= 1e-3 from every mu0 of the group
    assert np.min(np.abs(far[:, None] - mu0[None, :])) >= 1e-3
    near = np.array([mu0[0] - 5e-5, mu0[0] + 9e-5])            # within 1e-4 of column 0's sun: the closed form's limit branch
    mv = np.concatenate((far, near))
    sgn = VN.signed(mv)
    p0a, p0r = (VN.phase_p0_rows(fn, cols[0].mu, mu0, sgn) for fn in (FN_ATM, FN_AER))
    s, tau, _, _ = handle(cols, phase=False)
    levels = list(range(L))
    sig = tau / mu0[:, None]
    got = run_view_beam(s, mv, tau, sig, p0a, p0r, levels)[0]
    coded = run_view_closed_form(s, mv, tau, p0a, p0r, levels)
    for b, c in enumerate(cols):
        near_b = np.abs(sgn) - c.mu0                           # the lanes within 1e-4 of this column's sun
        near_b = np.abs(near_b) < 1e-4
        assert near_b.sum() == (4 if c.mu0 == mu0[0] else 0) and np.all(np.abs(np.abs(sgn[~near_b]) - c.mu0) >= 1e-3)
        top = np.max(np.abs(coded[b]))
        e = float(np.max(np.abs(got[b] - coded[b])[:, ~near_b]) / top)
        print("%s mu0=%g rho=%g: plane path vs the view stage's first order %.3e" % (group, c.mu0, c.grd_alb, e))
        assert e <= 1e-10
        if near_b.any():
            d = float(np.max(np.abs(got[b] - coded[b])[:, near_b]) / top)
            print("    lanes within 1e-4 of mu0: %.3e (the limit branch)" % d)
            assert d < 1e-4
    s.close()


# ---- c. the node pin: at node cosines it is the grid's beam kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["N32-L24-B3", "N33-L24-B3", "N32-L48-B3-2slabs"])
def test_node_cosines_are_the_grid_kernel(name):
    import test_gpu_spherical as TS
    cols = TS.shape_columns(name)
    sig, _ = TS.shape_model(name)
    L = len(cols[0].tau)
    s, tau, P0a, P0r = handle(cols, phase=False)
    grid = run_first_order(s, tau, sig, P0a, P0r)
    mv, idx = VN.node_views(cols[0].mu, cols[0].N)
    assert len(mv) <= 64
    got = run_view_beam(s, mv, tau, sig, P0a[:, idx], P0r[:, idx], list(range(L)))[0]
    for b in range(len(cols)):
        e = _err(got[b], grid[b][:, idx])
        print("%s column %d: view lanes at %d nodes vs sosrt_first_order_beam_dev %.3e" % (name, b, len(mv), e))
        assert e <= 1e-12
    s.close()


# ---- d. refusals: SOSRT_E_INVALID, a message, nothing written ---------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    cols, mv, sig, p0a, p0r, _ = shape_case("N33-L24-B3-V5")
    L, N = 24, 33
    s, tau, _, _ = handle(cols, phase=False)
    d_tau, d_sig, d_a, d_r = dev(tau), dev(sig), dev(p0a), dev(p0r)
    buf = dfull((3 * 3 * 2 * 10 + 32,))
    out = buf.data_ptr() + 16 * 8
    sync()

    def call(**k):
        s.view_first_order_beam_device(k.get("mu", mv), k.get("tau", d_tau.data_ptr()), k.get("sig", d_sig.data_ptr()),
                                       k.get("p0a", d_a.data_ptr()), k.get("p0r", d_r.data_ptr()), k.get("levels", [0, L - 1]),
                                       k.get("out", out), nset=k.get("nset", 3), B=k.get("B"))

    def refused(word, **k):
        with pytest.raises(ValueError) as ei:
            call(**k)
        assert word in str(ei.value), str(ei.value)
        assert np.all(np.isnan(host(buf, s))), "a refused call wrote to the output (%s)" % word

    for B in (0, 4, -1):
        refused("B=", B=B)
    refused("V=", mu=[])
    refused("V=", mu=np.linspace(0.1, 1, 65))
    for bad in ([0.3, np.nan, 0.5, 0.6, 0.7], [0.3, 0.005, 0.5, 0.6, 0.7], [1.5, 0.3, 0.5, 0.6, 0.7], [np.inf, 0.3, 0.5, 0.6, 0.7]):
        refused("mu_view", mu=bad)
    refused("levels", levels=[])
    refused("levels", levels=[0, -1])
    refused("levels", levels=[L, 0])
    for n in (0, -2):
        refused("nset", nset=n)
    for key, word in (("tau", "d_tau"), ("sig", "d_sigma"), ("p0a", "d_p0rows"), ("p0r", "d_p0rows"), ("out", "d_first_out")):
        refused(word, **{key: 0})
    # what beam_check refuses: the README first order
    s.set_first_order("readme")
    refused("README")
    s.set_first_order("coded")
    # Lambertian surfaces, as in the view stage
    args = ([c.idx_up for c in cols], [c.idx_down for c in cols], [c.mu0 for c in cols], [c.grd_alb for c in cols], 1.0, 0.97,
            cols[0].dtau_atm, [c.dtau_aer for c in cols], [c.tauStar_tot for c in cols])
    for surface in ("lambertian", "lambertian_readme"):
        s.set_columns(*args, surface=surface)
        refused("Lambertian")
    s.set_columns(*args)
    # columns off aerosol set 0, a per-zone P0 layout, atmosphere sets
    c0 = cols[0]
    s.set_phase_sets(c0.P_atm, np.stack([c0.P_aer, c0.P_aer]))
    s.set_columns(*args)
    s.set_aerosol_sets([0, 1, 0])
    refused("aerosol")
    s.set_aerosol_sets(np.tile(np.array([0, 1, 0], dtype=np.int32), (3, 1)))
    refused("aerosol")
    s.set_columns(*args)
    s.set_phase(c0.P_atm, c0.P_aer)
    s.set_atm_phase_sets(np.stack([c0.P_atm, c0.P_atm]))
    s.set_atmosphere_sets([0, 0, 1])
    refused("atmosphere")
    s.set_columns(*args)
    # the stage still works on this handle, and then writes its output and nothing else
    call()
    got = host(buf, s)
    assert np.all(np.isnan(got[:16])) and np.all(np.isnan(got[-16:])) and np.all(np.isfinite(got[16:-16]))
    s.close()
    # single-slab geometry
    s = Solver(L, N, max_batch=3)
    s.set_grid(O.make_mu(N))
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.4)
    buf.fill_(float("nan"))
    sync()
    refused("slab")
    s.close()


# ---- e. the stage leaves the handle as it was ------------------------------------------------------------------------------------------------
def test_the_stage_leaves_the_handle_untouched():
    torch = _torch()
    cols = [S.column(O, *S.SOLVE_CASES[0]), S.column(O, *S.SOLVE_CASES[1])]     # (columns the plain solve converges on)
    L = 24
    z = S.altitudes(L)
    s, tau, P0a, P0r = handle(cols)
    f0 = s.first_order(tau, P0a, P0r)
    r0 = s.solve(tau, P0a, P0r)
    assert np.all(r0.status == 0)
    e0 = s.epilogue(z_profile=z)                                # what the resident field and optical depths give
    d_t = dev(np.array([3, 2], dtype=np.int32), np.int32)
    sync()
    s.set_order_targets(d_t.data_ptr())                         # order targets are part of the state
    mv = np.array([0.05, 0.4, 0.77])
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    p0a, p0r = (VN.phase_p0_rows(fn, cols[0].mu, mu0, sgn) for fn in (FN_ATM, FN_AER))
    tau2 = tau * 1.25                                           # other optical depths than the resident ones
    sig = np.stack([S.slant_path(t, z, m) for t, m in zip(tau2, mu0)])
    d_in = [dev(x) for x in (tau2, sig, p0a, p0r)]
    before = [x.clone() for x in d_in]
    out = dfull((2, L, 6))
    sync()
    s.view_first_order_beam_device(mv, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), d_in[3].data_ptr(), list(range(L)),
                                   out.data_ptr())
    assert np.all(np.isfinite(host(out, s)))
    assert all(torch.equal(a, b) for a, b in zip(d_in, before))
    e1 = s.epilogue(z_profile=z)                                # the resident field and tau: same bytes
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    _, n_t, _ = solve_dev(s, dev(tau), dev(P0a), dev(P0r))      # the targets are still set
    assert np.array_equal(n_t, [3, 2])
    s.set_order_targets(None)
    r1 = s.solve(tau, P0a, P0r)                                 # the columns and the phase state: the same solve, bit for bit
    assert np.array_equal(r0.I, r1.I) and np.array_equal(r0.n, r1.n)
    assert np.array_equal(s.first_order(tau, P0a, P0r), f0)
    s.close()


# ---- f. the per-mode chain in the linear regime against the direct solve on the sphere's path --------------------------------------------------
def test_mode_chain_against_the_direct_solve():
    """One three-zone column, N = 32, L = 24, Rayleigh (modes 0..2 are all of it): per mode sosrt_first_order_beam_dev on the
    sphere's sigma fed P0^m, sosrt_solve_dev from it (mode 0 at tol 1e-4 gives n, the modes run n orders), the synthesis -- against
    azimuth_direct.direct_solve whose first order is the model's on the same sigma.  P0 scaled by 1e-6: every search of the
    blend stops at its first test (asserted), so the solve is linear in P0."""
    from test_gpu_azimuth import _solver, _three_zone
    from test_gpu_azimuth_direct import _accumulate
    torch = _torch()
    L, N, M, nq, SCALE = 24, 32, 2, 8, 1e-6
    nphi = 25
    mu0 = np.array([0.6])
    geo, sig = SV.sphere_geometry(0.6, L, N)
    s = _solver(L, N, B=1, max_orders=200)
    try:
        tau, _, _ = _three_zone(s, 1, mu0, L=L, N=N)
        s.set_phase(s.phase_matrix("rayleigh"), s.phase_matrix("rayleigh"))
        d_tau, d_sig = dev(tau), dev(sig[None])
        d_I1, d_I = dfull((1, L, 2 * N)), dfull((1, L, 2 * N))
        d_n = torch.zeros(1, dtype=torch.int32, device=d_tau.device)
        d_st = torch.zeros(1, dtype=torch.int32, device=d_tau.device)

        def solve(P0, targets=None):
            d_p = dev(SCALE * P0)
            sync()
            if targets is not None:
                s.set_order_targets(targets.data_ptr())
            try:
                s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_p.data_ptr(), d_p.data_ptr(), d_I1.data_ptr())
                s.solve_device(d_tau.data_ptr(), d_p.data_ptr(), d_p.data_ptr(), d_I.data_ptr(), tol=1e-4, d_I1=d_I1.data_ptr(),
                               d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
                s.synchronize()
            finally:
                s.set_order_targets(None)
            assert int(d_st.cpu()[0]) == 0
            return d_I.cpu().numpy()[0], int(d_n.cpu()[0])
        I0, n = solve(s.phase_p0("rayleigh", mu0))
        d_t = torch.tensor([n], dtype=torch.int32, device=d_tau.device)
        Pm, P0m = s.phase_modes("rayleigh", 1, M, nphi), s.phase_p0_modes("rayleigh", mu0, 1, M, nphi)
        Im = [I0]
        for m in range(1, M + 1):
            s.set_phase((-1) ** m * Pm[m - 1], (-1) ** m * Pm[m - 1])
            I, nn = solve(P0m[m - 1], d_t)
            assert nn == n
            Im.append(I)
        phi = 2 * np.pi * np.arange(nq) / nq
        got = _accumulate(s, np.stack(Im), phi)
    finally:
        s.close()
    fa = inputs._scalar_phase("rayleigh", 0.0)[0]
    with AD.record_blend() as log:
        _, Iq = AD.direct_solve(geo, fa, fa, nq, n, SCALE)
    assert log and all(log)
    ref = np.moveaxis(Iq, 0, -1)
    e = _err(got, ref)
    print("mode chain on the sphere, n = %d: synthesis vs the direct solve %.3e" % (n, e))
    assert e <= 1e-13


# ---- g. the drivers ------------------------------------------------------------------------------------------------------------------------------
DRV = dict(tauStar_atm=S.T_ATM, alb_atm=1.0, alb_aer=0.97, z0=S.Z0, nb_layers=24, nb_angles=32, atm_phase_fun="rayleigh",
           aer_phase_fun="hg", g_aer=0.7)
# (mu0, rho) at N = 32, L = 24: columns on which the reference's mu -> 0+ search stays on the grid on the plane and on the sphere
DRV_COLS = [(0.6, 0.3), (0.45, 0.3), (0.83, 0.3)]
MU0 = np.array([c[0] for c in DRV_COLS])
RHO = np.array([c[1] for c in DRV_COLS])
SPH = dict(beam="spherical", beam_stages=True)
OFF_GRID = np.array([0.0123, 0.31, 0.905])                     # >= 1e-3 from every mu0 above: no limit branch on the plane side


def batch(**kw):
    from sosrt import main
    return main.SOS_Aer_batch(MU0, S.T_AER, RHO, **dict(DRV, **kw))


@functools.lru_cache(maxsize=None)
def plain_calls():
    """(the plain call, the spherical call without stages): what the stages must leave bit for bit"""
    return batch(), batch(beam="spherical")


def same_solve(r, ref):
    assert np.array_equal(r.I, ref.I) and np.array_equal(r.n, ref.n) and np.array_equal(r.status, ref.status)
    assert (r.beam_slant is None) == (ref.beam_slant is None)
    if ref.beam_slant is not None:
        assert np.array_equal(r.beam_slant, ref.beam_slant)


def handle_still_serves(plain):
    same_solve(batch(), plain)


def test_driver_azimuths(monkeypatch):
    plain, sph0 = plain_calls()
    phi = np.linspace(0.0, np.pi, 5)
    kw = dict(azimuths=phi, n_modes=6, levels=(0, 5, -1))
    sph = batch(**SPH, **kw)
    same_solve(sph, sph0)
    assert sph.I_azimuth.shape == (3, 3, 64, 5) and sph.mode_status.shape == (7, 3) and not sph.mode_status.any()
    assert sph.beam_slant.shape == (3, 24)
    pl = batch(**kw)
    flat = batch(**SPH, earth_radius=1e15, **kw)
    e = _err(flat.I_azimuth, pl.I_azimuth)
    print("azimuths: earth_radius = 1e15 vs the plane call %.3e; the sphere moves I_azimuth by %.3e" % (e, _err(sph.I_azimuth, pl.I_azimuth)))
    assert e <= 1e-10
    assert _err(sph.I_azimuth, pl.I_azimuth) > 1e-4
    # the azimuth mean of the synthesis is mode 0, the spherical field itself
    many = batch(**SPH, azimuths=2 * np.pi * np.arange(16) / 16, n_modes=6, levels=(0, -1))
    assert _err(many.I_azimuth.mean(axis=-1), sph0.I[:, [0, 23]]) <= 1e-12
    with pytest.raises(ValueError, match="azimuths"):
        batch(beam="spherical", **kw)
    handle_still_serves(plain)

    def boom(self, *a, **k):
        raise RuntimeError("raised in between")
    with monkeypatch.context() as mp:
        mp.setattr(Solver, "first_order_beam_device", boom)
        with pytest.raises(RuntimeError, match="in between"):
            batch(**SPH, **kw)
    handle_still_serves(plain)


def test_driver_view_mu(monkeypatch):
    plain, sph0 = plain_calls()
    L, N = 24, 32
    mv_nodes, lanes = VN.node_views(O.make_mu(N), N)
    view_mu = np.concatenate((mv_nodes, OFF_GRID))
    V, Vn = len(view_mu), len(mv_nodes)
    assert np.min(np.abs(view_mu[:, None] - MU0[None, :])) >= 1e-3
    kw = dict(view_mu=view_mu, view_levels=(0, 5, -1))
    sph = batch(**SPH, **kw)
    same_solve(sph, sph0)
    assert sph.I_view.shape == sph.I_view_first.shape == sph.I_view_scattered.shape == (3, 3, 2 * V)
    assert np.array_equal(sph.view_mu_signed, np.concatenate((-view_mu, view_mu)))
    assert np.array_equal(sph.I_view, sph.I_view_first + sph.I_view_scattered) and np.all(np.isfinite(sph.I_view))
    pl = batch(**kw)
    flat = batch(**SPH, earth_radius=1e15, **kw)
    for k in ("I_view_first", "I_view_scattered", "I_view"):
        e = _err(getattr(flat, k), getattr(pl, k))
        print("view_mu %s: earth_radius = 1e15 vs the plane call %.3e" % (k, e))
        assert e <= 1e-10
    # the first term is the model's on the driver's own slant path
    sgn = VN.signed(view_mu)
    z = S.altitudes(L)
    for b, (m, r) in enumerate(DRV_COLS):
        c = S.column(O, N, L, m, r)
        p0a, p0r = (VN.phase_p0_rows(fn, c.mu, [m], sgn)[0] for fn in (FN_ATM, FN_AER))
        ref = SV.view_first_order_beam(c, S.slant_path(c.tau, z, m), p0a, p0r, view_mu)[[0, 5, L - 1]]
        assert _err(sph.I_view_first[b], ref) <= 1e-10
        # at node cosines I_view follows the field as the plane view stage does: to the stopping rule's tol, on the lanes that
        # the grid's mu -> 0 treatments leave alone (tests/test_gpu_view.py)
        sol = O.solve_column(c, literal=False, I1=S.first_order_beam(c, S.slant_path(c.tau, z, m)))
        err_h, rewritten = VN.node_errors(c, sol)
        ok_up = VN.untouched_up(err_h)
        assert ok_up.sum() >= 5
        up, down = lanes[Vn:], lanes[:Vn]
        d_up = np.abs(sph.I_view[b, 0, V:V + Vn] - sph.I[b, 0, up])[ok_up]
        print("column %d TOA-up: max |I_view - I| / I = %.2e" % (b, np.max(d_up / sph.I[b, 0, up][ok_up])))
        assert np.all(d_up <= 1e-4 * sph.I[b, 0, up][ok_up])
        ok_dn = ~rewritten[L - 1]
        d_dn = np.abs(sph.I_view[b, 2, :Vn] - sph.I[b, L - 1, down])[ok_dn]
        assert np.all(d_dn <= 1e-4 * sph.I[b, L - 1, down][ok_dn])
    with pytest.raises(ValueError, match="view_mu"):
        batch(beam="spherical", **kw)
    handle_still_serves(plain)

    def boom(self, *a, **k):
        raise RuntimeError("raised in between")
    with monkeypatch.context() as mp:
        mp.setattr(Solver, "view_first_order_beam_device", boom)
        with pytest.raises(RuntimeError, match="in between"):
            batch(**SPH, **kw)
    handle_still_serves(plain)


@pytest.mark.parametrize("first_order", ["exact", "modes"])
def test_driver_view_azimuths(first_order):
    plain, sph0 = plain_calls()
    view_mu = np.array([0.0123, 0.31, 0.5, 0.905, 1.0])
    phi = np.array([0.0, 0.7, np.pi])
    kw = dict(view_mu=view_mu, view_azimuths=phi, view_first_order=first_order, n_modes=6)
    sph = batch(**SPH, **kw)
    same_solve(sph, sph0)
    mono = batch(**SPH, view_mu=view_mu)
    assert np.array_equal(sph.I_view, mono.I_view) and np.array_equal(sph.I_view_first, mono.I_view_first)
    assert sph.I_view_azimuth.shape == sph.I_view_azimuth_first.shape == sph.I_view_azimuth_scattered.shape == (3, 2, 10, 3)
    assert sph.view_mode_status.shape == (7, 3) and not sph.view_mode_status.any() and np.all(np.isfinite(sph.I_view_azimuth))
    pl = batch(**kw)
    flat = batch(**SPH, earth_radius=1e15, **kw)
    for k in ("I_view_azimuth_first", "I_view_azimuth_scattered", "I_view_azimuth"):
        e = _err(getattr(flat, k), getattr(pl, k))
        print("view_azimuths (%s) %s: earth_radius = 1e15 vs the plane call %.3e; the sphere moves it by %.3e"
              % (first_order, k, e, _err(getattr(sph, k), getattr(pl, k))))
        assert e <= 1e-10
    assert _err(sph.I_view_azimuth, pl.I_view_azimuth) > 1e-4
    with pytest.raises(ValueError, match="view_mu"):
        batch(beam="spherical", **kw)
    handle_still_serves(plain)


def test_driver_view_azimuths_rayleigh_only():
    """A Rayleigh-only column has no mode above 2, so the exact first order is the sum of the modes' (1e-12), and its mean over
    48 uniform azimuths is the mode-0 first order, I_view_first (1e-12)."""
    view_mu = np.array([0.0123, 0.31, 0.6, 0.905, 1.0])
    phi = 2 * np.pi * np.arange(48) / 48
    kw = dict(SPH, aer_phase_fun="rayleigh", view_mu=view_mu, view_azimuths=phi, n_modes=3)
    ex = batch(view_first_order="exact", **kw)
    mo = batch(view_first_order="modes", **kw)
    e = _err(ex.I_view_azimuth_first, mo.I_view_azimuth_first)
    m = _err(ex.I_view_azimuth_first.mean(axis=-1), ex.I_view_first)
    print("Rayleigh only: exact vs modes first order %.3e; azimuth mean vs I_view_first %.3e" % (e, m))
    assert e <= 1e-12
    assert m <= 1e-12
    assert np.array_equal(ex.I_view_azimuth_scattered, mo.I_view_azimuth_scattered)


def test_the_sphere_moves_the_view_radiance_at_low_sun():
    """mu0 = 0.21 (N = 64, L = 24, a whole-solve column of DESIGN section 17): I_view at TOA on the upward lanes moves by more
    than 1e-3 of its maximum between plane and sphere; the model gives 3.2e-2 for the converged radiance at the nodes and
    2.2e-2 for its first order (tests/test_spherical_views_host.py)."""
    from sosrt import main
    kw = dict(DRV, nb_angles=64, view_mu=np.array([0.05, 0.2, 0.4, 0.6, 0.8, 1.0]), view_levels=(0,))
    pl = main.SOS_Aer_batch(0.21, S.T_AER, 0.3, **kw)
    sph = main.SOS_Aer_batch(0.21, S.T_AER, 0.3, **SPH, **kw)
    up_pl, up_sph = pl.I_view[0, 0, 6:], sph.I_view[0, 0, 6:]
    e = _err(up_sph, up_pl)
    print("mu0 = 0.21: I_view at TOA, upward lanes, moves by %.3e of its maximum" % e)
    assert e > 1e-3
