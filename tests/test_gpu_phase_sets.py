"""Several aerosol phase matrices in one batch on the device (sosrt_set_phase_sets / sosrt_set_aerosol_sets): per column against
the oracle's column of its own set and against the same columns solved set by set, per aerosol zone against the
superposition helper (tests/phase_sets_helper.py), and the combinations that are refused."""
import numpy as np
import pytest

import sos_oracle as O
from phase_sets_helper import solve_column_zone_sets
from sosrt import _lib, inputs
from sosrt import main as M
from sosrt.main import SOS_Aer_batch, SOS_Aer_layers, device_phase
from sosrt.solver import Solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu

GEOM = dict(z0=120, z_up=25, z_down=17)


def _fresh():
    for s_ in list(M._solvers.values()):
        s_.close()
    M._solvers.clear()


def _three_sets(N, mu0):
    """(P_atm, P0_atm [B, 2N], P_aer [3, 2N, 2N], P0 per set [3, B, 2N]): Rayleigh; HG g = 0.7, HG g = 0.3, the FWC table"""
    mu = O.make_mu(N)
    Pa = O.phase_rayleigh(N, mu, 0.5)[1]
    P0a = np.stack([O.phase_rayleigh(N, mu, m)[0] for m in mu0])
    mt, pt = inputs.fwc_table()
    fns = [lambda m: O.phase_hg(N, mu, m, 0.7), lambda m: O.phase_hg(N, mu, m, 0.3), lambda m: O.phase_table(N, mu, m, mt, pt)]
    Ps = np.stack([f(0.5)[1] for f in fns])
    P0s = np.stack([np.stack([f(m)[0] for m in mu0]) for f in fns])
    return Pa, P0a, Ps, P0s


def _batch(B, seed, nsets=3):
    # (aerosol depths up to 0.25: with the FWC table's forward peak the reference -- and the oracle, and the device -- end a
    # thicker column at L = 60 in the IndexError of spec:404)
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.2, 1.0, B), rng.choice([0.02, 0.05, 0.12, 0.25], B), rng.uniform(0.0, 0.8, B),
            (np.arange(B) % nsets).astype(np.int32))


def _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Pr, P0r, surface="specular", alb_aer=0.95):
    c = O.make_column(mu0[b], GEOM["z0"], GEOM["z_up"], GEOM["z_down"], L, 0.124, taer[b], rho[b], 1.0, alb_aer, N, P0a[b], Pa,
                      P0r, Pr, surface=surface)
    return O.solve_column(c, literal=False)


def test_one_set_through_the_new_entry_points_is_set_phase():
    """S = 1: a C4-like batch of 64 columns (L = 200, N = 128) has the bits of the set_phase path -- field, n, status."""
    L, N, B = 200, 128, 64
    mu0, taer, rho, _ = _batch(B, 4)
    mu = inputs.direction_grid(N)
    _fresh()
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200)
    ref = SOS_Aer_batch(mu0, taer, rho, aer_phase_fun="hg", g_aer=0.7, **kw)
    (s,) = M._solvers.values()
    Pa, Pr = s._P
    P0a, P0r = s.phase_p0("rayleigh", mu0), s.phase_p0("hg", mu0, 0.7)
    plan_before = s.plan_launch(B, B)
    got = SOS_Aer_batch(mu0, taer, rho, P_atm=Pa, P0_atm=P0a, P_aer=Pr[None], P0_aer=P0r, aer_set=np.zeros(B, dtype=np.int32), **kw)
    assert s.phase_sets_info()["sets"] == 1 and s.plan_launch(B, B) == plan_before
    assert np.array_equal(got.I, ref.I) and np.array_equal(got.n, ref.n) and np.array_equal(got.status, ref.status)
    _fresh()


@pytest.mark.parametrize("knobs", ["default", "staged", "dense"])
def test_mixed_batch_against_the_oracle_and_against_set_by_set(knobs, monkeypatch):
    """Three sets interleaved over 60 columns (two column groups of 30) whose order counts differ.  At this size the default
    plan gives a group of 30 the register tile (16 rows) for every order; SOSRT_GEMM_REGS=0 gives it the staged 32-row
    live-column tiles, and SOSRT_GEMM_SMALL=8 on top of that starts it on the dense tiling and goes over to the 64-row
    live-column tiles -- three runs, so that every tiling reads the set of a column; asserted through plan_launch.  Every column against the oracle's column of its own set at RTOL with the same n; bit for bit the columns
    solved set by set through set_phase (both runs take the single pass); a permutation of the columns permutes the results."""
    L, N, B = 60, 64, 60
    if knobs != "default":
        monkeypatch.setenv("SOSRT_GEMM_REGS", "0")
    if knobs == "dense":
        monkeypatch.setenv("SOSRT_GEMM_SMALL", "8")
    mu0, taer, rho, sets = _batch(B, 7)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa, **GEOM)
    _fresh()
    mixed = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P_aer=Ps, P0_aer=P0r, aer_set=sets, **kw)
    (s,) = M._solvers.values()
    gemms = {s.plan_launch(B, live)["gemm"] for live in (30, 20, 10, 2, 1)}
    if knobs == "dense":
        assert s.plan_launch(B, 30)["gemm"] == _lib.PLAN_GEMM_DENSE and _lib.PLAN_GEMM_LIVE64 in gemms
    elif knobs == "staged":
        assert gemms <= {_lib.PLAN_GEMM_LIVE32, _lib.PLAN_GEMM_LIVE32_DEEP}
    else:
        assert gemms == {_lib.PLAN_GEMM_LIVE16_REGS}
    assert (mixed.status == 0).all() and mixed.n.max() > mixed.n.min()
    for b in range(B):
        ref = _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Ps[sets[b]], P0r[b])
        assert mixed.n[b] == ref.n, b
        assert_close(mixed.I[b], ref.I, RTOL, "column %d (set %d)" % (b, sets[b]))
    perm = np.random.default_rng(1).permutation(B)
    p = SOS_Aer_batch(mu0[perm], taer[perm], rho[perm], P0_atm=P0a[perm], P_aer=Ps, P0_aer=P0r[perm], aer_set=sets[perm], **kw)
    info = s.phase_sets_info()
    assert info["sets"] == 3 and info["single_pass"]
    assert np.array_equal(p.I, mixed.I[perm]) and np.array_equal(p.n, mixed.n[perm])
    for k in range(3):
        c = np.flatnonzero(sets == k)
        one = SOS_Aer_batch(mu0[c], taer[c], rho[c], P0_atm=P0a[c], P_aer=Ps[k], P0_aer=P0r[c], **kw)
        assert s.phase_sets_info()["single_pass"]
        assert np.array_equal(one.n, mixed.n[c]), k
        assert np.array_equal(one.I, mixed.I[c]), k
    _fresh()


def test_named_aerosols_are_built_on_the_device():
    """aer_phase_fun as a list of names: the columns of every aerosol have the bits of a batch of that aerosol alone."""
    L, N, B = 60, 64, 12
    mu0, taer, rho, sets = _batch(B, 11)
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, **GEOM)
    _fresh()
    mixed = SOS_Aer_batch(mu0, taer, rho, aer_phase_fun=["hg", "hg", "fwc"], g_aer=[0.7, 0.3, 0.0], aer_set=sets, **kw)
    for k, (name, g) in enumerate((("hg", 0.7), ("hg", 0.3), ("fwc", 0.0))):
        c = np.flatnonzero(sets == k)
        one = SOS_Aer_batch(mu0[c], taer[c], rho[c], aer_phase_fun=name, g_aer=g, **kw)
        assert np.array_equal(one.I, mixed.I[c]) and np.array_equal(one.n, mixed.n[c]), name
    _fresh()


def test_more_groups_than_the_single_set_cache_keep_the_single_pass():
    """70 distinct aerosol depths x 2 sets: 70 groups, more than the 32 a batch on one set may cache -- with sets in use the
    cache grows (128 groups at this size) and the slab rows keep the single pass; a sample of columns against the oracle."""
    L, N, B = 60, 64, 70
    rng = np.random.default_rng(5)
    mu0, rho = rng.uniform(0.3, 1.0, B), rng.uniform(0.0, 0.5, B)
    taer = 0.05 + 0.01 * np.arange(B)
    sets = (np.arange(B) % 2).astype(np.int32)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa, **GEOM)
    _fresh()
    r = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P_aer=Ps[:2], P0_aer=P0r, aer_set=sets, **kw)
    (s,) = M._solvers.values()
    assert s.phase_sets_info()["group_cap"] == 128
    for b in (0, 1, 34, 35, 69):
        ref = _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Ps[sets[b]], P0r[b])
        assert r.n[b] == ref.n
        assert_close(r.I[b], ref.I, RTOL, "column %d" % b)
    # the groups of that batch (the driver has put the cached handle's columns back on set 0)
    s.set_aerosol_sets(sets)
    info = s.phase_sets_info()
    assert info["groups"] == 70 and info["single_pass"]
    _fresh()


@pytest.mark.parametrize("knobs", ["default", "staged", "dense"])
def test_two_pass_fallback_with_sets(knobs, monkeypatch):
    """More groups than the combined-matrix cache holds, so the slab rows take two passes (W_atm, then the W_aer of the tile's
    or the column's set) -- reported by phase_sets_info, otherwise this test has not tested it.  140 distinct aerosol depths x
    2 sets = 140 groups against a cache of 128 (two column groups of 70: by default the register tile; SOSRT_GEMM_REGS=0: the
    staged live-column tiles; SOSRT_GEMM_SMALL=8 on top: the dense tiling first), and a batch of 2 columns on 2 sets with the
    cache bounded to one matrix (SOSRT_MIX_GROUPS=1).  Every column against the oracle at RTOL.  (Two passes sum a slab row in
    another order than the single pass: no bit comparison with set-by-set runs here.)"""
    L, N, B = 60, 64, 140
    if knobs != "default":
        monkeypatch.setenv("SOSRT_GEMM_REGS", "0")
    if knobs == "dense":
        monkeypatch.setenv("SOSRT_GEMM_SMALL", "8")
    rng = np.random.default_rng(6)
    mu0, rho = rng.uniform(0.3, 1.0, B), rng.uniform(0.0, 0.5, B)
    taer = 0.05 + 0.005 * np.arange(B)
    sets = (np.arange(B) % 2).astype(np.int32)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa, **GEOM)
    _fresh()
    r = SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P_aer=Ps[:2], P0_aer=P0r, aer_set=sets, **kw)
    (s,) = M._solvers.values()
    if knobs == "dense":
        assert s.plan_launch(B, 70)["gemm"] == _lib.PLAN_GEMM_DENSE
    s.set_aerosol_sets(sets)                 # (the driver has put the cached handle's columns back on set 0)
    info = s.phase_sets_info()
    assert info["sets"] == 2 and info["groups"] == 0 and not info["single_pass"] and info["group_cap"] == 128
    assert (r.status == 0).all() and r.n.max() > r.n.min()
    for b in range(B):
        ref = _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Ps[sets[b]], P0r[b])
        assert r.n[b] == ref.n, b
        assert_close(r.I[b], ref.I, RTOL, "column %d (set %d)" % (b, sets[b]))
    # a batch of 2
    monkeypatch.setenv("SOSRT_MIX_GROUPS", "1")
    _fresh()
    r2 = SOS_Aer_batch(mu0[:2], taer[:2], rho[:2], P0_atm=P0a[:2], P_aer=Ps[:2], P0_aer=P0r[:2], aer_set=sets[:2], **kw)
    (s,) = M._solvers.values()
    s.set_aerosol_sets(sets[:2])
    info = s.phase_sets_info()
    assert info["groups"] == 0 and not info["single_pass"] and info["group_cap"] == 1
    for b in range(2):
        ref = _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Ps[sets[b]], P0r[b])
        assert r2.n[b] == ref.n
        assert_close(r2.I[b], ref.I, RTOL, "batch of 2, column %d" % b)
    _fresh()


def test_two_pass_fallback_with_sets_per_zone(monkeypatch):
    """Two layers on different sets with the cache bounded to one matrix: the dense tiling's tiles each read the W_aer of
    their set in the second pass; against the superposition helper."""
    monkeypatch.setenv("SOSRT_MIX_GROUPS", "1")
    slabs = [(25, 17, 0.12, 0.97), (12, 8, 0.2, 0.9)]
    mu0, rho = np.array([0.6, 0.75, 0.9]), np.array([0.15, 0.4, 0.0])
    r, refs = _layers_case(60, 32, mu0, rho, slabs, [("hg", 0.7), ("hg", 0.3)])
    (s,) = M._solvers.values()
    assert s.phase_sets_info()["group_cap"] == 1
    for b, ref in enumerate(refs):
        assert r.n[b] == ref.n
        assert_close(r.I[b], ref.I, RTOL, "column %d" % b)
    _fresh()


def test_order_loop_launch_and_float_contraction_with_sets():
    """Order-loop mode 1 is bit-identical to mode 0 with sets; the float contraction of the mixed batch has the bits of the
    float contraction of the set-by-set runs."""
    L, N, B = 200, 128, 12
    mu0, taer, rho, sets = _batch(B, 13)
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200)
    names = dict(aer_phase_fun=["hg", "hg", "fwc"], g_aer=[0.7, 0.3, 0.0])
    _fresh()
    base = SOS_Aer_batch(mu0, taer, rho, aer_set=sets, **names, **kw)
    (s,) = M._solvers.values()
    s.set_order_loop(1)
    planned = s.plan_launch(B, 1)["order_loop"]
    ol = SOS_Aer_batch(mu0, taer, rho, aer_set=sets, **names, **kw)
    launches, refused = s.order_loop_stats()
    s.set_order_loop(0)
    assert planned and launches >= 1                           # the order-loop launch was planned and made
    assert np.array_equal(ol.I, base.I) and np.array_equal(ol.n, base.n)
    s.set_contraction("f32")
    f32 = SOS_Aer_batch(mu0, taer, rho, aer_set=sets, **names, **kw)
    for k, (name, g) in enumerate((("hg", 0.7), ("hg", 0.3), ("fwc", 0.0))):
        c = np.flatnonzero(sets == k)
        one = SOS_Aer_batch(mu0[c], taer[c], rho[c], aer_phase_fun=name, g_aer=g, **kw)
        assert np.array_equal(one.I, f32.I[c]) and np.array_equal(one.n, f32.n[c]), name
    s.set_contraction("f64")
    assert_close(f32.I, base.I, 1e-4, "f32 against f64")
    _fresh()


def test_lambertian_surface_with_two_sets():
    L, N, B = 60, 64, 4
    mu0, taer, rho, sets = _batch(B, 17, nsets=2)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    _fresh()
    r = SOS_Aer_batch(mu0, taer, rho, tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa,
                      P0_atm=P0a, P_aer=Ps[:2], P0_aer=P0r, aer_set=sets, surface="lambertian", **GEOM)
    for b in range(B):
        ref = _oracle(b, mu0, taer, rho, L, N, Pa, P0a, Ps[sets[b]], P0r[b], surface="lambertian")
        assert r.n[b] == ref.n
        assert_close(r.I[b], ref.I, RTOL, "column %d" % b)
    _fresh()


def _layers_case(L, N, mu0, rho, slabs, aerosols):
    """SOS_Aer_layers with slab j on aerosols[j] = (name, g), and the helper's result for the same inputs (the phase data are
    those the driver builds on the device)."""
    _fresh()
    named = [sl + ({"name": a[0], "g": a[1]},) for sl, a in zip(slabs, aerosols)]
    r = SOS_Aer_layers(mu0, rho, named, nb_layers=L, nb_angles=N, max_orders=200)
    (s,) = M._solvers.values()
    refs = []
    for b in range(len(mu0)):
        m = np.array([mu0[b]])
        P0a, Pa = device_phase(s, "rayleigh", m)
        zp = [device_phase(s, a[0], m, a[1]) for a in aerosols]
        zp = [(p0[0], P) for p0, P in zp]
        c = O.make_column_slabs(mu0[b], 120, slabs, L, 0.124, rho[b], 1.0, N, P0a[0], Pa, zp[0][0], zp[0][1])
        refs.append(solve_column_zone_sets(c, zp))
    return r, refs


def test_two_layers_with_different_aerosols_against_the_superposition():
    """Upper layer HG g = 0.7, lower layer HG g = 0.3 (L = 60, N = 32) against the helper at RTOL; both layers on one set has
    the bits of four-entry slabs; the two aerosols swapped give a different field (a set index that is ignored would not)."""
    L, N = 60, 32
    mu0, rho = np.array([0.6, 0.75, 0.9]), np.array([0.15, 0.4, 0.0])
    slabs = [(25, 17, 0.12, 0.97), (12, 8, 0.2, 0.9)]
    r, refs = _layers_case(L, N, mu0, rho, slabs, [("hg", 0.7), ("hg", 0.3)])
    for b, ref in enumerate(refs):
        assert r.n[b] == ref.n
        assert_close(r.I[b], ref.I, RTOL, "column %d" % b)
    sw, _ = _layers_case(L, N, mu0[:1], rho[:1], slabs, [("hg", 0.3), ("hg", 0.7)])
    assert np.max(np.abs(sw.I[0] - r.I[0])) > 1e-3 * np.max(np.abs(r.I[0]))
    _fresh()
    same = SOS_Aer_layers(mu0, rho, [sl + ("hg",) for sl in slabs], nb_layers=L, nb_angles=N, max_orders=200)
    plain = SOS_Aer_layers(mu0, rho, slabs, nb_layers=L, nb_angles=N, max_orders=200)
    assert np.array_equal(same.I, plain.I) and np.array_equal(same.n, plain.n)
    _fresh()


def test_eva_over_wildfire():
    """The reference README's two aerosols at their altitudes, L = 200, N = 128, one column against the helper."""
    slabs = [(25, 17, 0.12, 0.97), (15, 14, 0.0075, 0.9)]
    r, refs = _layers_case(200, 128, np.array([0.5]), np.array([0.15]), slabs, [("eva", 0.0), ("wildfire", 0.0)])
    assert r.n[0] == refs[0].n
    assert_close(r.I[0], refs[0].I, RTOL, "EVA over wildfire")
    _fresh()


@pytest.mark.parametrize("N", [32, 128, 501])
def test_device_fold_is_the_host_fold(N):
    """Three matrices left on the device by phase_matrix_device (HG 0.7, HG 0.3, the FWC table), folded by
    set_phase_sets_device: plan_fold(1 + s) has the bits of the host fold of the same matrices (set_phase_sets), the
    asymmetry and the decision on the symmetric form are the host's; S = 1 likewise; a matrix without the flip symmetry, and
    one with a NaN, switch the symmetric form off."""
    import torch
    s = Solver(20, N, max_batch=1)
    h = Solver(20, N, max_batch=1)
    mu = inputs.direction_grid(N)
    s.set_grid(mu); h.set_grid(mu)
    Pa = s.phase_matrix("rayleigh")
    d_P = torch.empty((3, 2 * N, 2 * N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.set_phase_table(*inputs.fwc_table())
    for k, (kind, g) in enumerate((("hg", 0.7), ("hg", 0.3), ("table", 0.0))):
        s.phase_matrix_device(kind, d_P[k].data_ptr(), g)
    s.synchronize()
    Ps = d_P.cpu().numpy()
    assert np.array_equal(Ps[0], s.phase_matrix("hg", 0.7)) and np.array_equal(Ps[2], s.phase_matrix("table"))
    s.set_phase_sets_device(Pa, d_P.data_ptr(), 3)
    h.set_phase_sets(Pa, Ps)
    assert s.phase_sets_info()["sets"] == 3
    assert s.phase_asymmetry() == h.phase_asymmetry() and s.phase_asymmetry()[1]
    for k in range(3):
        assert np.array_equal(s.plan_fold(1 + k), h.plan_fold(1 + k)), k
    assert np.array_equal(s.plan_fold(0), h.plan_fold(0)) and s.phase_rank() == h.phase_rank()
    s.set_phase_sets_device(Pa, d_P[1].data_ptr(), 1)
    h.set_phase(Pa, Ps[1])
    assert s.phase_sets_info()["sets"] == 1 and np.array_equal(s.plan_fold(1), h.plan_fold(1))
    assert s.phase_asymmetry() == h.phase_asymmetry()
    bad = Ps.copy()
    bad[1, 3, 5] *= 1.5
    d_bad = torch.from_numpy(bad).cuda()
    s.set_phase_sets_device(Pa, d_bad.data_ptr(), 3)
    h.set_phase_sets(Pa, bad)
    assert s.phase_asymmetry() == h.phase_asymmetry() and not s.phase_asymmetry()[1]
    bad[2, 7, 9] = np.nan
    s.set_phase_sets_device(Pa, torch.from_numpy(bad).cuda().data_ptr(), 3)
    assert not s.phase_asymmetry()[1]
    with pytest.raises(ValueError):
        s.set_phase_sets_device(Pa, d_P.data_ptr(), 65)
    with pytest.raises(ValueError):
        s.set_phase_sets_device(Pa, 0, 3)
    s.close(); h.close()


def test_device_folded_sets_solve_like_host_folded_sets():
    """A mixed batch whose matrices were folded on the device has the bits of the batch folded on the host."""
    import torch
    from sosrt.solver import DevicePhaseSets
    L, N, B = 60, 64, 12
    mu0, taer, rho, sets = _batch(B, 23)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=Pa, P0_atm=P0a, P0_aer=P0r,
              aer_set=sets, **GEOM)
    _fresh()
    host = SOS_Aer_batch(mu0, taer, rho, P_aer=Ps, **kw)
    d_P = torch.from_numpy(Ps).cuda()
    torch.cuda.synchronize()
    dev = SOS_Aer_batch(mu0, taer, rho, P_aer=DevicePhaseSets(d_P.data_ptr(), 3, keep=d_P), **kw)
    assert np.array_equal(dev.I, host.I) and np.array_equal(dev.n, host.n) and (dev.status == 0).all()
    _fresh()


def test_spectrum_in_one_batch_against_the_loop():
    """8 wavelengths x 6 columns: one_batch=True returns what the per-wavelength loop returns, np.array_equal per wavelength
    -- both take the single pass (the loop: one group per solve; the one batch: 8 groups), asserted below."""
    from sosrt.main import SOS_Aer_spectrum
    wl = np.linspace(0.40, 0.87, 8)
    mu0 = np.array([0.3, 0.5, 0.7, 0.9, 0.4, 0.6])
    rho = np.array([0.0, 0.1, 0.3, 0.05, 0.5, 0.2])
    aer = dict(m=1.44 + 0.001j, r_m=0.35, sig=1.5)
    kw = dict(angstrom=1.3, nb_layers=60, nb_angles=64, nb_radius=40, ntab=2001, max_orders=200)
    _fresh()
    loop, bulk = SOS_Aer_spectrum(wl, mu0, 0.12, rho, aer, **kw)
    one, bulk1 = SOS_Aer_spectrum(wl, mu0, 0.12, rho, aer, one_batch=True, **kw)
    (s,) = M._solvers.values()
    s.set_aerosol_sets(np.repeat(np.arange(8, dtype=np.int32), 6))
    info = s.phase_sets_info()
    assert info["sets"] == 8 and info["groups"] == 8 and info["single_pass"]
    assert np.array_equal(bulk, bulk1) and len(one) == len(loop) == 8
    for w in range(8):
        assert (loop[w].status == 0).all()
        assert np.array_equal(one[w].n, loop[w].n), w
        assert np.array_equal(one[w].I, loop[w].I), w
        assert np.array_equal(one[w].tau, loop[w].tau)
    with pytest.raises(ValueError, match="at most 64"):
        SOS_Aer_spectrum(np.linspace(0.4, 0.9, 65), mu0, 0.12, rho, aer, one_batch=True, **kw)
    _fresh()


def test_refusals():
    L, N, B = 60, 32, 6
    mu0, taer, rho, sets = _batch(B, 19)
    Pa, P0a, Ps, P0s = _three_sets(N, mu0)
    P0r = P0s[sets, np.arange(B)]
    kw = dict(tauStar_atm=0.124, nb_layers=L, nb_angles=N, P_atm=Pa, P0_atm=P0a, P_aer=Ps, P0_aer=P0r, **GEOM)
    _fresh()
    with pytest.raises(ValueError, match="azimuths"):
        SOS_Aer_batch(mu0, taer, rho, aer_set=sets, azimuths=np.array([0.0, 1.0]), **kw)
    with pytest.raises(ValueError, match="readme"):
        SOS_Aer_batch(mu0, taer, rho, aer_set=sets, first_order="readme", surface="lambertian_readme", **kw)
    with pytest.raises(ValueError, match="devices"):
        SOS_Aer_batch(mu0, taer, rho, aer_set=sets, devices=[0, 1], **kw)
    with pytest.raises(ValueError, match="aer_set"):
        SOS_Aer_batch(mu0, taer, rho, **kw)                                    # a stack without aer_set
    with pytest.raises(ValueError):
        SOS_Aer_batch(mu0, taer, rho, aer_set=np.full(B, 3, dtype=np.int32), **kw)   # a set that is not there
    # handle level
    s = Solver(L, N, max_batch=B)
    mu = inputs.direction_grid(N)
    s.set_grid(mu)
    s.set_phase_sets(Pa, Ps)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    cols = lambda surface="specular": s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.95, 0.124 / L,
                                                    taer / (idn + 1 - iu), 0.124 + taer, surface=surface)
    cols("lambertian_readme")
    with pytest.raises(ValueError, match="README"):
        s.set_first_order("readme")
    cols()
    with pytest.raises(ValueError, match="outside"):
        s.set_aerosol_sets(np.array([0, 1, 2, 3, 0, 1]))
    with pytest.raises(ValueError, match="outside"):
        s.set_aerosol_sets(np.array([0, -1, 2, 0, 0, 1]))
    s.set_aerosol_sets(sets)
    with pytest.raises(ValueError, match="use aerosol set 2"):
        s.set_phase_sets(Pa, Ps[:2])                                           # fewer sets than the columns use
    with pytest.raises(ValueError, match="use aerosol set 2"):
        s.set_phase(Pa, Ps[0])
    cols()                                                                     # back on set 0
    s.set_phase(Pa, Ps[0])
    s.close()
    _fresh()


# ---- one handle through grow, reuse and a smaller request of every grow-only buffer -----------------------------------------
def _walk_step(s, step, L, mu0, taer, Pa, P0a, Ps, P0s):
    """Puts columns, phase data and sets of `step` on `s`; returns (tau, P0_atm, P0_aer) of its solve."""
    B = len(mu0)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, 0.15, 1.0, 0.95, 0.124 / L, taer / (idn + 1 - iu), 0.124 + taer)
    tau = np.stack([inputs.tau_profile(0.124, x, 120, 25, 17, L) for x in taer])
    kind, S, sets = step
    if kind == "plain":
        s.set_phase(Pa, Ps[0])
        return tau, P0a, P0s[0]
    s.set_phase_sets(Pa, Ps[:S])
    sets = np.asarray(sets, dtype=np.int32)
    if kind == "zones":                                  # a [B, 3] table: P0_aer is one row per zone of it
        table = np.zeros((B, 3), dtype=np.int32)
        table[:, 1] = sets
        s.set_aerosol_sets(table)
        P0r = np.zeros((B, 3, P0a.shape[1]))
        P0r[:, 1] = P0s[sets, np.arange(B)]
        return tau, P0a, P0r
    s.set_aerosol_sets(sets)
    return tau, P0a, P0s[sets, np.arange(B)]


@pytest.mark.parametrize("contraction", ["f64", "f32"])
def test_buffers_regrown_on_one_handle_leave_no_stale_state(contraction):
    """One handle (L = 24, N = 16, B = 4, three zones, specular) solves with 2 sets, 5 sets (two columns on set 4), 2 sets
    again, a per-zone P0_aer, and the plain single-set call: the stacks of folds, the combined matrices, their folded and
    float copies and the P0 staging grow, are reused and meet a smaller request.  After every step field, order counts and
    status are those of a fresh handle given that step alone, bit for bit.  A step the contraction refuses on the fresh
    handle must be refused on the walked one too."""
    L, N, B = 24, 16, 4
    # four (ca, cr) pairs; aerosol this thin because at N = 16 the reference ends a thicker column in the IndexError of spec:404
    # (the oracle solves each of these columns with each of the five sets in 7 to 9 orders)
    mu0, taer = np.array([0.45, 0.65, 0.85, 0.95]), np.array([0.03, 0.02, 0.01, 0.005])
    mu = O.make_mu(N)
    Pa = O.phase_rayleigh(N, mu, 0.5)[1]
    P0a = np.stack([O.phase_rayleigh(N, mu, m)[0] for m in mu0])
    gs = (0.7, 0.3, 0.5, 0.1, 0.8)
    Ps = np.stack([O.phase_hg(N, mu, 0.5, g)[1] for g in gs])
    P0s = np.stack([np.stack([O.phase_hg(N, mu, m, g)[0] for m in mu0]) for g in gs])
    steps = [("cols", 2, [0, 1, 0, 1]), ("cols", 5, [4, 1, 4, 2]), ("cols", 2, [0, 1, 0, 1]), ("zones", 2, [1, 0, 1, 0]),
             ("plain", 1, None)]

    def make():
        s = Solver(L, N, max_batch=B)
        s.set_grid(inputs.direction_grid(N))
        s.set_contraction(contraction)
        return s

    walked, solved = make(), 0
    for i, step in enumerate(steps):
        fresh = make()
        try:
            want = fresh.solve(*_walk_step(fresh, step, L, mu0, taer, Pa, P0a, Ps, P0s))
        except ValueError:
            want = None
        if want is None:
            with pytest.raises(ValueError):
                walked.solve(*_walk_step(walked, step, L, mu0, taer, Pa, P0a, Ps, P0s))
        else:
            got = walked.solve(*_walk_step(walked, step, L, mu0, taer, Pa, P0a, Ps, P0s))
            if contraction == "f64" and step[0] != "plain":
                # not vacuous: mix groups, the symmetric fold and the low-rank rows are all active on this handle
                assert walked.phase_sets_info()["groups"] > 1 and walked.phase_asymmetry()[1] and walked.phase_rank()[2]
            assert np.array_equal(got.I, want.I), (i, step)
            assert np.array_equal(got.n, want.n) and np.array_equal(got.status, want.status), (i, step)
            assert np.all(want.n > 2) and np.all(want.status == 0)      # every column ran its orders to convergence
            solved += 1
        fresh.close()
    walked.close()
    assert solved == len(steps) or contraction != "f64"
