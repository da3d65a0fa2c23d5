"""The stage kernels beside the solve on the device, through the C ABI, at the shapes the product ships at and at the limits the
header promises (tests/stage_shape_cases.py: floor N = 4, headline N = 128 / L = 200, shipped-N 501, cap-N 1024, cap-L 2048 with a
second two-slab zone table, many-columns B = 70 at N = 130), each against the NumPy model of that kernel with the measure and the
bound of the kernel's small-shape test.  Every output lies between two guards of NaN that must stay NaN.

What each test reaches that no other test of the suite does:

    test_slant_kernel                k_beam_slant with up to 32 level blocks and B > 1 (b = blockIdx.x / nblk)
    test_first_order_beam_kernel     k_first_order_beam: 64 KiB of dynamic LDS at L = 2048; nblk = 2 (full), 3 (with B = 70), 8, 16; the
                                     idle lanes' alias onto the node lane at N = 4, 130, 501
    test_beam_epilogue               k_epilogue_beam: L > 256 in the heating-rate stride, N in up to 16 trips of the flux loop,
                                     erase_pics beyond row 256 (cap-L-2slabs)
    test_view_beam_kernel            k_view_first_order_beam at 64 KiB of LDS; 300 levels as two launches, 2048 as eight
    test_emission_kernel             k_emission with up to 16 waves and the Lambertian cross-wave sum through s_red[16]
    test_emission_view_kernel        sosrt_emission_view_dev's second launch (out + l0 * 2V); V = 33, 64
    test_emission_epilogue           k_epilogue_emission as test_beam_epilogue
    test_view_radiance               k_view_source above N = 64 (k-chunks, Dp padding at D = 8, 1002), all three instantiations against
                                     the model off the grid; both chunk loops of sosrt_view_radiance_dev
    test_ground_source, test_ground_source_terms
                                     workgroups of up to 1024 threads
    test_ground_field                k_ground_first_order's ballot search in up to 16 trips and at N = 4, where one lane can pass
    test_bounce_accumulate           k_bounce_accumulate at the shapes
    test_view_ground, test_view_ground_terms
                                     the second launch of the two view-ground entries (the level table padded with 0)
    test_beam_and_emission_refuse_L_2049, test_V_65_is_refused_and_V_64_served
                                     the refusals of beam_check and emission_check at kBeamMaxL + 1, of V = SOSRT_MAX_VIEWS + 1
    test_view_scratch_grows_and_shrinks_with_the_call
                                     the handle's view scratch (d_fold, d_S) from V = 5 to 64 and back, from 6 levels to 300 and back
    test_first_order_profile_kernel  k_first_order_profile<false>: 48 KiB of dynamic LDS at kProfileMaxL = 1024; nblk = 1, 3 (with B =
                                     70: b = blockIdx.x / nblk with a remainder), 8, 16; zone boundaries deep in a long column
    test_first_order_profile_kernel_with_a_p0_per_zone
                                     k_first_order_profile<true> at L = 1024 on the two-slab table
    test_emission_profile_kernel     k_emission_profile's 1024-thread workgroup and its cross-wave sum over 16 waves on both
                                     Lambertian grounds; L = 1024
    test_profile_stage_refuses_L_1025
                                     the refusal of profile_check at kProfileMaxL + 1

At cap-L the emitted field is compared with the model's long double evaluation (stage_shape_cases.thermal_reference): float64
NumPy alone is 2e-13 from it there, a fifth of the bound of 1e-12, which stays."""
import numpy as np
import pytest

import brdf_np as G
import brdf_view_np as BV
import ross_li_np as RL
import sos_oracle as O
import spherical_np as S
import stage_shape_cases as C
import thermal_np as T
import view_np as VN
from sosrt.solver import Solver
from test_gpu_brdf import smooth_source
from test_gpu_profile import KERNEL_BAR, UNIT_BAR, set_cols, set_weights
from test_gpu_spherical import SURFACES, _err, _torch, dev, handle, host, sync
from test_gpu_thermal import handle as thermal_handle
from test_gpu_view import off_grid_columns, three_zone_solver
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu

EPI = ("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")


class Guarded:
    """A float64 output of `shape` on the device between two guards of NaN, each a row of the output long (at least 16 elements):
    `ptr` is the output's address, `get` checks the guards and returns the output."""

    def __init__(self, shape, fill=np.nan):
        torch = _torch()
        self.shape = tuple(int(n) for n in shape)
        self.n = int(np.prod(self.shape))
        self.pad = (max(self.shape[-1], 16) + 1) // 2 * 2
        self.buf = torch.full((self.n + 2 * self.pad,), np.nan, dtype=torch.float64, device=torch.device("cuda", 0))
        if not np.isnan(fill):
            self.buf[self.pad:self.pad + self.n] = fill
        self.ptr = self.buf.data_ptr() + 8 * self.pad

    def get(self, s):
        a = host(self.buf, s)
        assert np.all(np.isnan(a[:self.pad])) and np.all(np.isnan(a[self.pad + self.n:])), "the call wrote outside its output"
        return a[self.pad:self.pad + self.n].reshape(self.shape)


def plus_zero(a):
    return not np.any(a) and not np.any(np.signbit(a))


def mx(a):
    return float(np.max(np.abs(a)))


def beam_handle(name, surface="specular"):
    cols = C.beam_columns(name)
    return (cols,) + handle(cols, surface, phase=False, max_orders=1)


# ---- the beam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SIX)
def test_slant_kernel(name):
    cols, s, tau, _, _ = beam_handle(name)
    ref = C.beam_model(name)[0]
    B, L = tau.shape
    d_tau, d_z = dev(tau), dev(S.altitudes(L))

    def run(B):
        out = Guarded((B, L))
        sync()
        s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), out.ptr, B=B)
        return out.get(s)

    got = run(B)
    assert np.all(np.isfinite(got)) and np.all(got[:, 0] == 0)
    assert np.array_equal(run(B), got)                       # the same call: the same bits
    assert np.array_equal(run(1)[0], got[0])                 # the first column alone: the same bits
    worst = max(_err(got[b], ref[b]) for b in range(B))
    print("%s: slant kernel vs model %.3e of max sigma" % (name, worst))
    assert worst <= 1e-12
    suns = [c.mu0 for c in cols]
    assert 1.0 in suns and 0.05 in suns
    for b, c in enumerate(cols):
        if c.mu0 == 1.0:
            assert np.max(np.abs(got[b] - tau[b])) <= 1e-15, "mu0 = 1 must give tau"
    s.close()


@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_first_order_beam_kernel(name):
    sig, ref = C.beam_model(name)
    for surface in SURFACES:
        cols, s, tau, P0a, P0r = beam_handle(name, surface)
        B, L = tau.shape
        d = [dev(x) for x in (tau, sig, P0a, P0r)]

        def run(B):
            out = Guarded((B, L, s.D))
            sync()
            s.first_order_beam_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.ptr, B=B)
            return out.get(s)

        got = run(B)
        assert np.all(np.isfinite(got))
        worst = max(_err(got[b], ref[b]) for b in range(B))
        print("%s %s: first-order kernel vs model %.3e of the field maximum" % (name, surface, worst))
        assert worst <= 1e-12
        if surface == "specular":
            assert np.array_equal(run(B), got) and np.array_equal(run(1)[0], got[0])
        s.close()


def run_epilogue(s, B, L, call):
    out = {k: Guarded((B,) if k == "net_toa" else (B, L)) for k in EPI}
    sync()
    call(*[out[k].ptr for k in EPI])
    return {k: out[k].get(s) for k in EPI}


@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_beam_epilogue(name):
    cols, s, tau, _, _ = beam_handle(name)
    sig, I = C.beam_model(name)
    B, L = tau.shape
    d_tau, d_I, d_sig, d_z = dev(tau), dev(I), dev(sig), dev(S.altitudes(L))
    for norm in ("crit", "graphe"):
        call = lambda *p, B=B: s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), d_z.data_ptr(), norm, *p, B=B)
        got, ref = run_epilogue(s, B, L, call), C.beam_epilogue_model(name, norm)
        worst = {k: max(_err(np.atleast_1d(got[k][b]), np.atleast_1d(ref[k][b])) for b in range(B)) for k in EPI}
        print("%s %s: beam epilogue vs NumPy %s" % (name, norm, ", ".join("%s %.3e" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1e-10, worst
        again, one = run_epilogue(s, B, L, call), run_epilogue(s, 1, L, lambda *p: call(*p, B=1))
        assert all(np.array_equal(again[k], got[k]) and np.array_equal(one[k][0], got[k][0]) for k in EPI)
    s.close()


@pytest.mark.parametrize("V", [33, 64])
@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_view_beam_kernel(name, V):
    cols, s, tau, _, _ = beam_handle(name)
    mv, p0a, p0r, ref = C.beam_view_case(name, V)
    B, L = tau.shape
    d = [dev(x) for x in (tau, C.beam_model(name)[0], p0a, p0r)]

    def run(levels, B=B):
        out = Guarded((B, len(levels), 2 * V))
        sync()
        s.view_first_order_beam_device(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), levels, out.ptr, B=B)
        return out.get(s)

    levels = C.levels_300(L)
    top = np.max(np.abs(ref), axis=(1, 2))[:, None, None]
    got = run(levels)
    assert np.all(np.isfinite(got))
    worst = float(np.max(np.abs(got - ref[:, levels]) / top))
    print("%s V=%d: view beam kernel at 300 levels vs model %.3e of the field maximum" % (name, V, worst))
    assert worst <= 1e-12
    assert np.array_equal(run(levels), got)
    assert np.array_equal(np.concatenate((run(levels[:256]), run(levels[256:])), axis=1), got)   # one call of 300 is two of 256 and 44
    assert np.array_equal(run(levels, B=1)[0], got[0])
    if name in C.CAP_L:                                      # every level: eight launches
        every = run(list(range(L)))
        worst = float(np.max(np.abs(every - ref) / top))
        print("%s V=%d: view beam kernel at all %d levels vs model %.3e" % (name, V, L, worst))
        assert worst <= 1e-12 and np.array_equal(every[:, levels], got)
    s.close()


# ---- thermal emission ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_emission_kernel(name, surface):
    cols = C.thermal_columns(name, surface)
    pl, bs, es = C.thermal_sources(name)
    s, tau = thermal_handle(cols, phase=False, max_orders=1)
    B, L = tau.shape
    d = [dev(x) for x in (tau, pl, bs, es)]

    def run(explicit, B=B):
        out = Guarded((B, L, s.D))
        sync()
        s.emission_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.ptr, d[3].data_ptr() if explicit else 0, B=B)
        return out.get(s)

    for explicit in (False, True):
        ref = C.thermal_reference(name, surface, explicit)
        got = run(explicit)
        assert np.all(np.isfinite(got))
        worst = max(_err(got[b], ref[b]) for b in range(B))
        print("%s %s emissivity %s: emission kernel vs model %.3e of the field maximum" % (name, surface, "given" if explicit else "1 - rho", worst))
        assert worst <= 1e-12
    assert np.array_equal(run(True), got) and np.array_equal(run(True, B=1)[0], got[0])
    s.close()


@pytest.mark.parametrize("V", [33, 64])
@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_emission_view_kernel(name, V):
    cols = C.thermal_columns(name, "specular")
    pl, bs, es = C.thermal_sources(name)
    mv, ref = C.thermal_view_reference(name, V)
    s, tau = thermal_handle(cols, phase=False, max_orders=1)
    B, L = tau.shape
    d = [dev(x) for x in (tau, pl, bs, es)]

    def run(levels, B=B):
        out = Guarded((B, len(levels), 2 * V))
        sync()
        s.emission_view_device(mv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), levels, out.ptr, d[3].data_ptr(), B=B)
        return out.get(s)

    levels = C.levels_300(L)
    got = run(levels)
    assert np.all(np.isfinite(got))
    worst = max(_err(got[b], ref[b][levels]) for b in range(B))
    print("%s V=%d: emission view kernel at 300 levels vs model %.3e" % (name, V, worst))
    assert worst <= 1e-12
    assert np.array_equal(run(levels), got)
    assert np.array_equal(np.concatenate((run(levels[:256]), run(levels[256:])), axis=1), got)
    assert np.array_equal(run(levels, B=1)[0], got[0])
    if name in C.CAP_L:
        every = run(list(range(L)))
        worst = max(_err(every[b], ref[b]) for b in range(B))
        print("%s V=%d: emission view kernel at all %d levels vs model %.3e" % (name, V, L, worst))
        assert worst <= 1e-12 and np.array_equal(every[:, levels], got)
    s.close()


@pytest.mark.parametrize("name", C.WITH_SLABS)
def test_emission_epilogue(name):
    cols = C.thermal_columns(name, "specular")
    I = C.thermal_model(name, "specular", False)
    s, tau = thermal_handle(cols, phase=False, max_orders=1)
    B, L = tau.shape
    d_tau, d_I, d_z = dev(tau), dev(I), dev(T.altitudes(L))
    call = lambda *p, B=B: s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), *p, B=B)
    got, ref = run_epilogue(s, B, L, call), C.thermal_epilogue_model(name)
    worst = dict.fromkeys(EPI, 0.0)
    for b, c in enumerate(cols):
        for k in EPI:
            # (a column whose atmosphere has tau* < 1e-3: its fluxes are checked, its heating rate is not; tests/test_gpu_thermal.py)
            if k == "heating_rate" and c.tauStar_tot < 1e-3:
                continue
            worst[k] = max(worst[k], _err(np.atleast_1d(got[k][b]), np.atleast_1d(ref[k][b])))
    print("%s: emission epilogue vs NumPy %s" % (name, ", ".join("%s %.3e" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1e-10, worst
    again, one = run_epilogue(s, B, L, call), run_epilogue(s, 1, L, lambda *p: call(*p, B=1))
    assert all(np.array_equal(again[k], got[k]) and np.array_equal(one[k][0], got[k][0]) for k in EPI)
    s.close()


# ---- view radiance -------------------------------------------------------------------------------------------------------------------------
def run_view(s, mv, d, levels, quad, B, scat=True, first=True):
    """(scattered, first order) [B, nlev, 2V] of sosrt_view_radiance_dev; d: the device arrays of a view case and tau"""
    V2 = 2 * len(mv)
    o_scat, o_first = (Guarded((B, len(levels), V2)) for _ in range(2))
    sync()
    s.view_radiance_device(mv, d["tau"].data_ptr(), d["src"].data_ptr(), d["rows_atm"].data_ptr(), d["rows_aer"].data_ptr(), levels,
                           d_scat_out=o_scat.ptr if scat else 0, d_first_out=o_first.ptr if first else 0,
                           d_p0rows_atm=d["p0a"].data_ptr(), d_p0rows_aer=d["p0r"].data_ptr(), quadrature=quad, B=B)
    return o_scat.get(s), o_first.get(s)


@pytest.mark.parametrize("V", [5, 33, 64])
@pytest.mark.parametrize("name", C.VIEW_SHAPES)
def test_view_radiance(name, V):
    cols = C.view_columns(name)
    k = C.view_case(name, V)
    s, tau, _, _ = handle(cols, phase=False, max_orders=1)
    B, L = tau.shape
    d = {x: dev(k[x]) for x in ("src", "rows_atm", "rows_aer", "p0a", "p0r")}
    d["tau"] = dev(tau)
    levels = C.levels_300(L)
    for quad in ("grid", "linear"):
        scat, first = run_view(s, k["mv"], d, levels, quad, B)
        e1 = assert_close(scat, k["scat"][quad][:, levels], RTOL, "%s scattered radiance" % quad)
        e2 = assert_close(first, k["first"][:, levels], RTOL, "first order")
        print("%s V=%d %s: scattered %.2e, first order %.2e" % (name, V, quad, e1, e2))
        again = run_view(s, k["mv"], d, levels, quad, B)
        assert np.array_equal(again[0], scat) and np.array_equal(again[1], first)
        a, b = run_view(s, k["mv"], d, levels[:256], quad, B), run_view(s, k["mv"], d, levels[256:], quad, B)
        assert np.array_equal(np.concatenate((a[0], b[0]), axis=1), scat) and np.array_equal(np.concatenate((a[1], b[1]), axis=1), first)
        one = run_view(s, k["mv"], d, levels, quad, 1)
        assert np.array_equal(one[0][0], scat[0]) and np.array_equal(one[1][0], first[0])
    s.close()


# ---- the BRDF ground -------------------------------------------------------------------------------------------------------------------------
def run_source(s, d, B, r0=True, scale=True):
    out = Guarded((B, s.N - 1))
    sync()
    s.ground_source_device(d["I"].data_ptr(), d["tau"].data_ptr(), d["R"].data_ptr(), out.ptr, d["r0"].data_ptr() if r0 else 0,
                           d["scale"].data_ptr() if scale else 0, B=B)
    return out.get(s)


def run_source_terms(s, K, d_I, d_tau, d_R, d_w, d_r0, B):
    out = Guarded((B, s.N - 1))
    sync()
    s.ground_source_terms_device(K, d_I.data_ptr(), d_tau.data_ptr(), d_R.data_ptr(), d_w.data_ptr(), out.ptr,
                                 0 if d_r0 is None else d_r0.data_ptr(), B=B)
    return out.get(s)


@pytest.mark.parametrize("name", C.SIX)
def test_ground_source(name):
    cols, s, tau, _, _ = beam_handle(name)
    g = C.ground_case(name)
    B = len(cols)
    d = dict(I=dev(g["I"]), tau=dev(tau), R=dev(g["R"].T), r0=dev(g["r0"]), scale=dev(g["scale"]))
    for use_r0, use_scale in ((True, True), (False, True), (True, False), (False, False)):
        ref = np.stack([G.ground_source(g["R"], g["I"][b, -1], g["r0"][b] if use_r0 else None, tau[b, -1], cols[b].mu0,
                                        g["scale"][b] if use_scale else 1.0) for b in range(B)])
        got = run_source(s, d, B, use_r0, use_scale)
        live = [b for b in range(B) if not (use_scale and g["scale"][b] == 0)]
        err = max(np.max(np.abs(got[b] - ref[b]) / np.abs(ref[b])) for b in live)
        print("%s beam %s scale %s: ground source %.3e relative" % (name, use_r0, use_scale, err))
        assert err <= 1e-13
        if use_scale:
            assert len(live) < B and all(plus_zero(got[b]) for b in range(B) if b not in live)    # scale 0: exact +0
        assert np.array_equal(run_source(s, d, B, use_r0, use_scale), got)
        assert np.array_equal(run_source(s, d, 1, use_r0, use_scale)[0], got[0])
    s.close()


@pytest.mark.parametrize("name", C.SIX)
def test_ground_source_terms(name):
    cols, s, tau, _, _ = beam_handle(name)
    g = C.ground_case(name)
    B = len(cols)
    d_I, d_tau, d_R, d_w, d_r0 = dev(g["I"]), dev(tau), dev(np.swapaxes(g["Rs"], 1, 2)), dev(g["weight"]), dev(g["r0s"])
    for beam in (d_r0, None):
        ref = np.stack([RL.ground_source_terms(g["Rs"], g["I"][b, -1], None if beam is None else g["r0s"][:, b], tau[b, -1], cols[b].mu0,
                                               g["weight"][b]) for b in range(B)])
        got = run_source_terms(s, 3, d_I, d_tau, d_R, d_w, beam, B)
        err = mx(got - ref) / mx(ref)
        print("%s beam %s: ground source over 3 terms %.3e of its maximum" % (name, beam is not None, err))
        assert err <= 1e-13
        assert plus_zero(got[1])                             # all weights 0: exact +0
        assert np.array_equal(run_source_terms(s, 3, d_I, d_tau, d_R, d_w, beam, B), got)
        assert np.array_equal(run_source_terms(s, 3, d_I, d_tau, d_R, d_w, beam, 1)[0], got[0])
    # K = 1: the bits of the single-term kernel with scale = weight
    w0 = dev(g["weight"][:, :1].copy())
    d = dict(I=d_I, tau=d_tau, R=dev(g["Rs"][0].T), r0=dev(g["r0s"][0]), scale=w0)
    assert np.array_equal(run_source_terms(s, 1, d_I, d_tau, d["R"], w0, d["r0"], B), run_source(s, d, B))
    s.close()


def run_field(s, d_tau, S, B, L):
    torch = _torch()
    d_S, out = dev(S), Guarded((B, L, s.D))
    d_st = torch.full((B + 2,), -7, dtype=torch.int32, device=d_tau.device)
    sync()
    s.ground_first_order_device(d_tau.data_ptr(), d_S.data_ptr(), out.ptr, d_st.data_ptr() + 4, B=B)
    G_, st = out.get(s), d_st.cpu().numpy()
    assert st[0] == -7 and st[-1] == -7, "the call wrote outside its status"
    return G_, st[1:-1]


@pytest.mark.parametrize("name", C.SIX)
def test_ground_field(name):
    cols, s, tau, _, _ = beam_handle(name)
    B, L = tau.shape
    N = cols[0].N
    d_tau = dev(tau)
    # (N = 4: the one lane the search can test passes where the source is small enough for its absolute 1e-4)
    smooth = smooth_source(N, B) * (0.01 if N == 4 else 1.0)
    sources = [("smooth", smooth)] + ([("rough then smooth", C.rough_then_smooth(smooth))] if N >= 66 else [])
    for what, S_ in sources:
        got, st = run_field(s, d_tau, S_, B, L)
        assert np.array_equal(st, np.zeros(B, dtype=np.int32))
        e_plain, e_blend, lanes = 0.0, 0.0, 0
        for b, c in enumerate(cols):
            ref, status, blended = G.ground_field(S_[b], c.tau, c.mu, N)
            d = np.abs(got[b] - ref) / np.max(ref)
            assert status == 0 and blended.any()
            e_plain, e_blend, lanes = max(e_plain, np.max(d[~blended])), max(e_blend, np.max(d[blended])), max(lanes, blended.sum(axis=1).max())
            assert plus_zero(got[b][:, :N + 1])              # lane N and the downward lanes: +0
        print("%s %s: ground field %.3e unblended, %.3e blended, up to %d blended lanes in a row" % (name, what, e_plain, e_blend, lanes))
        assert e_plain <= 1e-12 and e_blend <= 1e-10
        if what != "smooth":
            assert lanes >= N - 12                           # the search went on into its last trip of 64 lanes
        again, _ = run_field(s, d_tau, S_, B, L)
        one, _ = run_field(s, d_tau, S_[:1], 1, L)
        assert np.array_equal(again, got) and np.array_equal(one[0], got[0])
    s.close()


@pytest.mark.parametrize("name", C.SIX)
def test_bounce_accumulate(name):
    cols, s, tau, _, _ = beam_handle(name)
    B, L = tau.shape
    N = cols[0].N
    total0 = np.array(C.ground_case(name)["I"])
    Ik = 0.01 * total0[:, ::-1, ::-1] * np.array([(1.0, -1.0, 0.5)[b % 3] for b in range(B)])[:, None, None]
    Ik[1, 0, N:] = Ik[1, -1, :N] = 0
    total0[1, 0, N:] = total0[1, -1, :N] = 0                 # the second column: both rows of the ratio are zero in the total
    d_Ik, ratio = dev(Ik), Guarded((B,))
    tot = Guarded((B, L, 2 * N))
    tot.buf[tot.pad:tot.pad + tot.n] = dev(total0).reshape(-1)
    sync()
    s.bounce_accumulate_device(d_Ik.data_ptr(), tot.ptr, ratio.ptr, B=B)
    got, r = tot.get(s), ratio.get(s)
    assert np.array_equal(got, total0 + Ik)
    ref = np.array([G.bounce_ratio(Ik[b], (total0 + Ik)[b], N) for b in range(B)])
    print("%s: ratios within %.3e of the model's" % (name, np.max(np.abs(r - ref) / np.maximum(ref, 1))))
    assert r[1] == 0 and np.all(np.abs(r - ref) <= 1e-15 * np.maximum(ref, 1))
    s.close()


def run_view_ground(s, mv, d_tau, levels, B, d_I=None, d_Rv=None, d_r0v=None, d_w=None, K=None):
    """(out [B, nlev, 2V], S [B, V]) of sosrt_view_ground_dev (d_w: the scale, or None) or with K of sosrt_view_ground_terms_dev"""
    V = len(mv)
    out, S_ = Guarded((B, len(levels), 2 * V)), Guarded((B, V))
    ptr = lambda t: 0 if t is None else t.data_ptr()
    sync()
    if K is None:
        s.view_ground_device(mv, d_tau.data_ptr(), levels, out.ptr, d_I=ptr(d_I), d_Rv=ptr(d_Rv), d_r0v=ptr(d_r0v), d_scale=ptr(d_w),
                             d_S_out=S_.ptr, B=B)
    else:
        s.view_ground_terms_device(K, mv, d_tau.data_ptr(), levels, d_w.data_ptr(), out.ptr, d_I=ptr(d_I), d_Rv=ptr(d_Rv), d_r0v=ptr(d_r0v),
                                   d_S_out=S_.ptr, B=B)
    return out.get(s), S_.get(s)


@pytest.mark.parametrize("V", [33, 64])
@pytest.mark.parametrize("name", C.SIX)
def test_view_ground(name, V):
    cols, s, tau, _, _ = beam_handle(name)
    g, v = C.ground_case(name), C.ground_view_case(name, V)
    B, L = tau.shape
    mv = v["mv"]
    d_tau, d_I, d_Rv, d_r0v, d_sc = dev(tau), dev(g["I"]), dev(v["Rv"].T), dev(v["r0v"]), dev(g["scale"])
    levels = C.levels_300(L)
    run = lambda levels, B=B: run_view_ground(s, mv, d_tau, levels, B, d_I, d_Rv, d_r0v, d_sc)
    got, S_ = run(levels)
    eS = eG = 0.0
    for b, c in enumerate(cols):
        if g["scale"][b] == 0:
            assert plus_zero(got[b]) and plus_zero(S_[b])
            continue
        Sref = G.ground_source(v["Rv"], g["I"][b, -1], v["r0v"][b], tau[b, -1], c.mu0, g["scale"][b])
        ref = BV.view_ground(Sref, tau[b], mv)[levels]
        eS, eG = max(eS, np.max(np.abs(S_[b] - Sref) / np.abs(Sref))), max(eG, np.max(np.abs(got[b] - ref)) / np.max(ref))
        assert plus_zero(got[b][:, :V])                      # downward lanes: exactly +0
    print("%s V=%d: view ground at 300 levels: source %.3e relative, radiance %.3e of its maximum" % (name, V, eS, eG))
    assert eS <= 1e-13 and eG <= 1e-12
    again, a, b_ = run(levels), run(levels[:256]), run(levels[256:])
    assert np.array_equal(again[0], got) and np.array_equal(again[1], S_)
    assert np.array_equal(np.concatenate((a[0], b_[0]), axis=1), got) and np.array_equal(a[1], S_) and np.array_equal(b_[1], S_)
    one = run(levels, B=1)
    assert np.array_equal(one[0][0], got[0]) and np.array_equal(one[1][0], S_[0])
    s.close()


@pytest.mark.parametrize("V", [33, 64])
@pytest.mark.parametrize("name", C.SIX)
def test_view_ground_terms(name, V):
    cols, s, tau, _, _ = beam_handle(name)
    g, v = C.ground_case(name), C.ground_view_case(name, V)
    B, L = tau.shape
    mv = v["mv"]
    d_tau, d_I, d_Rv, d_r0v, d_w = dev(tau), dev(g["I"]), dev(np.swapaxes(v["Rvs"], 1, 2)), dev(v["r0vs"]), dev(g["weight"])
    levels = C.levels_300(L)
    run = lambda levels, B=B: run_view_ground(s, mv, d_tau, levels, B, d_I, d_Rv, d_r0v, d_w, K=3)
    got, S_ = run(levels)
    Sref = np.stack([RL.ground_source_terms(v["Rvs"], g["I"][b, -1], v["r0vs"][:, b], tau[b, -1], cols[b].mu0, g["weight"][b]) for b in range(B)])
    ref = np.stack([BV.view_ground(Sref[b], tau[b], mv)[levels] for b in range(B)])
    eS, eG = mx(S_ - Sref) / mx(Sref), mx(got - ref) / mx(ref)
    print("%s V=%d: view ground over 3 terms at 300 levels: source %.3e, radiance %.3e of their maxima" % (name, V, eS, eG))
    assert eS <= 1e-13 and eG <= 1e-13
    assert plus_zero(got[:, :, :V]) and plus_zero(got[1]) and plus_zero(S_[1])       # downward lanes; all weights 0
    again, a, b_ = run(levels), run(levels[:256]), run(levels[256:])
    assert np.array_equal(again[0], got) and np.array_equal(again[1], S_)
    assert np.array_equal(np.concatenate((a[0], b_[0]), axis=1), got)
    one = run(levels, B=1)
    assert np.array_equal(one[0][0], got[0]) and np.array_equal(one[1][0], S_[0])
    s.close()


# ---- per-level weights on the source function ----------------------------------------------------------------------------
def run_first_order(s, d, B, L, profile=True):
    out = Guarded((B, L, s.D))
    sync()
    f = s.first_order_profile_device if profile else s.first_order_beam_device
    f(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.ptr, B=B)
    return out.get(s)


@pytest.mark.parametrize("path", ["plane", "slant"])
@pytest.mark.parametrize("name", C.PROFILE)
def test_first_order_profile_kernel(name, path):
    cols, s, tau, P0a, P0r = beam_handle(name)
    B, L = tau.shape
    wa, wr = C.profile_weights(name)
    ref = C.profile_first_order_model(name, path)
    d = [dev(x) for x in (tau, C.profile_sigma(name, path), P0a, P0r)]
    keep = set_weights(s, wa, wr)
    got = run_first_order(s, d, B, L)
    assert np.all(np.isfinite(got))
    worst = max(_err(got[b], ref[b]) for b in range(B))
    print("%s %s: first-order profile kernel vs model %.3e of the field maximum" % (name, path, worst))
    assert worst <= KERNEL_BAR
    assert np.array_equal(run_first_order(s, d, B, L), got)                  # the same call: the same bits
    assert np.array_equal(run_first_order(s, d, 1, L)[0], got[0])            # the first column alone: the same bits
    keep = set_weights(s, np.ones_like(wa), None)                            # unit weights: the beam kernel
    unit = run_first_order(s, d, B, L)
    keep = set_weights(s, None, None)
    beam = run_first_order(s, d, B, L, profile=False)
    e = max(_err(unit[b], beam[b]) for b in range(B))
    print("%s %s: unit weights vs sosrt_first_order_beam_dev %.3e (bit-equal: %s)" % (name, path, e, np.array_equal(unit, beam)))
    assert e <= UNIT_BAR
    del keep
    s.close()


def test_first_order_profile_kernel_with_a_p0_per_zone():
    """ZP0 = true at L = 1024: [B][5][2N] P0 of the aerosol, as the kernel takes it after sosrt_set_aerosol_sets on a zone table"""
    name = "profile-cap-L-2slabs"
    cols = C.beam_columns(name)
    N, L, B = C.SHAPES[name]
    mu = cols[0].mu
    s = Solver(L, N, max_batch=B, max_orders=1)
    s.set_grid(mu)
    s.set_phase_sets(O.phase_rayleigh(N, mu, 0.5)[1], np.stack([O.phase_hg(N, mu, 0.5, 0.7)[1], O.phase_hg(N, mu, 0.5, 0.3)[1]]))
    set_cols(s, cols)
    s.set_aerosol_sets(np.tile(np.array([0, 0, 0, 1, 0], dtype=np.int32), (B, 1)))
    tau = np.stack([c.tau for c in cols])
    d = [dev(x) for x in (tau, C.profile_sigma(name, "plane"), np.stack([c.P0_atm for c in cols]), C.profile_p0_zones(name))]
    keep = set_weights(s, *C.profile_weights(name))
    got, ref = run_first_order(s, d, B, L), C.profile_first_order_model(name, "plane", True)
    assert np.all(np.isfinite(got))
    worst = max(_err(got[b], ref[b]) for b in range(B))
    plain = max(_err(C.profile_first_order_model(name, "plane")[b], ref[b]) for b in range(B))
    print("%s, a P0 per zone: first-order profile kernel vs model %.3e (the model with one P0 is %.1e from it)" % (name, worst, plain))
    assert worst <= KERNEL_BAR and plain > 1e-3
    assert np.array_equal(run_first_order(s, d, B, L), got) and np.array_equal(run_first_order(s, d, 1, L)[0], got[0])
    del keep
    s.close()


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("name", C.PROFILE)
def test_emission_profile_kernel(name, surface):
    cols = C.thermal_columns(name, surface)
    pl, bs, es = C.thermal_sources(name)
    s, tau = thermal_handle(cols, phase=False, max_orders=1)
    B, L = tau.shape
    wa, wr = C.profile_weights(name, True)
    d = [dev(x) for x in (tau, pl, bs, es)]

    def run(explicit, B=B, profile=True):
        out = Guarded((B, L, s.D))
        sync()
        f = s.emission_profile_device if profile else s.emission_device
        f(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.ptr, d[3].data_ptr() if explicit else 0, B=B)
        return out.get(s)

    keep = set_weights(s, wa, wr)
    for explicit in (False, True):
        ref = C.profile_emission_model(name, surface, explicit)
        got = run(explicit)
        assert np.all(np.isfinite(got))
        worst = max(_err(got[b], ref[b]) for b in range(B))
        print("%s %s emissivity %s: emission profile kernel vs model %.3e of the field maximum" % (name, surface, "given" if explicit else "1 - rho", worst))
        assert worst <= KERNEL_BAR
    assert np.array_equal(run(True), got) and np.array_equal(run(True, B=1)[0], got[0])
    keep = set_weights(s, None, np.ones_like(wr))                            # unit weights: the emission kernel
    unit = run(False)
    keep = set_weights(s, None, None)
    plain = run(False, profile=False)
    e = max(_err(unit[b], plain[b]) for b in range(B))
    print("%s %s: unit weights vs sosrt_emission_dev %.3e (bit-equal: %s)" % (name, surface, e, np.array_equal(unit, plain)))
    assert e <= UNIT_BAR
    del keep
    s.close()


# ---- the limits ------------------------------------------------------------------------------------------------------------------------------
def test_profile_stage_refuses_L_1025():
    """One layer above kProfileMaxL = 1024 the handle exists and takes weights, and both entries of the profile stage refuse it
    with SOSRT_E_INVALID and a message that names 1024; the guarded outputs stay NaN.  (At L = 1024 the same calls are served: the
    profile-cap-L cases above.)"""
    L, N, B = 1025, 32, 2
    s = Solver(L, N, max_batch=B, max_orders=1)
    s.set_grid(O.make_mu(N))
    iu, idn = O.slab_indices(S.Z0, 25, 17, L)
    s.set_columns(np.full(B, iu), np.full(B, idn), [0.5, 0.6], 0.3, 1.0, 0.97, S.T_ATM / L, S.T_AER / (idn + 1 - iu), S.T_ATM + S.T_AER)
    tau = np.stack([O.tau_profile(S.T_ATM, S.T_AER, S.Z0, 25, 17, L)] * B)
    d_tau, d_sig, d_P0, d_bs = dev(tau), dev(tau / 0.5), dev(np.ones((B, 2 * N))), dev(np.ones(B))
    keep = set_weights(s, np.full((B, L), 0.5), None)
    out = Guarded((B, L, 2 * N))
    sync()
    t = d_tau.data_ptr()
    calls = {"sosrt_first_order_profile_dev": lambda: s.first_order_profile_device(t, d_sig.data_ptr(), d_P0.data_ptr(), d_P0.data_ptr(), out.ptr),
             "sosrt_emission_profile_dev": lambda: s.emission_profile_device(t, t, d_bs.data_ptr(), out.ptr)}
    for what, call in calls.items():
        with pytest.raises(ValueError) as ei:
            call()
        assert what in str(ei.value) and "1024" in str(ei.value), str(ei.value)
        assert np.all(np.isnan(out.get(s))), "%s: a refused call wrote to its output" % what
    del keep
    s.close()


def test_beam_and_emission_refuse_L_2049():
    """One layer above kBeamMaxL = kEmissionMaxL = 2048 the handle exists, and each of the four beam entries and of the three
    emission entries refuses it with SOSRT_E_INVALID and a message that names 2048, writing nothing.  (At L = 2048 the same
    calls are served: the cap-L cases above.)"""
    L, N, B, V = 2049, 32, 2, 3
    s = Solver(L, N, max_batch=B, max_orders=1)
    s.set_grid(O.make_mu(N))
    iu, idn = O.slab_indices(S.Z0, 25, 17, L)
    s.set_columns(np.full(B, iu), np.full(B, idn), [0.5, 0.6], 0.3, 1.0, 0.97, S.T_ATM / L, S.T_AER / (idn + 1 - iu), S.T_ATM + S.T_AER)
    tau = np.stack([O.tau_profile(S.T_ATM, S.T_AER, S.Z0, 25, 17, L)] * B)
    d_tau, d_z, d_sig = dev(tau), dev(S.altitudes(L)), dev(tau / 0.5)
    d_P0, d_I, d_bs, d_rows = dev(np.ones((B, 2 * N))), dev(np.ones((B, L, 2 * N))), dev(np.ones(B)), dev(np.ones((B, 2 * V)))
    o_row, o_field, o_view = Guarded((B, L), -7.0), Guarded((B, L, 2 * N), -7.0), Guarded((B, 2, 2 * V), -7.0)
    mv, lev = [0.2, 0.5, 1.0], [0, L - 1]
    sync()
    t, z, g, f = d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(), d_I.data_ptr()
    calls = {
        "sosrt_beam_slant_dev": lambda: s.beam_slant_device(t, z, o_row.ptr),
        "sosrt_first_order_beam_dev": lambda: s.first_order_beam_device(t, g, d_P0.data_ptr(), d_P0.data_ptr(), o_field.ptr),
        "sosrt_epilogue_beam_dev": lambda: s.epilogue_beam_device(t, f, g, z, "crit", o_row.ptr, d_heating_rate=o_row.ptr),
        "sosrt_view_first_order_beam_dev": lambda: s.view_first_order_beam_device(mv, t, g, d_rows.data_ptr(), d_rows.data_ptr(), lev, o_view.ptr),
        "sosrt_emission_dev": lambda: s.emission_device(t, t, d_bs.data_ptr(), o_field.ptr),
        "sosrt_emission_view_dev": lambda: s.emission_view_device(mv, t, t, d_bs.data_ptr(), lev, o_view.ptr),
        "sosrt_epilogue_emission_dev": lambda: s.epilogue_emission_device(t, f, z, o_row.ptr, d_heating_rate=o_row.ptr),
    }
    for what, call in calls.items():
        with pytest.raises(ValueError) as ei:
            call()
        assert what in str(ei.value) and "2048" in str(ei.value), str(ei.value)
        assert all(np.all(o.get(s) == -7.0) for o in (o_row, o_field, o_view)), "%s: a refused call wrote to an output" % what
    s.close()


def test_V_65_is_refused_and_V_64_served():
    """SOSRT_MAX_VIEWS = 64 view cosines are served by every entry that takes them, 65 refused with nothing written"""
    name = "floor"
    cols, s, tau, _, _ = beam_handle(name)
    B, L = tau.shape
    N = cols[0].N
    g = C.ground_case(name)
    rng = np.random.default_rng(65)
    ones = lambda *shape: dev(rng.uniform(0.5, 1.0, shape))
    d_tau, d_sig, d_I, d_bs, d_w = dev(tau), dev(C.beam_model(name)[0]), dev(g["I"]), dev(np.ones(B)), dev(g["weight"])
    lev = [0, L - 1]
    for V, served in ((65, False), (64, True)):
        mv = np.linspace(0.01, 1.0, V)
        d_rows, d_p0, d_Rv, d_r0v = ones(2 * V, 2 * N), ones(B, 2 * V), ones(3, N - 1, V), ones(3, B, V)
        outs = [Guarded((B, 2, 2 * V), -7.0) for _ in range(6)]
        sync()
        t = d_tau.data_ptr()
        calls = [
            lambda: s.view_radiance_device(mv, t, d_I.data_ptr(), d_rows.data_ptr(), d_rows.data_ptr(), lev, d_scat_out=outs[0].ptr,
                                           d_first_out=outs[1].ptr, d_p0rows_atm=d_p0.data_ptr(), d_p0rows_aer=d_p0.data_ptr()),
            lambda: s.emission_view_device(mv, t, t, d_bs.data_ptr(), lev, outs[2].ptr),
            lambda: s.view_first_order_beam_device(mv, t, d_sig.data_ptr(), d_p0.data_ptr(), d_p0.data_ptr(), lev, outs[3].ptr),
            lambda: s.view_ground_device(mv, t, lev, outs[4].ptr, d_I=d_I.data_ptr(), d_Rv=d_Rv.data_ptr(), d_r0v=d_r0v.data_ptr()),
            lambda: s.view_ground_terms_device(3, mv, t, lev, d_w.data_ptr(), outs[5].ptr, d_I=d_I.data_ptr(), d_Rv=d_Rv.data_ptr(),
                                               d_r0v=d_r0v.data_ptr()),
        ]
        for call in calls:
            if served:
                call()
            else:
                with pytest.raises(ValueError) as ei:
                    call()
                assert "V=65" in str(ei.value) and "64" in str(ei.value), str(ei.value)
        for o in outs:
            a = o.get(s)
            assert (not np.any(a == -7.0) and np.all(np.isfinite(a))) if served else np.all(a == -7.0)
    s.close()


# ---- the handle's view scratch ---------------------------------------------------------------------------------------------------------------
def test_view_scratch_grows_and_shrinks_with_the_call():
    """sosrt_view_radiance_dev reserves its scratch (the folded rows, the source at the lanes) per call from V and B.  On one
    handle: V = 5, then 64, then 5 again -- and 6 levels, then 300, then 6 again -- give the third result the bits of the first,
    and the handle's solve afterwards has the bits of a fresh handle's."""
    N, L, B, g_ = 33, 24, 3, 0.7
    cols = off_grid_columns(N, L, B)
    s, tau, P0a, P0r = three_zone_solver(cols, g_)
    fresh = s.solve(tau, P0a, P0r)
    s.close()
    s, _, _, _ = three_zone_solver(cols, g_)
    rng = np.random.default_rng(3)
    src = dev(rng.uniform(0.1, 1.0, (B, L, 2 * N)) * np.exp(-np.linspace(0, 2, L))[None, :, None])
    d_tau = dev(tau)
    mu0 = [c.mu0 for c in cols]

    def call(V, levels):
        mv = np.linspace(0.01, 1.0, V)
        sgn = VN.signed(mv)
        rows = np.random.default_rng(V)
        d = dict(tau=d_tau, src=src, rows_atm=dev(rows.uniform(0.5, 2.0, (2 * V, 2 * N))), rows_aer=dev(rows.uniform(0.1, 4.0, (2 * V, 2 * N))),
                 p0a=dev(VN.phase_p0_rows(C.FN_ATM, cols[0].mu, mu0, sgn)), p0r=dev(VN.phase_p0_rows(C.FN_AER, cols[0].mu, mu0, sgn)))
        return [run_view(s, mv, d, levels, quad, B) for quad in ("grid", "linear")]

    def same(a, b):
        return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))

    few, many = [0, L - 1, 7, 3, 12, 7], C.levels_300(L)
    first = call(5, few)
    wide = call(64, few)
    assert same(call(5, few), first)
    long_ = call(5, many)
    assert same(call(5, few), first)
    assert all(np.all(np.isfinite(x)) for p in wide + long_ for x in p)
    after = s.solve(tau, P0a, P0r)
    assert np.array_equal(after.I, fresh.I) and np.array_equal(after.n, fresh.n) and np.array_equal(after.status, fresh.status)
    s.close()
