"""The BRDF builders on the device (csrc/brdf.hip: k_brdf_pairs<NM, KIND>, k_brdf_view_beam_azimuth) through the seven entries of
the C ABI, for every kind, at the shapes the product ships at and at the limits the header promises (tests/brdf_builder_cases.py:
N = 4, 128, 501, 1024 and B = 70; nphi = 3, 256, 257 and 65537; up to 65 modes in nine launches; V = 1, 33, 64; 361 x 70 x 64
exact azimuths), each against the NumPy model of its kind in the ROW-WISE measure of the cases module -- per exit direction, the
largest error over that direction's largest stored value -- with the suite's measure 'of the array's maximum' printed beside it.
The bound is the suite's bar for a builder against its model, 1e-12.  Every output lies between two guards of NaN, is
prefilled with NaN and must come back finite.

What each test reaches that no other test of the suite does:

    test_builders_against_the_model   the pair flattening idx -> (second, first) over up to 1 046 529 pairs (4089 blocks, one live
                                      lane in the last) and over 9 pairs in one block; flux_weight at M = 3; the node loop with
                                      exactly one chunk, a second chunk of one node and 257 chunks; mode_cos with m q up to 4.2e6;
                                      nine launches with the output offset m * n at N = 128; (q, b, v) flattened over 1.6e6 lanes.
                                      At N >= 501 the model is evaluated on 18 rows; the rest of the array is held by the
                                      operator's reciprocity, R^m[i, j] / (2 w_j |mu_j|) against its transpose on the WHOLE array,
                                      and by the view-rows entry at the grid's nodes, 64 per call, bit for bit on every row whose
                                      cosine the entry accepts (>= 0.01: all but the first 4 of 500, the first 10 of 1023, which
                                      the sample holds).
    test_bit_guarantees               the builders' bit guarantees (tests/test_gpu_cox_munk.py) at these shapes, one kind per case
    test_lambertian_at_the_chunk_edges
                                      the Lambertian modes m >= 1 at nphi = 257 and 65537; -0 under sign_odd
    test_driver_at_the_benchmark_direction_count
                                      SOS_Aer_batch(surface='brdf') at (L, N, B) = (64, 128, 2) for RPV, Ross-Li and Cox-Munk
                                      against the model's series on the oracle

Measured figures: profiles/brdf_builder_shapes_errors.txt."""
import numpy as np
import pytest

import brdf_builder_cases as K
import brdf_np as G
from sosrt.main import SOS_Aer_batch
from test_gpu_brdf import dev, params_of, sync
from test_gpu_brdf_view import grid_handle
from test_gpu_stage_shapes import Guarded
from util import RTOL

pytestmark = pytest.mark.gpu


# ---- the seven entries, each output between guards, in the layout of its model ---------------------------------------------------------
def finite(a, what):
    assert np.all(np.isfinite(a)), "%s: the call left NaN in its output" % what
    return a


def run_operator(s, brdf, nphi):
    M = s.N - 1
    out = Guarded((M, M))
    sync()
    kind, p = params_of(brdf)
    s.brdf_operator_device(kind, out.ptr, p, nphi)
    return finite(out.get(s), "operator").T                                     # [i, j]


def run_beam(s, brdf, mu0, nphi):
    d_mu0, out = dev(mu0), Guarded((len(mu0), s.N - 1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_beam_device(kind, d_mu0.data_ptr(), out.ptr, p, nphi, B=len(mu0))
    return finite(out.get(s), "beam rows")                                      # [b, i]


def run_operator_modes(s, brdf, m_first, m_count, nphi, sign_odd=False):
    M = s.N - 1
    out = Guarded((m_count, M, M))
    sync()
    kind, p = params_of(brdf)
    s.brdf_operator_modes_device(kind, out.ptr, m_first, m_count, p, nphi, sign_odd=sign_odd)
    return np.swapaxes(finite(out.get(s), "operator modes"), 1, 2)              # [m, i, j]


def run_beam_modes(s, brdf, mu0, m_first, m_count, nphi):
    d_mu0, out = dev(mu0), Guarded((m_count, len(mu0), s.N - 1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_beam_modes_device(kind, d_mu0.data_ptr(), out.ptr, m_first, m_count, p, nphi, B=len(mu0))
    return finite(out.get(s), "beam modes")                                     # [m, b, i]


def run_view_rows(s, brdf, mv, m_first, m_count, nphi, sign_odd=False):
    out = Guarded((m_count, s.N - 1, len(mv)))
    sync()
    kind, p = params_of(brdf)
    s.brdf_view_rows_modes_device(kind, mv, out.ptr, m_first, m_count, p, nphi, sign_odd=sign_odd)
    return np.swapaxes(finite(out.get(s), "view rows"), 1, 2)                   # [m, v, j]


def run_view_beam(s, brdf, mu0, mv, m_first, m_count, nphi):
    d_mu0, out = dev(mu0), Guarded((m_count, len(mu0), len(mv)))
    sync()
    kind, p = params_of(brdf)
    s.brdf_view_beam_modes_device(kind, d_mu0.data_ptr(), mv, out.ptr, m_first, m_count, p, nphi, B=len(mu0))
    return finite(out.get(s), "view beam rows")                                 # [m, b, v]


def run_view_azimuth(s, brdf, mu0, mv, phi):
    d_mu0, d_phi, out = dev(mu0), dev(phi), Guarded((len(phi), len(mu0), len(mv)))
    sync()
    kind, p = params_of(brdf)
    s.brdf_view_beam_azimuth_device(kind, d_mu0.data_ptr(), mv, d_phi.data_ptr(), len(phi), out.ptr, p, B=len(mu0))
    return finite(out.get(s), "exact azimuth")                                  # [q, b, v]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. every entry against the model, row-wise --------------------------------------------------------------------------------------------
def reciprocity(R, wj):
    """(row-wise asymmetry, its row) of S[m, i, k] = R^m[i, N-2-k] / (2 w |mu|)_{N-2-k} = rho^m(c_i, c_k), c the nodes' cosines"""
    S = (R / wj[None, None, :])[:, :, ::-1]
    e = np.max(np.abs(S - np.swapaxes(S, 1, 2)), axis=(0, 2))
    d = np.max(np.abs(S), axis=(0, 2))
    return float(np.max(e / d)), int(np.argmax(e / d))


def model_asymmetry(name, nphi, kind):
    """the same of the model on the sampled rows: its rows against operator_columns_ref, their transposed partners"""
    N = K.SHAPES[name][0]
    rows, Rref = K.operator_ref(name, nphi, kind)
    wj = K.grid(N)[2]
    S = (Rref / wj[None, None, :])[:, :, ::-1]                                                   # [m, rows, k]
    cols = N - 2 - rows
    St = np.swapaxes(K.operator_columns_ref(name, nphi, kind) / wj[cols][None, None, :], 1, 2)   # [m, rows, k] = rho^m(c_k, c_row)
    return float(np.max(np.max(np.abs(S - St), axis=(0, 2)) / np.max(np.abs(S), axis=(0, 2))))


@pytest.mark.parametrize("kind", list(K.KINDS))
@pytest.mark.parametrize("plan", K.PLANS, ids=K.PLAN_IDS)
def test_builders_against_the_model(plan, kind):
    """Every entry of one (shape, nphi) for one kind: each call of the plan through the four mode entries (V = 1, 33, 64), the two
    azimuth-mean entries beside the call that holds mode 0, the exact-azimuth entry; at N >= 501 the whole operator's reciprocity
    and the view-rows entry at the nodes.  Every figure is printed, then all are asserted.

    With one running sum per lane over the azimuth nodes (the kernel before this test) the cases [floor-nphi65537-*] fail for
    every kind but the Lambertian: mode 0 on 65537 nodes 1.25e-12 row-wise and 1.16e-12 of the array's maximum (RPV operator), up to
    1.45e-12 (Cox-Munk view beam rows); with the sum in blocks of 4096 nodes <= 1.0e-13."""
    name, nphi, calls = plan
    N, B = K.SHAPES[name]
    brdf, mu0, ms = K.KINDS[kind], K.suns(name), K.plan_modes(name, nphi)
    s = grid_handle(N, B=B, L=K.L)
    rows, Rref = K.operator_ref(name, nphi, kind)
    r0ref = K.beam_ref(name, nphi, kind)
    wj = K.grid(N)[2]
    err = {}

    def compare(what, got, ref, axes, m0):
        ref0 = None if m0 == 0 else ref[1]
        err[what] = (K.rowwise(got, ref[0], axes, ref0), K.globalwise(got, ref[0]))
        print("%s %s nphi=%d %s: %.3e row-wise, %.3e of the array's maximum" % ((kind, name, nphi, what) + err[what]))

    for m0, mc in calls:
        tag = "modes %d..%d" % (m0, m0 + mc - 1)
        call = lambda ref: (K.pick(ref, ms, m0, mc), ref[:1])
        R = run_operator_modes(s, brdf, m0, mc, nphi)
        compare("operator %s" % tag, R[:, rows], call(Rref), 1, m0)
        r0 = run_beam_modes(s, brdf, mu0, m0, mc, nphi)
        compare("beam rows %s" % tag, r0, call(r0ref), 2, m0)
        for V in K.VIEWS:
            mv = K.view_mu(name, V)
            compare("view rows V=%d %s" % (V, tag), run_view_rows(s, brdf, mv, m0, mc, nphi), call(K.view_rows_ref(name, nphi, kind, V)), 1, m0)
            compare("view beam rows V=%d %s" % (V, tag), run_view_beam(s, brdf, mu0, mv, m0, mc, nphi),
                    call(K.view_beam_ref(name, nphi, kind, V)), 2, m0)
        if m0 == 0:                                          # the two azimuth-mean entries
            compare("operator mean", run_operator(s, brdf, nphi)[None, rows], (Rref[:1], None), 1, 0)
            compare("beam rows mean", run_beam(s, brdf, mu0, nphi)[None], (r0ref[:1], None), 2, 0)
        if N >= 501:
            # the rows no model looks at: reciprocity of the whole array, and the view-rows entry at every node, 64 per call
            asym_model = model_asymmetry(name, nphi, kind)
            asym, worst_row = reciprocity(R, wj)
            print("%s %s nphi=%d %s: reciprocity of the whole operator %.3e row-wise (row %d); the model's on the sampled rows %.3e"
                  % (kind, name, nphi, tag, asym, worst_row, asym_model))
            if asym_model <= 0.1 * K.KERNEL_BAR:
                err["reciprocity %s" % tag] = (asym, asym)
            up = K.grid(N)[0]
            served = np.flatnonzero(up >= 0.01)              # (the entry takes view cosines in [0.01, 1]: all nodes but the first 4 or 10)
            for n0 in range(0, len(served), 64):
                nodes = served[n0:n0 + 64]
                assert same_bits(run_view_rows(s, brdf, up[nodes], m0, mc, nphi), R[:, nodes]), "view rows at the nodes %d.. (%s)" % (n0, tag)
    for V in K.VIEWS:
        mv = K.view_mu(name, V)
        compare("exact azimuth V=%d" % V, run_view_azimuth(s, brdf, mu0, mv, K.PHI_AT), (K.azimuth_reference(name, kind, V), None), (1, 2), 0)
    if name == "many-columns":
        compare("exact azimuth V=64 at 361 azimuths", run_view_azimuth(s, brdf, mu0, K.view_mu(name, 64), K.PHI_MANY),
                (K.azimuth_reference(name, kind, 64, True), None), (1, 2), 0)
    s.close()
    bad = {k: v for k, v in err.items() if not v[0] <= K.KERNEL_BAR}
    assert not bad, bad


# ---- 2. the bit guarantees at these shapes ----------------------------------------------------------------------------------------------------
# one kind per case, every kind used
ROTATION = ["ross-thick-floor0", "rpv", "cox-munk-U2-shadow", "li-sparse", "ross-thick", "cox-munk-U10-noshadow", "li-sparse-floor0", "rpv",
            "lambertian"]


@pytest.mark.parametrize("plan,kind", list(zip(K.PLANS, ROTATION)), ids=["%s-%s" % pk for pk in zip(K.PLAN_IDS, ROTATION)])
def test_bit_guarantees(plan, kind):
    """A repeated call has the same bits; mode 0 of the mode entries has the bits of the azimuth-mean entries; a mode's bits do
    not depend on m_first or m_count (at nphi = 65537: the single-mode calls 63 and 64 against the launch of eight 57..64; else
    the first and the last mode alone and a range that starts inside one launch and ends in the next); sign_odd is the exact
    negation of the odd modes; the last column of the beam call alone (column 69 of 70) has the same bits."""
    name, nphi, calls = plan
    N, B = K.SHAPES[name]
    brdf, mu0 = K.KINDS[kind], K.suns(name)
    mv = K.view_mu(name, 33)
    s = grid_handle(N, B=B, L=K.L)
    m0, mc = max(calls, key=lambda c: c[1])
    entries = {"operator": lambda a, n, **kw: run_operator_modes(s, brdf, a, n, nphi, **kw),
               "beam rows": lambda a, n: run_beam_modes(s, brdf, mu0, a, n, nphi),
               "view rows": lambda a, n, **kw: run_view_rows(s, brdf, mv, a, n, nphi, **kw),
               "view beam rows": lambda a, n: run_view_beam(s, brdf, mu0, mv, a, n, nphi)}
    whole = {k: f(m0, mc) for k, f in entries.items()}
    if (0, 1) in calls or m0 == 0:
        first = whole if m0 == 0 else {k: f(0, 1) for k, f in entries.items()}
        assert same_bits(first["operator"][0], run_operator(s, brdf, nphi)) and same_bits(first["beam rows"][0], run_beam(s, brdf, mu0, nphi))
    if len(calls) > 1:
        parts = [c for c in calls if c != (m0, mc) and m0 <= c[0] and c[0] + c[1] <= m0 + mc]
        assert parts
    else:
        parts = [(m0, 1), (m0 + mc - 1, 1)] + ([(m0 + 3, min(mc - 3, 9))] if mc > 4 else [])
    for k, f in entries.items():
        assert same_bits(f(m0, mc), whole[k]), "%s: a repeated call" % k
        for a, n in parts:
            assert same_bits(f(a, n), whole[k][a - m0:a - m0 + n]), "%s: modes %d..%d alone" % (k, a, a + n - 1)
    sgn = np.array([(-1.0) ** m for m in range(m0, m0 + mc)])[:, None, None]
    for k in ("operator", "view rows"):
        assert same_bits(entries[k](m0, mc, sign_odd=True), sgn * whole[k]), "%s: sign_odd" % k
    assert same_bits(run_beam_modes(s, brdf, mu0[B - 1:], m0, mc, nphi), whole["beam rows"][:, B - 1:])
    assert same_bits(run_view_beam(s, brdf, mu0[B - 1:], mv, m0, mc, nphi), whole["view beam rows"][:, B - 1:])
    s.close()


@pytest.mark.parametrize("nphi", [257, 65537])
def test_lambertian_at_the_chunk_edges(nphi):
    """The Lambertian modes m >= 1 stay below 1e-15 (tests/test_gpu_brdf_azimuth.py: test_lambertian_modes_on_the_device) with a
    second chunk of one node and with 257 chunks; under sign_odd an odd mode is the exact negation, -0 for +0 included."""
    N, B = K.SHAPES["floor"]
    s = grid_handle(N, B=B, L=K.L)
    mu0, mv = K.suns("floor"), K.view_mu("floor", 64)
    calls = [(0, 10)] if nphi == 257 else [(0, 1), (1, 1), (63, 1), (64, 1), (57, 8)]
    for m0, mc in calls:
        R, r0 = run_operator_modes(s, "lambertian", m0, mc, nphi), run_beam_modes(s, "lambertian", mu0, m0, mc, nphi)
        Rv, r0v = run_view_rows(s, "lambertian", mv, m0, mc, nphi), run_view_beam(s, "lambertian", mu0, mv, m0, mc, nphi)
        lo = 1 if m0 == 0 else 0
        level = max(float(np.max(np.abs(x[lo:]), initial=0.0)) for x in (R, r0, Rv, r0v))
        print("nphi=%d modes %d..%d: Lambertian modes m >= 1 at most %.2e" % (nphi, m0, m0 + mc - 1, level))
        assert level <= 1e-15
        if m0 == 0:
            assert same_bits(R[0], run_operator(s, "lambertian", nphi)) and np.max(np.abs(r0[0] - 1)) <= 1e-12
        sgn = np.array([(-1.0) ** m for m in range(m0, m0 + mc)])[:, None, None]
        assert same_bits(run_operator_modes(s, "lambertian", m0, mc, nphi, sign_odd=True), sgn * R)
        assert same_bits(run_view_rows(s, "lambertian", mv, m0, mc, nphi, sign_odd=True), sgn * Rv)
    s.close()


# ---- 3. the driver at the benchmark's direction count ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", list(K.DRIVER_GROUNDS))
def test_driver_at_the_benchmark_direction_count(ground):
    """SOS_Aer_batch(surface='brdf') at (L, N, B) = (64, 128, 2), mu0 = 0.6 and 0.85, against the model's series on the oracle as the
    small-shape driver tests compare it: equal bounces, equal status, the field within RTOL of each column's maximum.  A column for
    which the model's mu -> 0 search leaves the ground row (the reference's IndexError) must be COL_INDEXERROR on the device; on
    the CPU the model gives status 0 for every column of every ground here (bounces 4, 5 / 3, 3 / 4, 4)."""
    ref, bounces, ratio, status = K.driver_model(ground)
    cols = K.driver_columns()
    c = cols[0]
    r = SOS_Aer_batch(list(K.DRIVER_SUNS), 0.3, 1.0, tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=K.DRIVER_L, nb_angles=K.DRIVER_N,
                      P_atm=c.P_atm, P_aer=c.P_aer, P0_atm=np.stack([x.P0_atm for x in cols]), P0_aer=np.stack([x.P0_aer for x in cols]),
                      max_orders=64, surface="brdf", brdf=K.DRIVER_GROUNDS[ground], raise_on_error=False)
    err = [float(np.max(np.abs(r.I[b] - ref[b])) / np.max(np.abs(ref[b]))) for b in range(len(cols))]
    print("%s L=%d N=%d: bounces %s (model %s), status %s (model %s), field vs the model's series %s of the maximum, ratios %s"
          % (ground, K.DRIVER_L, K.DRIVER_N, r.bounces, bounces, r.status, status, ["%.2e" % e for e in err], r.bounce_ratio))
    assert np.all(np.isfinite(r.I))
    assert np.array_equal(r.bounces, bounces) and np.array_equal(r.status, status)
    assert (status == G.COL_OK).any()
    assert max(err) <= RTOL
    assert np.all(np.abs(r.bounce_ratio - ratio) <= 1e-6 * np.maximum(ratio, 1e-12))
