"""The phase builders (csrc/phase.hip, csrc/phasefn.hpp) and the azimuth synthesis (csrc/epilogue.hip) on the device, through the C
ABI, at the shapes the product ships at and at the limits the header promises (tests/phase_shape_cases.py: floor N = 4, headline
N = 128, many-columns B = 70 at N = 130, shipped-N 501, cap-N 1024), each entry against the NumPy model of the suite with the
measure and the bound of the small-shape tests -- the largest difference over the mode-0 maximum of the same phase function,
1e-12 -- for Rayleigh, HG(0.9), whose mode 64 is 1.4e-4 of mode 0, and the fwc table, whose mode 64 is 2e-3 of it.  At N = 501
and 1024 the model covers the 32 second directions of phase_shape_cases.columns and two identities cover the whole table.
Every output lies between two guards of NaN that must stay NaN.

What each test reaches that no other test of the suite does:

    test_matrix_entries          k_phase_pairs<COLUMN, NODES, K> against a model above N = 128: four and eight trips of the stride
                                 loops, the normaliser's sum over 1002 and 2048 exits; K = 65 and modes 34..64 against a model at
                                 all; m = 64 through K = 9 with m_first = 57, 63; the sum rule and reciprocity on whole tables
    test_p0_entries              k_phase_pairs<MU0, NODES, K> likewise; 70 columns of P0; mu0 = 1, where s = 0 and the odd modes
                                 are exact zeros; a column alone against the column in its batch
    test_row_entries             k_phase_pairs<COLUMN, LANES, K> with 128 lanes and with 65 accumulators against a model; rows at
                                 node lanes against the matrix entry bit for bit at N = 4, 128, 130, 501, 1024 and K = 9..65
    test_p0_row_entries          k_phase_pairs<MU0, LANES, K> with B = 70 x 128 lanes x 64 modes; k_phase_p0_azimuth's stride loop in
                                 24 trips (48 azimuths x 128 lanes)
    test_isotropic_at_floor      the constant branch of all nine entries at D = 8
    test_host_pointer_entries    the four host entries against their device entries at N = 501, the P0 ones at B = max_batch
    test_synthesis, test_synthesis_with_levels_outside, test_view_synthesis
                                 k_azimuth_accumulate, k_azimuth_synthesize and k_view_azimuth_accumulate against an independent
                                 long double sum: D = 2048, M = 64, 361 azimuths (2888 trips of the 256-thread stride loop), NaN
                                 rows at B = 70, 1225 and 1216 blocks of the view kernel
    test_refusals                mode 65 at N = 1024, nphi = m_last + 1, V2 = 129, M = 65: refused, nothing written

Figures of one run are in profiles/phase_shapes_errors.txt."""
import numpy as np
import pytest

import phase_shape_cases as C
from phase_builder_cases import PHI
from sosrt import inputs
from sosrt.solver import Solver
from test_gpu_spherical import dev, sync
from test_gpu_stage_shapes import Guarded

pytestmark = pytest.mark.gpu

CASES = [(name, kind, g) for name in C.SHAPES for kind, g in C.KINDS]
IDS = ["%s-%s" % c[:2] for c in CASES]


def solver(name):
    N, B = C.SHAPES[name]
    s = Solver(4, N, max_batch=B)
    s.set_grid(C.grid(name))
    s.set_phase_table(*inputs.fwc_table())
    return s


def run(s, shape, call, fill=np.nan):
    """The output [shape] of call(address), from between its guards"""
    out = Guarded(shape, fill)
    sync()
    call(out.ptr)
    return out.get(s)


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def worst(got, ref, scale):
    assert got.shape == ref.shape and not np.isnan(got).any()
    return float(np.max(np.abs(got - ref)) / scale)


def report(name, kind, entry, e, bar=C.BOUND):
    print("%-13s %-9s %-44s %.2e  (bar %.1e)" % (name, kind, entry, e, bar))
    assert e <= bar, "%s %s %s: %.3e > %.1e" % (name, kind, entry, e, bar)


def odd_of(mset):
    return (np.arange(mset[0], mset[0] + mset[1]) & 1).astype(bool)


def check_signs_and_zeros(kind, mset, plain, signed, what):
    """sign_odd flips exactly the odd modes; Rayleigh's modes m >= 3 are exact zeros"""
    odd = odd_of(mset)
    assert bits(signed[odd], -plain[odd]) and bits(signed[~odd], plain[~odd]), what + ": sign_odd"
    if kind == "rayleigh":
        z = np.arange(mset[0], mset[0] + mset[1]) >= 3
        assert not np.any(plain[z]) and not np.any(signed[z]), what + ": modes m >= 3 are exact zeros"
        assert mset[0] >= 3 or np.any(plain[~z])


def mset_name(mset):
    return "modes %d..%d on %d nodes" % (mset[0], mset[0] + mset[1] - 1, mset[2])


# ---- the matrix and its modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,g", CASES, ids=IDS)
def test_matrix_entries(name, kind, g):
    s = solver(name)
    D, mu, c = s.D, C.grid(name), C.columns(name)
    scale = C.scales(name, kind, g)[0]
    large = name in C.LARGE

    def identities(P, mset, what):
        rule, rec = C.identity_tolerances(name, kind, g, mset)
        if mset is None:
            report(name, kind, what + ": sum rule over all columns", float(np.max(np.abs(C._trapz(P[0], mu, axis=0) - 4))) / 4, rule)
        Z = C.normalisers(name, kind, g, C._nphi(mset))[0]
        report(name, kind, what + ": reciprocity, whole table", C.reciprocity(P, P, Z, Z, scale, float(np.max(Z))), rec)

    matrix = lambda p: s.phase_matrix_device(kind, p, g)
    P0 = run(s, (D, D), matrix)
    report(name, kind, "phase_matrix_device", worst(P0[:, c], C.matrix_model(name, kind, g, None)[0], scale))
    assert bits(run(s, (D, D), matrix), P0), "the same call twice"
    if large:
        identities(P0[None], None, "phase_matrix_device")
    for mset in C.MATRIX_SETS[name]:
        mf, mc, nphi = mset
        what = "phase_modes_device " + mset_name(mset)
        P = run(s, (mc, D, D), lambda p: s.phase_modes_device(kind, p, mf, mc, nphi, g))
        report(name, kind, what, worst(P[:, :, c], C.matrix_model(name, kind, g, mset), scale))
        check_signs_and_zeros(kind, mset, P, run(s, (mc, D, D), lambda p: s.phase_modes_device(kind, p, mf, mc, nphi, g, sign_odd=True)), what)
        if large:
            identities(P, mset, what)
    for nphi in (25, 131):                                   # mode 0 through the mode entry is the 25-node builder, whatever nphi
        P = run(s, (2, D, D), lambda p: s.phase_modes_device(kind, p, 0, 2, nphi, g))
        assert bits(P[0], P0), "mode 0 of phase_modes_device on %d nodes" % nphi
    s.close()


# ---- P0 and its modes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,g", CASES, ids=IDS)
def test_p0_entries(name, kind, g):
    s = solver(name)
    D, mu, mu0 = s.D, C.grid(name), C.suns(name)
    B = len(mu0)
    sp0 = C.scales(name, kind, g)[1]
    d_mu0 = dev(mu0)
    per_column = lambda got, ref: max(worst(got[..., b, :], ref[..., b, :], sp0[b]) for b in range(B))
    p0 = lambda B: (lambda p: s.phase_p0_device(kind, d_mu0.data_ptr(), p, B, g))
    P0 = run(s, (B, D), p0(B))
    report(name, kind, "phase_p0_device B=%d" % B, per_column(P0, C.p0_model(name, kind, g, None)[0]))
    assert bits(run(s, (B, D), p0(B)), P0), "the same call twice"
    assert bits(run(s, (1, D), p0(1)), P0[:1]), "the first column alone"
    if name in C.LARGE:
        rule = C.identity_tolerances(name, kind, g, None)[0]
        report(name, kind, "phase_p0_device: sum rule over all rows", float(np.max(np.abs(C._trapz(P0, mu, axis=1) - 2))) / 2, rule)
    for mset in C.SMALL_SETS:
        mf, mc, nphi = mset
        what = "phase_p0_modes_device " + mset_name(mset)
        modes = lambda B: (lambda p: s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p, B, mf, mc, nphi, g))
        P = run(s, (mc, B, D), modes(B))
        report(name, kind, what, per_column(P, C.p0_model(name, kind, g, mset)))
        assert bits(run(s, (mc, 1, D), modes(1)), P[:, :1]), what + ": the first column alone"
        assert mu0[0] == 1.0 and not np.any(P[odd_of(mset), 0]), what + ": mu0 = 1, the odd modes are exact zeros"
        if kind == "rayleigh":
            assert not np.any(P[np.arange(mf, mf + mc) >= 3])
    for nphi in (25, 131):
        P = run(s, (2, B, D), lambda p: s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p, B, 0, 2, nphi, g))
        assert bits(P[0], P0), "mode 0 of phase_p0_modes_device on %d nodes" % nphi
    s.close()


# ---- rows at view cosines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,g", CASES, ids=IDS)
def test_row_entries(name, kind, g):
    s = solver(name)
    D, c = s.D, C.columns(name)
    sr = C.scales(name, kind, g)[2]
    for V2 in C.V2S:
        sgn = C.lanes(name, V2)
        r0 = run(s, (V2, D), lambda p: s.phase_rows_device(kind, sgn, p, g))
        report(name, kind, "phase_rows_device V2=%d" % V2, worst(r0[:, c], C.rows_model(name, kind, g, None, V2)[0], sr[V2]))
        for mset in C.SMALL_SETS:
            mf, mc, nphi = mset
            what = "phase_rows_modes_device V2=%d %s" % (V2, mset_name(mset))
            rows = lambda sign: (lambda p: s.phase_rows_modes_device(kind, sgn, p, mf, mc, nphi, g, sign_odd=sign))
            r = run(s, (mc, V2, D), rows(False))
            report(name, kind, what, worst(r[:, :, c], C.rows_model(name, kind, g, mset, V2), sr[V2]))
            check_signs_and_zeros(kind, mset, r, run(s, (mc, V2, D), rows(True)), what)
    # at node lanes: the rows of the matrix entries, bit for bit, at every compiled bound of the accumulators
    k, sgn = C.node_lanes(name), C.lanes(name, 128)
    assert bits(r0[:len(k)], run(s, (D, D), lambda p: s.phase_matrix_device(kind, p, g))[k]), "rows at node lanes, mode 0"
    for mf, mc, nphi in (C.MATRIX_SETS[name] if name in C.LARGE else C.NODE_K_SETS):
        P = run(s, (mc, D, D), lambda p: s.phase_modes_device(kind, p, mf, mc, nphi, g))
        r = run(s, (mc, 128, D), lambda p: s.phase_rows_modes_device(kind, sgn, p, mf, mc, nphi, g))
        assert bits(r[:, :len(k)], P[:, k]), "rows at node lanes, " + mset_name((mf, mc, nphi))
    s.close()


@pytest.mark.parametrize("name,kind,g", CASES, ids=IDS)
def test_p0_row_entries(name, kind, g):
    s = solver(name)
    mu0 = C.suns(name)
    B = len(mu0)
    spr = C.scales(name, kind, g)[3]
    d_mu0 = dev(mu0)
    for V2 in C.V2S:
        sgn = C.lanes(name, V2)
        rows = lambda B: (lambda p: s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p, B, g))
        r0 = run(s, (B, V2), rows(B))
        report(name, kind, "phase_p0_rows_device V2=%d" % V2, worst(r0, C.p0_rows_model(name, kind, g, None, V2)[0], spr[V2]))
        assert bits(run(s, (1, V2), rows(1)), r0[:1]) and bits(run(s, (B, V2), rows(B)), r0), "the first column alone; the call twice"
        for mset in C.SMALL_SETS:
            mf, mc, nphi = mset
            what = "phase_p0_rows_modes_device V2=%d %s" % (V2, mset_name(mset))
            modes = lambda B: (lambda p: s.phase_p0_rows_modes_device(kind, d_mu0.data_ptr(), sgn, p, B, mf, mc, nphi, g))
            r = run(s, (mc, B, V2), modes(B))
            report(name, kind, what, worst(r, C.p0_rows_model(name, kind, g, mset, V2), spr[V2]))
            assert bits(run(s, (mc, 1, V2), modes(1)), r[:, :1]), what + ": the first column alone"
            assert not np.any(r[odd_of(mset), 0]), what + ": mu0 = 1, the odd modes are exact zeros"
            if kind == "rayleigh":
                assert not np.any(r[np.arange(mf, mf + mc) >= 3])
        for phi in (PHI, C.PHI48):
            d_phi, n = dev(phi), len(phi)
            what = "phase_p0_rows_azimuth_device V2=%d, %d azimuths" % (V2, n)
            point = lambda B: (lambda p: s.phase_p0_rows_azimuth_device(kind, d_mu0.data_ptr(), sgn, d_phi.data_ptr(), n, p, B, g))
            got, ref = run(s, (n, B, V2), point(B)), C.p0_azimuth_reference(name, kind, g, V2, n)
            assert not np.isnan(got).any()
            report(name, kind, what + " (element-wise)", float(np.max(np.abs(got - ref) / np.abs(ref))))
            assert bits(run(s, (n, 1, V2), point(1)), got[:, :1]), what + ": the first column alone"
    s.close()


def test_isotropic_at_floor():
    """Constants and exact zeros from all nine entries"""
    name = "floor"
    s = solver(name)
    D, mu0, sgn = s.D, C.suns(name), C.lanes(name, 128)
    B = len(mu0)
    d_mu0, d_phi = dev(mu0), dev(C.PHI48)
    mf, mc, nphi = C.FULL
    assert np.all(run(s, (D, D), lambda p: s.phase_matrix_device("iso", p)) == 2.0)
    assert np.all(run(s, (B, D), lambda p: s.phase_p0_device("iso", d_mu0.data_ptr(), p, B)) == 1.0)
    assert np.all(run(s, (128, D), lambda p: s.phase_rows_device("iso", sgn, p)) == 2.0)
    assert np.all(run(s, (B, 128), lambda p: s.phase_p0_rows_device("iso", d_mu0.data_ptr(), sgn, p, B)) == 1.0)
    assert np.all(run(s, (48, B, 128), lambda p: s.phase_p0_rows_azimuth_device("iso", d_mu0.data_ptr(), sgn, d_phi.data_ptr(), 48, p, B)) == 1.0)
    for sign in (False, True):
        zeros = [run(s, (mc, D, D), lambda p: s.phase_modes_device("iso", p, mf, mc, nphi, sign_odd=sign)),
                 run(s, (mc, 128, D), lambda p: s.phase_rows_modes_device("iso", sgn, p, mf, mc, nphi, sign_odd=sign))]
        if not sign:
            zeros += [run(s, (mc, B, D), lambda p: s.phase_p0_modes_device("iso", d_mu0.data_ptr(), p, B, mf, mc, nphi)),
                      run(s, (mc, B, 128), lambda p: s.phase_p0_rows_modes_device("iso", d_mu0.data_ptr(), sgn, p, B, mf, mc, nphi))]
        for z in zeros:
            assert not np.isnan(z).any() and not np.any(z)
    s.close()


def test_host_pointer_entries():
    """phase_matrix, phase_p0, phase_modes and phase_p0_modes give the bits of their device entries at N = 501, the P0 ones at
    B = max_batch"""
    name, kind, g = "shipped-N", "hg", 0.9
    s = solver(name)
    D, mu0 = s.D, C.suns(name)
    B = len(mu0)
    assert B == s.max_batch
    d_mu0 = dev(mu0)
    assert bits(s.phase_matrix(kind, g), run(s, (D, D), lambda p: s.phase_matrix_device(kind, p, g)))
    assert bits(s.phase_p0(kind, mu0, g), run(s, (B, D), lambda p: s.phase_p0_device(kind, d_mu0.data_ptr(), p, B, g)))
    mf, mc, nphi = C.MATRIX_SETS[name][1]
    assert bits(s.phase_modes(kind, mf, mc, nphi, g), run(s, (mc, D, D), lambda p: s.phase_modes_device(kind, p, mf, mc, nphi, g)))
    for mf, mc, nphi in [(0, 3, 25)] + C.SMALL_SETS:
        assert bits(s.phase_p0_modes(kind, mu0, mf, mc, nphi, g),
                    run(s, (mc, B, D), lambda p: s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p, B, mf, mc, nphi, g)))
    s.close()


# ---- the synthesis ----------------------------------------------------------------------------------------------------------------------
def azimuths(n):
    return np.array([0.7]) if n == 1 else np.linspace(-1.0, 7.0, n)


def synthesize_both(s, I, levels, phi, B):
    """(the sequence of accumulate launches in ascending m, the one launch), each [B, nlev, D, nphi] from between guards"""
    M, D = I.shape[0] - 1, I.shape[-1]
    d_I, d_lev, d_phi = dev(I), dev(levels, np.int32), dev(phi)
    nlev, n = len(levels), len(phi)
    seq, one = Guarded((B, nlev, D, n), 5.0), Guarded((B, nlev, D, n), 6.0)
    sync()
    for m in range(M + 1):
        s.azimuth_accumulate_device(m, d_I[m].data_ptr(), d_lev.data_ptr(), nlev, d_phi.data_ptr(), n, seq.ptr, B=B)
    s.azimuth_synthesize_device(M, d_I[0].data_ptr(), d_I[1:].data_ptr() if M else 0, d_lev.data_ptr(), nlev, d_phi.data_ptr(), n, one.ptr, B=B)
    return seq.get(s), one.get(s)


def against_the_sum(what, got, vals, phi, M):
    ref, mag = C.synthesis_reference(vals, phi)
    e = float(np.max(np.abs(got - ref) / mag))
    print("%-60s %.2e of the terms' magnitudes (bar (M + 4) 2^-53 = %.2e)" % (what, e, C.synthesis_bar(M)))
    assert e <= C.synthesis_bar(M), what


@pytest.mark.parametrize("M", [0, 1, 64])
@pytest.mark.parametrize("nphi_out", [1, 7, 361])
def test_synthesis(nphi_out, M):
    N, L, B, levels = 1024, 24, 2, [0, 23, 7]
    s = Solver(L, N, max_batch=B)
    s.set_grid(inputs.direction_grid(N))
    I = C.synthesis_fields((B, L, 2 * N), M, 100 + M)
    phi = azimuths(nphi_out)
    seq, one = synthesize_both(s, I, levels, phi, B)
    s.close()
    assert not np.isnan(seq).any() and bits(seq, one), "the one launch is the sequence of launches"
    against_the_sum("synthesis N=1024 M=%d, %d azimuths" % (M, nphi_out), one, I[:, :, levels], phi, M)


@pytest.mark.parametrize("M", [0, 64])
def test_synthesis_with_levels_outside(M):
    """Levels -1 and L among four at B = 70: their rows are NaN in every column, the other rows are the sum"""
    N, L, B, levels = 130, 4, 70, [-1, 2, 4, 0]
    s = Solver(L, N, max_batch=B)
    s.set_grid(inputs.direction_grid(N))
    I = C.synthesis_fields((B, L, 2 * N), M, 200 + M)
    phi = azimuths(7)
    seq, one = synthesize_both(s, I, levels, phi, B)
    s.close()
    assert np.array_equal(seq, one, equal_nan=True) and bits(seq[:, [1, 3]], one[:, [1, 3]]), "the one launch is the sequence of launches"
    for got in (seq, one):
        assert np.isnan(got[:, [0, 2]]).all() and not np.isnan(got[:, [1, 3]]).any()
    against_the_sum("synthesis N=130 B=70 M=%d, levels outside" % M, one[:, [1, 3]], I[:, :, [2, 0]], phi, M)


@pytest.mark.parametrize("B,nlev,V2,nphi_out", [(70, 5, 128, 7), (70, 5, 127, 7), (1, 1, 1, 1)])
def test_view_synthesis(B, nlev, V2, nphi_out):
    """Modes 0..64 at the view lanes: 313600 elements are 1225 full blocks, 311150 are 1215 and a partial one, 1 is one lane"""
    M = 64
    s = Solver(4, 8, max_batch=B)
    vals = C.synthesis_fields((B, nlev, V2), M, 300 + V2)
    phi = azimuths(nphi_out)
    d_vals, d_phi = dev(vals), dev(phi)
    out = Guarded((B, nlev, V2, nphi_out), 5.0)
    sync()
    for m in range(M + 1):
        s.view_azimuth_accumulate_device(m, d_vals[m].data_ptr(), nlev, V2, d_phi.data_ptr(), nphi_out, out.ptr, B=B)
    got = out.get(s)
    s.close()
    assert not np.isnan(got).any()
    against_the_sum("view synthesis (B, nlev, V2, nphi) = (%d, %d, %d, %d) M=64" % (B, nlev, V2, nphi_out), got, vals, phi, M)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Each refused before a launch: the outputs, sized for the call had it been served, keep their fill"""
    name, kind, g = "cap-N", "hg", 0.9
    s = solver(name)
    D, mu0 = s.D, C.suns(name)
    B = len(mu0)
    d_mu0, d_phi = dev(mu0), dev(PHI)
    sgn, too_many = C.lanes(name, 128), np.linspace(-1, 1, 129)

    def refused(what, shape, call):
        out = Guarded(shape, -7.0)
        sync()
        with pytest.raises(ValueError):
            call(out.ptr)
        assert np.all(out.get(s) == -7.0), what + ": the output was written"

    for what, (mf, mc, nphi) in (("mode 65", (64, 2, 131)), ("nphi = m_last + 1", (1, 3, 4))):
        refused("phase_modes_device, " + what, (mc, D, D), lambda p: s.phase_modes_device(kind, p, mf, mc, nphi, g))
        refused("phase_p0_modes_device, " + what, (mc, B, D), lambda p: s.phase_p0_modes_device(kind, d_mu0.data_ptr(), p, B, mf, mc, nphi, g))
        refused("phase_rows_modes_device, " + what, (mc, 128, D), lambda p: s.phase_rows_modes_device(kind, sgn, p, mf, mc, nphi, g))
        refused("phase_p0_rows_modes_device, " + what, (mc, B, 128), lambda p: s.phase_p0_rows_modes_device(kind, d_mu0.data_ptr(), sgn, p, B, mf, mc, nphi, g))
    refused("phase_rows_device, V2 = 129", (129, D), lambda p: s.phase_rows_device(kind, too_many, p, g))
    refused("phase_p0_rows_device, V2 = 129", (B, 129), lambda p: s.phase_p0_rows_device(kind, d_mu0.data_ptr(), too_many, p, B, g))
    refused("phase_rows_modes_device, V2 = 129", (3, 129, D), lambda p: s.phase_rows_modes_device(kind, too_many, p, 1, 3, 25, g))
    refused("phase_p0_rows_modes_device, V2 = 129", (3, B, 129), lambda p: s.phase_p0_rows_modes_device(kind, d_mu0.data_ptr(), too_many, p, B, 1, 3, 25, g))
    refused("phase_p0_rows_azimuth_device, V2 = 129", (len(PHI), B, 129),
            lambda p: s.phase_p0_rows_azimuth_device(kind, d_mu0.data_ptr(), too_many, d_phi.data_ptr(), len(PHI), p, B, g))
    # the synthesis: M = 65 modes behind mode 0, mode 65 at the view lanes
    L = 4
    d_I, d_lev = dev(C.synthesis_fields((B, L, D), 65, 1)), dev([0, 3], np.int32)
    refused("azimuth_synthesize_device, M = 65", (B, 2, D, len(PHI)),
            lambda p: s.azimuth_synthesize_device(65, d_I[0].data_ptr(), d_I[1:].data_ptr(), d_lev.data_ptr(), 2, d_phi.data_ptr(), len(PHI), p, B=B))
    d_val = dev(np.ones((B, 2, 129)))
    refused("view_azimuth_accumulate_device, mode 65", (B, 2, 128, len(PHI)),
            lambda p: s.view_azimuth_accumulate_device(65, d_val.data_ptr(), 2, 128, d_phi.data_ptr(), len(PHI), p, B=B))
    refused("view_azimuth_accumulate_device, V2 = 129", (B, 2, 129, len(PHI)),
            lambda p: s.view_azimuth_accumulate_device(1, d_val.data_ptr(), 2, 129, d_phi.data_ptr(), len(PHI), p, B=B))
    s.close()
