"""The cases of tests/test_gpu_phase_builder_bits.py, shared with tools/record_phase_builder_bits.py (which records their bits with
the parent commit's library): every entry of the C ABI that builds a phase table on the device (csrc/phase.hip through
csrc/api_phasefn.hip and csrc/api_view.hip), on the smallest shapes that reach every loop and every compiled bound of the builders.

A case is one entry at one N; run(name) calls it for every phase function, batch width, set of view lanes and set of modes the
entry takes, and returns one SHA-256 digest per phase function over all those outputs in order.  The digests are compared with
those the parent commit's library gave (tests/golden/phase_builder_bits.json), never with the code under test.

  N        32: D = 64, three of the builder's four waves only take part in the reduction; 33: D = 66, the last wave is partial;
           129: D = 258, two threads take a second element of the stride loop (one phase function only)
  mu0      [0.3, 0.6, 0.95], and its first column alone
  lanes    V2 = 1, 10 (with grid nodes, both mu = 0 nodes among them) and 128 (the most a call takes: the four edge cosines +-1 and
           +-0.01, then random ones)
  modes    (m_first, m_count, nphi): 4, 9 (fills the bound 9), 10, 18, 34 and 65 (fills kMaxModes + 1) accumulators; (0, 3, 25) where
           the entry takes mode 0, which it has from the 25-node builder; sign_odd both ways where the entry has it"""
import hashlib

import numpy as np

from sosrt import inputs

NS = (32, 33, 129)
ALL_KINDS = [("iso", 0.0), ("rayleigh", 0.0), ("hg", 0.7), ("table", 0.0)]
MU0 = np.array([0.3, 0.6, 0.95])
MODE_SETS = [(1, 3, 25), (1, 8, 25), (1, 9, 25), (5, 17, 41), (1, 33, 71), (1, 64, 131)]
MODE_SETS_0 = [(0, 3, 25)] + MODE_SETS
PHI = np.array([0.0, 0.3, np.pi / 2, np.pi, 4.0, -1.0])     # (the azimuths of test_gpu_view_azimuth.py: test_exact_p0_builder)


def kinds(N):
    return ALL_KINDS if N != 129 else [("hg", 0.7)]


def lanes(N):
    """The three sets of exit cosines."""
    mu = inputs.direction_grid(N)
    rng = np.random.default_rng(7)
    return [np.array([-0.01]),
            np.array([mu[N - 1], mu[N], mu[1], mu[N + 5], mu[2 * N - 2], -1.0, 1.0, 0.01, 0.37, -0.62]),
            np.concatenate(([-1.0, 1.0, 0.01, -0.01], rng.uniform(-1, 1, 124)))]


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _out(shape):
    """A device buffer of NaN: an element the builder leaves out fails the case."""
    torch = _torch()
    t = torch.full(tuple(shape), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _host(t, s):
    s.synchronize()
    return t.cpu().numpy()


# ---- the entries: generators of the outputs of one phase function ---------------------------------------------------------------
def matrix(s, kind, g):
    yield s.phase_matrix(kind, g)


def matrix_dev(s, kind, g):
    o = _out((s.D, s.D))
    s.phase_matrix_device(kind, o.data_ptr(), g)
    yield _host(o, s)


def p0(s, kind, g):
    for B in (3, 1):
        yield s.phase_p0(kind, MU0[:B], g)


def p0_dev(s, kind, g):
    for B in (3, 1):
        d_mu0, o = _dev(MU0[:B]), _out((B, s.D))
        s.phase_p0_device(kind, d_mu0.data_ptr(), o.data_ptr(), B, g)
        yield _host(o, s)


def modes(s, kind, g):
    for mf, mc, nphi in MODE_SETS_0:
        yield s.phase_modes(kind, mf, mc, nphi, g)


def modes_dev(s, kind, g):
    for mf, mc, nphi in MODE_SETS_0:
        for sign in (False, True):
            o = _out((mc, s.D, s.D))
            s.phase_modes_device(kind, o.data_ptr(), mf, mc, nphi, g, sign_odd=sign)
            yield _host(o, s)


def p0_modes(s, kind, g):
    for B in (3, 1):
        for mf, mc, nphi in MODE_SETS_0:
            yield s.phase_p0_modes(kind, MU0[:B], mf, mc, nphi, g)


def p0_modes_dev(s, kind, g):
    for B in (3, 1):
        d_mu0 = _dev(MU0[:B])
        for mf, mc, nphi in MODE_SETS_0:
            o = _out((mc, B, s.D))
            s.phase_p0_modes_device(kind, d_mu0.data_ptr(), o.data_ptr(), B, mf, mc, nphi, g)
            yield _host(o, s)


def rows_dev(s, kind, g):
    for sgn in lanes(s.N):
        o = _out((len(sgn), s.D))
        s.phase_rows_device(kind, sgn, o.data_ptr(), g)
        yield _host(o, s)


def p0_rows_dev(s, kind, g):
    for B in (3, 1):
        d_mu0 = _dev(MU0[:B])
        for sgn in lanes(s.N):
            o = _out((B, len(sgn)))
            s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, o.data_ptr(), B, g)
            yield _host(o, s)


def rows_modes_dev(s, kind, g):
    for sgn in lanes(s.N):
        for mf, mc, nphi in MODE_SETS:
            for sign in (False, True):
                o = _out((mc, len(sgn), s.D))
                s.phase_rows_modes_device(kind, sgn, o.data_ptr(), mf, mc, nphi, g, sign_odd=sign)
                yield _host(o, s)


def p0_rows_modes_dev(s, kind, g):
    for B in (3, 1):
        d_mu0 = _dev(MU0[:B])
        for sgn in lanes(s.N):
            for mf, mc, nphi in MODE_SETS:
                o = _out((mc, B, len(sgn)))
                s.phase_p0_rows_modes_device(kind, d_mu0.data_ptr(), sgn, o.data_ptr(), B, mf, mc, nphi, g)
                yield _host(o, s)


def p0_rows_azimuth_dev(s, kind, g):
    d_phi = _dev(PHI)
    for B in (3, 1):
        d_mu0 = _dev(MU0[:B])
        for sgn in lanes(s.N):
            o = _out((len(PHI), B, len(sgn)))
            s.phase_p0_rows_azimuth_device(kind, d_mu0.data_ptr(), sgn, d_phi.data_ptr(), len(PHI), o.data_ptr(), B, g)
            yield _host(o, s)


ENTRIES = {"phase_matrix": matrix, "phase_matrix_dev": matrix_dev, "phase_p0": p0, "phase_p0_dev": p0_dev, "phase_modes": modes,
           "phase_modes_dev": modes_dev, "phase_p0_modes": p0_modes, "phase_p0_modes_dev": p0_modes_dev, "phase_rows_dev": rows_dev,
           "phase_p0_rows_dev": p0_rows_dev, "phase_rows_modes_dev": rows_modes_dev, "phase_p0_rows_modes_dev": p0_rows_modes_dev,
           "phase_p0_rows_azimuth_dev": p0_rows_azimuth_dev}
CASES = {"%s_N%d" % (e, N): (e, N) for e in ENTRIES for N in NS}


def run(name):
    """{phase function: digest of the case's outputs for it, in order}"""
    from sosrt.solver import Solver
    entry, N = CASES[name]
    s = Solver(4, N, max_batch=3)
    try:
        s.set_grid(inputs.direction_grid(N))
        s.set_phase_table(*inputs.fwc_table())
        digests = {}
        for kind, g in kinds(N):
            h, n = hashlib.sha256(), 0
            for a in ENTRIES[entry](s, kind, g):
                a = np.ascontiguousarray(a)
                assert a.dtype == np.float64 and not np.isnan(a).any(), (name, kind, n)
                h.update(str(a.shape).encode() + a.tobytes())
                n += 1
            digests[kind] = h.hexdigest()
    finally:
        s.close()
    return digests
