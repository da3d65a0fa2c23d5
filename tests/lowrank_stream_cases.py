"""The cases of tests/test_gpu_lowrank_stream.py, shared with tools/record_lowrank_bits.py (which records their bits with the
parent commit's library): fixed seeds, the atmospheres of tests/legendre_phase.py at every rank 0 .. 4 plus Rayleigh.

A case returns SHA-256 digests of what the library computed; the recorded digests come from the parent, never from the code under
test (tests/golden/lowrank_stream_bits.json)."""
import functools
import hashlib

import numpy as np

import legendre_phase as LP
import sos_oracle as O
from sosrt import inputs

ATMOSPHERES = ("zero", "r1", "r2", "r3", "r4", "rayleigh")

# Solver.source over (L, N, B, first slab row, last slab row).  The dense launch deals the plain rows over the resident workgroups
# in runs of whole batches of 4 rows per wave (csrc/kernels.hpp: lr_stream_run; two rounds of the 1024 workgroups resident on an
# MI355X), so the batches a wave gets follow from the count of plain rows P = B (L - slab rows):
#   P <= 32768: runs of 16 rows, one batch a wave, waves (and with P = 8 whole quarters of the workgroup) without a row;
#     B = 301 (P = 20769): the last workgroup has one row -- a batch of 1;
#   B = 602 (P = 41538): runs of 32, two batches a wave, the last workgroup 2 rows -- a batch of 2;
#   B = 1003 (P = 69207): runs of 48, three batches (the pipeline's two register sets both reused), the last workgroup 39 rows
#     -- three waves of 12 and a wave of 3.
# Widths: D = 8 and 74 (< 128: lanes with nothing to do), 200 (D % 128 != 0), 256 (the headline: one unit a row), 512 (two units a
# row), 1002 (four, ragged; at ranks 3 and 4 the factors do not fit the stream's LDS and the rows go batch by batch).
SOURCE_SHAPES = {
    "L9_N4": (9, 4, 1, 3, 3),
    "L21_N37_B2": (21, 37, 2, 7, 7),
    "L70_N64_B5": (70, 64, 5, 20, 40),
    "L70_N4_B301": (70, 4, 301, 3, 3),
    "L70_N4_B602": (70, 4, 602, 3, 3),
    "L70_N4_B1003": (70, 4, 1003, 3, 3),
    "L37_N100_B3": (37, 100, 3, 10, 20),
    "L40_N128_B9": (40, 128, 9, 12, 14),
    "L24_N256": (24, 256, 1, 5, 9),
    "L12_N501": (12, 501, 1, 4, 6),
}


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def atmosphere(N, name, mu0=None):
    """(P [2N, 2N], P0 [2N] or None)"""
    mu = inputs.direction_grid(N)
    if name == "rayleigh":
        P = inputs.phase_function("rayleigh", N, mu, 0.5, 0.0)[1]
        return P, (None if mu0 is None else O.phase_p0("rayleigh", N, mu, mu0, 0.0))
    r = ATMOSPHERES.index(name)
    P, P0 = LP.legendre_phase(N, mu, LP.terms(r), mu0=mu0)
    return P, P0


@functools.lru_cache(maxsize=None)
def hg(N):
    return inputs.phase_function("hg", N, inputs.direction_grid(N), 0.5, 0.7)[1]


def source_case(shape, atm):
    """Digest of Solver.source(X) for columns with different coefficients each."""
    from sosrt.solver import Solver
    L, N, B, iu, idn = SOURCE_SHAPES[shape]
    b = np.arange(B)
    s = Solver(L, N, max_batch=B)
    try:
        s.set_grid(inputs.direction_grid(N))
        s.set_phase(atmosphere(N, atm)[0], hg(N))
        s.set_columns(np.full(B, iu), np.full(B, idn), 0.3 + 0.6 * (b % 7) / 7, 0.1 * (b % 5), 1.0 - 0.05 * (b % 11),
                      0.95 - 0.05 * (b % 3), 0.002 * (1 + b % 4), 0.03 / (1 + b % 6), np.full(B, 0.5))
        rng = np.random.default_rng(7000 * L + 13 * N + B)
        X = rng.choice([-1.0, 1.0], (B, L, 2 * N)) * 10.0 ** rng.uniform(-6, 0, (B, L, 2 * N))
        J = s.source(X)
    finally:
        s.close()
    assert not np.isnan(J).any()
    return digest(J)


# ---- whole solves ------------------------------------------------------------------------------------------------------------------
KNOBS = ("SOSRT_GEMM_REGS", "SOSRT_GEMM_SMALL", "SOSRT_DENSE_LIVE_LIST", "SOSRT_GROUPS", "SOSRT_SPLIT_MIN", "SOSRT_ORDER_LOOP",
         "SOSRT_RING_MOMENTS")


def fresh(monkeypatch=None, **env):
    """Close the cached handles; with `monkeypatch`, clear the knobs and set `env`."""
    from sosrt import main as M
    if monkeypatch is not None:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    for s_ in list(M._solvers.values()):
        s_.close()
    M._solvers.clear()


# Columns that converge while the dense tiling still runs: B = 8, L = 40, N = 64.  Columns 1, 4 and 6 absorb (single-scattering
# albedos 0.30 / 0.35) over a black ground and stop several orders before the five others (albedos 1.0 / 0.95, bright ground), which
# meanwhile keep 5 of 8 = 62.5 % of the batch live.  test_the_converging_batch_spreads_its_order_counts checks the spread with the
# oracle, without a GPU.
CONV = dict(L=40, N=64,
            mu0=np.array([0.9, 0.5, 0.7, 0.6, 0.8, 0.95, 0.4, 0.75]),
            taer=np.array([0.6, 0.02, 0.6, 0.6, 0.02, 0.6, 0.02, 0.6]),
            rho=np.array([0.8, 0.0, 0.7, 0.8, 0.0, 0.75, 0.0, 0.8]),
            alb_atm=np.array([1.0, 0.30, 1.0, 1.0, 0.30, 1.0, 0.30, 1.0]),
            alb_aer=np.array([0.95, 0.35, 0.95, 0.95, 0.35, 0.95, 0.35, 0.95]))
CONV_EARLY = (1, 4, 6)


def conv_inputs(atm="rayleigh"):
    c = CONV
    N = c["N"]
    mu = inputs.direction_grid(N)
    P0a = np.stack([atmosphere(N, atm, float(m))[1] for m in c["mu0"]])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in c["mu0"]])
    return P0a, P0r, dict(tauStar_atm=0.124, nb_layers=c["L"], nb_angles=N, max_orders=200, P_atm=atmosphere(N, atm)[0], P_aer=hg(N))


def conv_solve(cols=slice(None), atm="rayleigh"):
    from sosrt.main import SOS_Aer_batch
    c = CONV
    P0a, P0r, kw = conv_inputs(atm)
    return SOS_Aer_batch(c["mu0"][cols], c["taer"][cols], c["rho"][cols], alb_atm=c["alb_atm"][cols], alb_aer=c["alb_aer"][cols],
                         P0_atm=P0a[cols], P0_aer=P0r[cols], **kw)


def conv_oracle_orders(atm="rayleigh"):
    c = CONV
    P0a, P0r, kw = conv_inputs(atm)
    n = []
    for b in range(len(c["mu0"])):
        col = O.make_column(c["mu0"][b], 120, 25, 17, c["L"], 0.124, c["taer"][b], c["rho"][b], c["alb_atm"][b], c["alb_aer"][b],
                            c["N"], P0a[b], kw["P_atm"], P0r[b], kw["P_aer"])
        n.append(O.solve_column(col, literal=False).n)
    return np.array(n)


# a batch whose columns stop at different orders, through every live-column tiling (tests/test_gpu_contraction_edges.py: _batch)
TILINGS = dict(L=72, N=64, B=40)
TILING_ENV = {"default": {}, "gemm_regs_0": {"SOSRT_GEMM_REGS": "0"}, "gemm_small_0": {"SOSRT_GEMM_SMALL": "0"},
              "gemm_small_0_regs_0": {"SOSRT_GEMM_SMALL": "0", "SOSRT_GEMM_REGS": "0"}, "dense_live_list_0": {"SOSRT_DENSE_LIVE_LIST": "0"}}


@functools.lru_cache(maxsize=None)
def tilings_inputs(atm):
    L, N, B = TILINGS["L"], TILINGS["N"], TILINGS["B"]
    rng = np.random.default_rng(100 * L + N + ATMOSPHERES.index(atm))
    mu = inputs.direction_grid(N)
    mu0 = rng.uniform(0.2, 1.0, B)
    taer = rng.choice([0.02, 0.12, 0.6], B)
    rho = rng.uniform(0.0, 0.8, B)
    P0a = np.stack([atmosphere(N, atm, float(m))[1] if atm != "zero" else np.zeros(2 * N) for m in mu0])
    P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in mu0])
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, P_atm=atmosphere(N, atm)[0], P_aer=hg(N))
    return mu0, taer, rho, P0a, P0r, kw


def tilings_solve(atm):
    from sosrt.main import SOS_Aer_batch
    mu0, taer, rho, P0a, P0r, kw = tilings_inputs(atm)
    return SOS_Aer_batch(mu0, taer, rho, P0_atm=P0a, P0_aer=P0r, **kw)


def solve_digests(r):
    return {"I": digest(r.I), "n": digest(np.asarray(r.n, dtype=np.int64))}
