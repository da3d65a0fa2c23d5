#!/usr/bin/env python3
"""Cost of the azimuth-resolved solve on the C4 batch: 512 columns = 8 mu0 x 8 tau*_aer x 8 grd_alb, L = 200,
N = 128, Rayleigh + EVA, M = 16 modes, 36 azimuths, TOA and surface rows.  Prints milliseconds of the mode-0 solve, of each
mode m >= 1 (its host fold, its solve with the mode-0 order counts, its synthesis), and of the builders.

    python3 tools/time_azimuth.py [M] [reps]

    python3 tools/time_azimuth.py --mode-batch [--tree DIR] [--batches 1,8,64,512] [--modes 16] [--reps 10] [--loop-only]

--mode-batch: the WHOLE call SOS_Aer_batch(..., azimuths=36 angles, n_modes=M) on the first B columns of that batch, median of
`reps` after one warm-up call: with the loop over the modes, with mode_batch=True, and the stages of the batched driver
(`stage_timing`: a run of its own, since it waits for the device around every stage).  --tree DIR imports the package
(and its library) from another checkout of the repository, e.g. of the parent commit, whose loop is then what is timed
(--loop-only: a tree without mode_batch).  Run the variants alternating, in one visit to the device."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt import inputs  # noqa: E402
from sosrt.solver import Solver  # noqa: E402


STAGES = {"builders": ("set_phase_table", "phase_modes", "phase_modes_device", "phase_p0_modes_device"),
          "atm_factorisation": ("set_atm_phase_sets",), "device_fold": ("set_phase_sets_device",),
          "columns": ("set_columns", "set_aerosol_sets", "set_atmosphere_sets"), "solve": ("solve_device",),
          "synthesis": ("azimuth_synthesize_device",)}


def stage_timing(SM):
    """Wraps the Solver methods that make up the stages of main.azimuth_modes_batched (STAGES), and the host's table builder
    inputs._scalar_phase ("builders"): inside that driver, and only there, each call waits for the device before and after and
    adds its wall milliseconds to the returned dict.  "columns" includes putting the B columns back at the end.  The returned
    function takes the wrappers off."""
    from sosrt import inputs as _inputs
    acc, on, saved = {}, [False], []

    def timed(f, key, sync):
        def g(*a, **k):
            if not on[0]:
                return f(*a, **k)
            sync(a)
            t0 = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                sync(a)
                acc[key] = acc.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        return g

    def patch(obj, name, key, sync):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, timed(getattr(obj, name), key, sync))

    for key, names in STAGES.items():
        for name in names:
            patch(Solver, name, key, lambda a: a[0].synchronize())
    patch(_inputs, "_scalar_phase", "builders", lambda a: None)
    driver = SM.azimuth_modes_batched

    def batched(*a, **k):
        on[0] = True
        try:
            return driver(*a, **k)
        finally:
            on[0] = False
    saved.append((SM, "azimuth_modes_batched", driver))
    SM.azimuth_modes_batched = batched

    def undo():
        for obj, name, f in saved:
            setattr(obj, name, f)
    return acc, undo


def whole_calls(argv):
    from sosrt import main as SM
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    batches = [int(x) for x in opt("--batches", "1,8,64,512").split(",")]
    M_, reps, loop_only = int(opt("--modes", "16")), int(opt("--reps", "10")), "--loop-only" in argv
    side = 8
    g = np.meshgrid(np.linspace(0.2, 1.0, side), np.geomspace(0.01, 1.0, side), np.linspace(0.0, 0.8, side), indexing="ij")
    mu0, taer, rho = (x.reshape(-1).copy() for x in g)
    pick = lambda B: np.linspace(0, mu0.size - 1, B).astype(int)       # (spread over the batch: several aerosol depths)
    phi = np.linspace(0, 2 * np.pi, 37)[:36]
    kw = dict(alb_aer=0.97, nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", aer_phase_fun="eva", azimuths=phi, n_modes=M_)

    def med(f):
        f()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return np.median(t), np.min(t), np.max(t)

    for B in batches:
        c = pick(B)
        call = lambda **k: SM.SOS_Aer_batch(mu0[c], taer[c], rho[c], **kw, **k)
        plain = med(lambda: SM.SOS_Aer_batch(mu0[c], taer[c], rho[c], **{k: v for k, v in kw.items() if k not in ("azimuths", "n_modes")}))
        loop = med(call)
        line = "WHOLE tree=%s B=%d M=%d plain_ms=%.3f loop_ms=%.3f (min %.3f max %.3f)" % (os.path.basename(ROOT), B, M_, plain[0], *loop)
        if not loop_only:
            bat = med(lambda: call(mode_batch=True))
            st, undo = stage_timing(SM)
            tot = med(lambda: call(mode_batch=True))
            undo()
            line += " batched_ms=%.3f (min %.3f max %.3f) ratio_loop_over_batched=%.2f; stages per call, ms (timed run %.3f ms): %s" % (
                *bat, loop[0] / bat[0], tot[0], " ".join("%s=%.3f" % (k, v / (reps + 1)) for k, v in sorted(st.items())))
        print(line, flush=True)


if "--mode-batch" in sys.argv or "--loop-only" in sys.argv:
    whole_calls(sys.argv)
    sys.exit(0)

M = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
L, N, side = 200, 128, 8
B, D, nphi = side ** 3, 2 * N, max(25, 2 * M + 1)
g = np.meshgrid(np.linspace(0.2, 1.0, side), np.geomspace(0.01, 1.0, side), np.linspace(0.0, 0.8, side), indexing="ij")
mu0, taer, rho = (x.reshape(-1).copy() for x in g)
iu, idn = inputs.slab_indices(120, 25, 17, L)
tau = np.stack([inputs.tau_profile(0.124, t, 120, 25, 17, L) for t in taer])
dev = torch.device("cuda", 0)
s = Solver(L, N, max_batch=B, max_orders=256)
s.set_grid(inputs.direction_grid(N))
tab = inputs._scalar_phase("eva")[1][1]
s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.97, 0.124 / L, taer / (idn + 1 - iu), 0.124 + taer)
d_tau = torch.from_numpy(tau).to(dev)
d_mu0 = torch.from_numpy(mu0).to(dev)
d_I = torch.empty((B, L, D), dtype=torch.float64, device=dev)
d_Im = torch.empty_like(d_I)
d_n = torch.zeros(B, dtype=torch.int32, device=dev)
d_nm = torch.zeros(B, dtype=torch.int32, device=dev)
phi = torch.linspace(0, 2 * np.pi, 37, dtype=torch.float64, device=dev)[:36].contiguous()
lev = torch.tensor([0, L - 1], dtype=torch.int32, device=dev)
out = torch.empty((B, 2, D, 36), dtype=torch.float64, device=dev)
P0a = torch.empty((M + 1, B, D), dtype=torch.float64, device=dev)
P0r = torch.empty_like(P0a)


def ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    s.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def builders():
    global Pa, Pr
    Pa = s.phase_modes("rayleigh", 0, M + 1, nphi)
    s.phase_p0_modes_device("rayleigh", d_mu0.data_ptr(), P0a.data_ptr(), B, 0, M + 1, nphi)
    s.set_phase_table(*tab)
    Pr = s.phase_modes("table", 0, M + 1, nphi)
    s.phase_p0_modes_device("table", d_mu0.data_ptr(), P0r.data_ptr(), B, 0, M + 1, nphi)


rows = []
for rep in range(REPS):
    t_build = ms(builders)
    s.set_phase(Pa[0], Pr[0])
    t0 = ms(lambda: s.solve_device(d_tau.data_ptr(), P0a[0].data_ptr(), P0r[0].data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr()))
    t_syn = [ms(lambda: s.azimuth_accumulate_device(0, d_I.data_ptr(), lev.data_ptr(), 2, phi.data_ptr(), 36, out.data_ptr()))]
    s.set_order_targets(d_n.data_ptr())
    t_fold, t_mode = [], []
    for m in range(1, M + 1):
        t_fold.append(ms(lambda: s.set_phase(Pa[m], Pr[m])))
        t_mode.append(ms(lambda: s.solve_device(d_tau.data_ptr(), P0a[m].data_ptr(), P0r[m].data_ptr(), d_Im.data_ptr(),
                                                d_n_orders=d_nm.data_ptr())))
        assert torch.equal(d_nm, d_n)
        t_syn.append(ms(lambda: s.azimuth_accumulate_device(m, d_Im.data_ptr(), lev.data_ptr(), 2, phi.data_ptr(), 36, out.data_ptr())))
    s.set_order_targets(None)
    rows.append((t0, t_build, np.array(t_mode), np.array(t_fold), np.array(t_syn)))
    n = d_n.cpu().numpy()
    print("rep %d: mode-0 solve %.3f ms (orders: max %d, sum %d); modes 1..%d: solve %.3f ms each (min %.3f, max %.3f), "
          "host fold %.3f ms each; builders (P^m, P0^m, m = 0..%d, both phase functions, nphi = %d) %.3f ms; synthesis %.4f ms per mode"
          % (rep, t0, n.max(), n.sum(), M, np.mean(t_mode), np.min(t_mode), np.max(t_mode), np.mean(t_fold), M, nphi, t_build,
             np.mean(t_syn)), flush=True)
t0, tb, tm, tf, ts = rows[-1]
print("SUMMARY C4 (B=%d, L=%d, N=%d, eva, M=%d, 36 azimuths, 2 levels): mode0_ms=%.3f per_mode_ms=%.3f per_mode_fold_ms=%.3f "
      "builders_ms=%.3f synthesis_ms_per_mode=%.4f total_ms=%.3f (%.2f x the mode-0 solve)"
      % (B, L, N, M, t0, tm.mean(), tf.mean(), tb, ts.mean(), t0 + tm.sum() + tf.sum() + tb + ts.sum(),
         (t0 + tm.sum() + tf.sum() + tb + ts.sum()) / t0))
s.close()
