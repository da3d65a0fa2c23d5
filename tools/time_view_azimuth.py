#!/usr/bin/env python3
"""Cost of the azimuth-resolved view radiance on the C4 batch: 512 columns = 8 mu0 x 8 tau*_aer x 8 grd_alb,
L = 200, N = 128, Rayleigh + EVA, M = 16 modes, 36 azimuths, TOA and surface rows, V = 16 and 64 view cosines.

    python3 tools/time_view_azimuth.py [--views 16,64] [--modes 16] [--reps 10] [--batch 512] [--out profiles/view_azimuth_timing.txt]

Per V, median of `reps` wall times after one warm-up call, all in one visit to the device:
  view_mu        SOS_Aer_batch(..., view_mu=)                          the azimuth average at the view lanes
  azimuths       SOS_Aer_batch(..., azimuths=36 angles, n_modes=M)      the grid's azimuth synthesis: the same mode solves
  view_azimuths  SOS_Aer_batch(..., view_mu=, view_azimuths=36 angles)  with view_first_order 'exact' and 'modes'
and the view share of the 'exact' call, from a run of its own in which every call of the stage waits for the device before and
after: the builders of rows (all modes, once), the view stage per mode, the synthesis per mode, the exact first order (36
closed-form evaluations).  The lines go to stdout and to --out."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt import main as SM  # noqa: E402
from sosrt.solver import Solver  # noqa: E402

STAGES = {"row_builders": ("phase_rows_modes_device", "phase_p0_rows_modes_device", "phase_p0_rows_azimuth_device"),
          "view_stage": ("view_radiance_device",), "synthesis": ("view_azimuth_accumulate_device",)}


def stage_timing():
    """Wraps the Solver methods of the view stage inside main.view_azimuth_modes: each call waits for the device before and
    after and adds its wall milliseconds (and a count) to the returned dict.  The returned function takes the wrappers off."""
    acc, cnt, on, saved = {}, {}, [False], []

    def timed(f, key):
        def g(self, *a, **k):
            if not on[0]:
                return f(self, *a, **k)
            self.synchronize()
            t0 = time.perf_counter()
            try:
                return f(self, *a, **k)
            finally:
                self.synchronize()
                acc[key] = acc.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
                cnt[key] = cnt.get(key, 0) + 1
        return g

    for key, names in STAGES.items():
        for name in names:
            saved.append((Solver, name, getattr(Solver, name)))
            setattr(Solver, name, timed(getattr(Solver, name), key))
    driver = SM.view_azimuth_modes

    def wrapped(*a, **k):
        on[0] = True
        try:
            return driver(*a, **k)
        finally:
            on[0] = False
    saved.append((SM, "view_azimuth_modes", driver))
    SM.view_azimuth_modes = wrapped

    def undo():
        for obj, name, f in saved:
            setattr(obj, name, f)
    return acc, cnt, undo


def main(argv):
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    views = [int(x) for x in opt("--views", "16,64").split(",")]
    M, reps, B = int(opt("--modes", "16")), int(opt("--reps", "10")), int(opt("--batch", "512"))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "view_azimuth_timing.txt"))
    side = 8
    g = np.meshgrid(np.linspace(0.2, 1.0, side), np.geomspace(0.01, 1.0, side), np.linspace(0.0, 0.8, side), indexing="ij")
    mu0, taer, rho = (x.reshape(-1).copy() for x in g)
    c = np.linspace(0, mu0.size - 1, B).astype(int)
    phi = np.linspace(0, 2 * np.pi, 37)[:36]
    kw = dict(alb_aer=0.97, nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", aer_phase_fun="eva")
    call = lambda **k: SM.SOS_Aer_batch(mu0[c], taer[c], rho[c], **kw, **k)

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

    lines = ["# tools/time_view_azimuth.py: B=%d L=200 N=128 rayleigh+eva M=%d 36 azimuths 2 levels, median (min max) of %d wall times, ms"
             % (B, M, reps)]
    plain = med(call)
    az = med(lambda: call(azimuths=phi, n_modes=M))
    lines.append("plain_ms=%.3f (%.3f %.3f) azimuths_ms=%.3f (%.3f %.3f)" % (*plain, *az))
    print(lines[-1], flush=True)
    for V in views:
        vmu = np.linspace(0.05, 1.0, V)
        base = med(lambda: call(view_mu=vmu))
        exact = med(lambda: call(view_mu=vmu, view_azimuths=phi, n_modes=M))
        modes = med(lambda: call(view_mu=vmu, view_azimuths=phi, n_modes=M, view_first_order="modes"))
        acc, cnt, undo = stage_timing()
        timed = med(lambda: call(view_mu=vmu, view_azimuths=phi, n_modes=M))
        undo()
        per = {k: v / (reps + 1) for k, v in acc.items()}
        n_stage = cnt["view_stage"] // (reps + 1)
        lines.append("V=%d view_mu_ms=%.3f (%.3f %.3f) view_azimuths_exact_ms=%.3f (%.3f %.3f) view_azimuths_modes_ms=%.3f (%.3f %.3f) "
                     "exact_over_azimuths=%.3f; view share of the exact call (timed run %.3f ms): row_builders=%.3f "
                     "view_stage=%.3f over %d calls (%d modes + 36 first orders) synthesis=%.3f over %d calls"
                     % (V, *base, *exact, *modes, exact[0] / az[0], timed[0], per["row_builders"], per["view_stage"], n_stage, M,
                        per["synthesis"], cnt["synthesis"] // (reps + 1)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
