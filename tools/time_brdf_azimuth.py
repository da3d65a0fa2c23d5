#!/usr/bin/env python3
"""Cost of the azimuth-resolved radiance over a BRDF ground on the C4 batch: 512 columns = 8 mu0 x 64
tau*_aer, L = 200, N = 128, Rayleigh + EVA, RPV (0.2, 0.8, -0.1), M = 16 modes, 36 azimuths, TOA and surface rows.

    python3 tools/time_brdf_azimuth.py [reps] [--out FILE]

Whole calls of `SOS_Aer_batch` (the fields come back to the host), milliseconds, median (min, max) of `reps` after a warm-up,
host clock: the new call (surface='brdf', azimuths=, brdf_modes=True) beside the same batch with azimuths= on the specular ground
and the surface='brdf' call without azimuths; their ratio beside the reflections + 1 the code makes one expect; and the build of
the operator and beam-row modes 1..16 alone, stream synchronised around it.  Writes profiles/brdf_azimuth_timing.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt.main import BRDF_NPHI, SOS_Aer_batch, get_solver  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "brdf_azimuth_timing.txt")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
L, N, M, RPV = 200, 128, 16, ("rpv", 0.2, 0.8, -0.1)
g = np.meshgrid(np.linspace(0.2, 1.0, 8), np.geomspace(0.01, 1.0, 64), indexing="ij")
mu0, taer = (x.reshape(-1).copy() for x in g)
PHI = np.linspace(0, 2 * np.pi, 36, endpoint=False)
KW = dict(nb_layers=L, nb_angles=N, aer_phase_fun="eva", alb_aer=0.97)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def timed(grd_alb, **kw):
    call = lambda: SOS_Aer_batch(mu0, taer, grd_alb, **KW, **kw)
    out = call()                                             # warm-up: the handle, the phase matrices, torch's allocator
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), min(t), max(t)


say("Azimuth-resolved radiance over a BRDF ground on the C4 batch (B=%d L=%d N=%d, Rayleigh + EVA, RPV %s, M=%d, %d azimuths): whole "
    "SOS_Aer_batch calls, ms, median (min, max) of %d" % (mu0.size, L, N, RPV[1:], M, PHI.size, REPS))
res = {}
for name, alb, kw in (("brdf, azimuths, brdf_modes=True", 1.0, dict(surface="brdf", brdf=RPV, azimuths=PHI, n_modes=M, brdf_modes=True)),
                      ("specular (albedo 0.3), azimuths", 0.3, dict(azimuths=PHI, n_modes=M)),
                      ("brdf without azimuths", 1.0, dict(surface="brdf", brdf=RPV))):
    res[name] = timed(alb, **kw)
    out, med, lo, hi = res[name]
    say("  %-34s %9.2f  (%.2f, %.2f)   orders of the mode-0 solve: max %d, sum %d" % (name, med, lo, hi, int(out.n.max()), int(out.n.sum())))
new, spec = res["brdf, azimuths, brdf_modes=True"], res["specular (albedo 0.3), azimuths"]
K = new[0].bounce_orders.shape[0]
say("  new / specular azimuths = %.2f (reflections + 1 = %d);  orders of the reflections' solves: max %s;  mode status: %d non-zero"
    % (new[1] / spec[1], K + 1, new[0].bounce_orders.max(axis=1), int((new[0].mode_status != 0).sum())))

# the build of the modes 1..M of the operator and of the beam rows alone
s = get_solver(L, N, mu0.size, 256)
dev = torch.device("cuda", 0)
d_mu0 = torch.from_numpy(mu0).to(dev)
d_R = torch.empty((M, N - 1, N - 1), dtype=torch.float64, device=dev)
d_r0 = torch.empty((M, mu0.size, N - 1), dtype=torch.float64, device=dev)
t = []
for _ in range(REPS + 1):
    torch.cuda.synchronize()
    s.synchronize()
    t0 = time.perf_counter()
    s.brdf_operator_modes_device("rpv", d_R.data_ptr(), 1, M, RPV[1:], BRDF_NPHI, sign_odd=True)
    s.brdf_beam_modes_device("rpv", d_mu0.data_ptr(), d_r0.data_ptr(), 1, M, RPV[1:], BRDF_NPHI, B=mu0.size)
    s.synchronize()
    t.append((time.perf_counter() - t0) * 1e3)
t = t[1:]
say("  build of (-1)^m R^m and r0^m, m = 1..%d on %d nodes (2 launches each): %.3f ms  (%.3f, %.3f)" % (M, BRDF_NPHI, float(np.median(t)), min(t), max(t)))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
