#!/usr/bin/env python3
"""Cost of the view radiance over a BRDF ground on the C4 batch: 512 columns = 8 mu0 x 64 tau*_aer, L = 200,
N = 128, Rayleigh + EVA, RPV (0.2, 0.8, -0.1), V = 16 and 64 view cosines, M = 16 modes, 36 azimuths, TOA and surface rows.

    python3 tools/time_brdf_view.py [reps] [--out FILE]

Whole calls of `SOS_Aer_batch` (the fields come back to the host), milliseconds, median (min, max) of `reps` after a warm-up,
host clock: the new view_mu call (surface='brdf', brdf_view=True) beside the surface='brdf' call without views and the specular
view_mu call; the new view_azimuths call beside the azimuths call over the same ground (brdf_modes=True) and the specular
view_azimuths call; and the new stages alone, stream synchronised around them: the build of the view rows and beam rows of the
modes 1..16, the exact beam rows at the 36 azimuths, one launch of the view ground stage.  Writes profiles/brdf_view_timing.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt.main import BRDF_NPHI, SOS_Aer_batch, get_solver  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "brdf_view_timing.txt")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
L, N, M, RPV = 200, 128, 16, ("rpv", 0.2, 0.8, -0.1)
g = np.meshgrid(np.linspace(0.2, 1.0, 8), np.geomspace(0.01, 1.0, 64), indexing="ij")
mu0, taer = (x.reshape(-1).copy() for x in g)
PHI = np.linspace(0, 2 * np.pi, 36, endpoint=False)
VIEWS = {V: np.linspace(0.05, 1.0, V) for V in (16, 64)}
KW = dict(nb_layers=L, nb_angles=N, aer_phase_fun="eva", alb_aer=0.97)
BRDF = dict(surface="brdf", brdf=RPV)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def timed(name, grd_alb, **kw):
    call = lambda: SOS_Aer_batch(mu0, taer, grd_alb, **KW, **kw)
    out = call()                                             # warm-up: the handle, the phase matrices, torch's allocator
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(t))
    say("  %-52s %9.2f  (%.2f, %.2f)   orders of the mode-0 solve: max %d, sum %d" % (name, med, min(t), max(t), int(out.n.max()), int(out.n.sum())))
    return out, med


say("View radiance over a BRDF ground on the C4 batch (B=%d L=%d N=%d, Rayleigh + EVA, RPV %s, M=%d, %d azimuths): whole "
    "SOS_Aer_batch calls, ms, median (min, max) of %d" % (mu0.size, L, N, RPV[1:], M, PHI.size, REPS))
plain, t_plain = timed("brdf without views", 1.0, **BRDF)
K = plain.bounce_orders.shape[0]
for V, vmu in VIEWS.items():
    _, t_spec = timed("specular (albedo 0.3), view_mu, V=%d" % V, 0.3, view_mu=vmu)
    new, t_new = timed("brdf, view_mu, brdf_view=True, V=%d" % V, 1.0, view_mu=vmu, brdf_view=True, **BRDF)
    say("    new - brdf without views = %.2f ms (specular view_mu - specular plain is the view stage's own cost); new / specular view_mu = %.2f; "
        "reflections %d; ground's share of I_view at TOA: max %.3f" % (t_new - t_plain, t_new / t_spec, K,
                                                                     float(np.max(new.I_view_ground[:, 0] / np.maximum(new.I_view[:, 0], 1e-300)))))
_, t_spec0 = timed("specular (albedo 0.3), plain", 0.3)
_, t_az = timed("brdf, azimuths, brdf_modes=True", 1.0, azimuths=PHI, n_modes=M, brdf_modes=True, **BRDF)
for V, vmu in VIEWS.items():
    for first in ("exact", "modes"):
        _, t_sva = timed("specular, view_azimuths (%s), V=%d" % (first, V), 0.3, view_mu=vmu, view_azimuths=PHI, n_modes=M, view_first_order=first)
        new, t_new = timed("brdf, view_azimuths (%s), brdf_view=True, V=%d" % (first, V), 1.0, view_mu=vmu, view_azimuths=PHI, n_modes=M,
                           view_first_order=first, brdf_view=True, **BRDF)
        say("    new / brdf azimuths = %.2f; new / specular view_azimuths = %.2f (reflections + 1 = %d); mode status: %d non-zero"
            % (t_new / t_az, t_new / t_sva, K + 1, int((new.view_mode_status != 0).sum())))

# the new stages alone
s = get_solver(L, N, mu0.size, 256)
dev = torch.device("cuda", 0)
B = mu0.size
d_mu0, d_phi = torch.from_numpy(mu0).to(dev), torch.from_numpy(PHI).to(dev)
d_tau = torch.from_numpy(np.ascontiguousarray(plain.tau)).to(dev)
d_I = torch.from_numpy(np.ascontiguousarray(plain.I)).to(dev)
f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)


def stage(what, fn):
    t = []
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t = t[1:]
    say("  %-96s %.3f ms  (%.3f, %.3f)" % (what, float(np.median(t)), min(t), max(t)))


for V, vmu in VIEWS.items():
    d_Rv, d_r0v, d_az, d_out = f64(M, N - 1, V), f64(M, B, V), f64(PHI.size, B, V), f64(B, 2, 2 * V)

    def build():
        s.brdf_view_rows_modes_device("rpv", vmu, d_Rv.data_ptr(), 1, M, RPV[1:], BRDF_NPHI, sign_odd=True)
        s.brdf_view_beam_modes_device("rpv", d_mu0.data_ptr(), vmu, d_r0v.data_ptr(), 1, M, RPV[1:], BRDF_NPHI, B=B)
    stage("V=%d: build of (-1)^m Rv^m and r0v^m, m = 1..%d on %d nodes (2 launches each)" % (V, M, BRDF_NPHI), build)
    stage("V=%d: exact beam rows at %d azimuths (1 launch)" % (V, PHI.size),
          lambda: s.brdf_view_beam_azimuth_device("rpv", d_mu0.data_ptr(), vmu, d_phi.data_ptr(), PHI.size, d_az.data_ptr(), RPV[1:], B=B))
    stage("V=%d: view ground stage, one reflection, TOA and surface rows (1 launch)" % V,
          lambda: s.view_ground_device(vmu, d_tau.data_ptr(), [0, L - 1], d_out.data_ptr(), d_I=d_I.data_ptr(), d_Rv=d_Rv[0].data_ptr(),
                                       d_r0v=d_r0v[0].data_ptr(), B=B))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
