#!/usr/bin/env python3
"""Cost of the BRDF ground on the C4 batch: 512 columns = 8 mu0 x 64 tau*_aer, L = 200, N = 128, Rayleigh +
EVA, ground albedo 0.3.

    python3 tools/time_brdf.py [reps] [--out FILE]

Whole calls of `solve_batch_device` (the result stays on the device), milliseconds, median (min, max) of `reps` after a warm-up,
host clock around a call that ends in a synchronise: surface='brdf' with brdf='lambertian' beside the same batch on the in-loop
ground surface='lambertian_readme' and on the specular ground, their ratio and the bounce counts.  Writes
profiles/brdf_timing.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt.main import solve_batch_device  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "brdf_timing.txt")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
L, N, RHO = 200, 128, 0.3
g = np.meshgrid(np.linspace(0.2, 1.0, 8), np.geomspace(0.01, 1.0, 64), indexing="ij")
mu0, taer = (x.reshape(-1).copy() for x in g)
KW = dict(nb_layers=L, nb_angles=N, aer_phase_fun="eva", alb_aer=0.97)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def timed(**kw):
    call = lambda: solve_batch_device(mu0, taer, RHO, **KW, **kw)[0]
    out = call()                                             # warm-up: the handle, the phase matrices, torch's allocator
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), min(t), max(t)


say("BRDF ground on the C4 batch (B=%d L=%d N=%d, Rayleigh + EVA, albedo %g): whole solve_batch_device calls, ms, median (min, max) of %d"
    % (mu0.size, L, N, RHO, REPS))
res = {}
for name, kw in (("specular", dict(surface="specular")), ("lambertian_readme (in-loop)", dict(surface="lambertian_readme")),
                 ("brdf='lambertian' (series)", dict(surface="brdf", brdf="lambertian"))):
    res[name] = timed(**kw)
    out, med, lo, hi = res[name]
    say("  %-30s %9.2f  (%.2f, %.2f)   orders of the plain solve: max %d, sum %d" % (name, med, lo, hi, int(out["n"].max()), int(out["n"].sum())))
series, loop = res["brdf='lambertian' (series)"], res["lambertian_readme (in-loop)"]
b = series[0]["bounces"].cpu().numpy()
say("  series / in-loop = %.2f;  bounces: max %d, mean %.2f (every column runs the batch's maximum);  status: %d columns non-zero"
    % (series[1] / loop[1], b.max(), b.mean(), int((series[0]["status"] != 0).sum())))
say("  (the in-loop call starts from the coded first order, whose ground reflects the beam specularly: the two calls are the same work"
    " on the same columns, not the same field)")
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
