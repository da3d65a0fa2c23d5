#!/usr/bin/env python3
"""Cost of the Cox-Munk kind against the kinds beside it, by the method of tools/time_phase_builders.py.

    python3 tools/time_ocean_ground.py [--reps 10] [--rounds 3] [--calls 10] [--out profiles/cox_munk_timing.txt]

Builders: each of the seven builder entries of the C ABI (csrc/brdf.hip) per kind, on a shape a user runs -- N = 128, B = 512
columns, V = 64 view cosines, 65 azimuth nodes, modes 1..16, 36 azimuths -- timed with device events on the handle's stream around
the call after one warm-up call, `reps` calls in each of `rounds` fresh processes, pooled: median (min max) in microseconds.
Whole calls: SOS_Aer_batch on the 512-column batch (8 mu0 x 8 tau*_aer x 8 f_iso, L = 200, N = 128, Rayleigh + HG 0.7) over the
ocean, the Ross-Li and the Lambertian ground, `calls` calls after one warm-up in one more fresh process, timed on the host around
a device synchronize: median (min max) in milliseconds.  A process that fails ends the run: nothing is started on the device
after it."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))

N, B, V, MODES, NPHI, NAZ = 128, 512, 64, (1, 16), 65, 36
KINDS = (("lambertian", ()), ("rpv", (0.2, 0.8, -0.1)), ("ross_thick", (0.17364817766693033,)), ("li_sparse_r", (0.17364817766693033,)),
         ("cox_munk", (0.0286, 1.34, 1.0)), ("cox_munk", (0.0286, 1.34, 0.0)))


def label(kind, p):
    return kind if kind != "cox_munk" else "cox_munk shadow %d" % p[2]


def builders(reps):
    """{entry/kind: [microseconds] * reps}"""
    import numpy as np
    import torch
    from sosrt import inputs
    from sosrt.solver import Solver
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    buf = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    s = Solver(8, N, max_batch=B)
    stream = torch.cuda.Stream(device=dev)
    s.set_stream(stream.cuda_stream)
    s.set_grid(inputs.direction_grid(N))
    iu, idn = inputs.slab_indices(120, 25, 17, 8)
    mu0 = np.linspace(0.2, 1.0, B)
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, 0.0, 1.0, 0.95, 0.124 / 8, 0.3 / (idn + 1 - iu), 0.424)
    M1, (mf, mc) = N - 1, MODES
    vmu = np.linspace(0.05, 1.0, V)
    d_mu0, d_phi = up(mu0), up(np.linspace(0, 2 * np.pi, NAZ + 1)[:NAZ])
    o_R, o_r0, o_Rm, o_r0m = buf(M1, M1), buf(B, M1), buf(mc, M1, M1), buf(mc, B, M1)
    o_Rv, o_r0v, o_az = buf(mc, M1, V), buf(mc, B, V), buf(NAZ, B, V)
    entries = {
        "brdf_operator_dev": lambda k, p: s.brdf_operator_device(k, o_R.data_ptr(), p, NPHI),
        "brdf_beam_dev": lambda k, p: s.brdf_beam_device(k, d_mu0.data_ptr(), o_r0.data_ptr(), p, NPHI, B=B),
        "brdf_operator_modes_dev": lambda k, p: s.brdf_operator_modes_device(k, o_Rm.data_ptr(), mf, mc, p, NPHI, sign_odd=True),
        "brdf_beam_modes_dev": lambda k, p: s.brdf_beam_modes_device(k, d_mu0.data_ptr(), o_r0m.data_ptr(), mf, mc, p, NPHI, B=B),
        "brdf_view_rows_modes_dev": lambda k, p: s.brdf_view_rows_modes_device(k, vmu, o_Rv.data_ptr(), mf, mc, p, NPHI, sign_odd=True),
        "brdf_view_beam_modes_dev": lambda k, p: s.brdf_view_beam_modes_device(k, d_mu0.data_ptr(), vmu, o_r0v.data_ptr(), mf, mc, p, NPHI, B=B),
        "brdf_view_beam_azimuth_dev": lambda k, p: s.brdf_view_beam_azimuth_device(k, d_mu0.data_ptr(), vmu, d_phi.data_ptr(), NAZ,
                                                                                  o_az.data_ptr(), p, B=B),
    }
    torch.cuda.synchronize()
    out = {}
    for name, f in entries.items():
        for kind, p in KINDS:
            f(kind, p)
            s.synchronize()
            t = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f(kind, p)
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3)
            out["%s/%s" % (name, label(kind, p))] = t
    s.close()
    return out


def whole_calls(calls):
    """{ground: {"ms": [...], "bounces": max, "orders": sum of the reflections' orders of the slowest column, "status": any}}"""
    import numpy as np
    import torch
    from sosrt.main import SOS_Aer_batch
    side = 8
    mu0, taer, f_iso = np.linspace(0.2, 1.0, side), np.geomspace(0.05, 0.8, side), np.linspace(0.0, 0.1, side)
    M0, TA, FI = (x.ravel() for x in np.meshgrid(mu0, taer, f_iso, indexing="ij"))
    wind = np.array([2.0, 5.0, 10.0])[np.arange(B) % 3]
    grounds = {
        "cox_munk, one wind (5 m/s)": ("cox_munk", 5.0, 1.34, FI, 1.0),
        "cox_munk, three winds (2, 5, 10 m/s)": ("cox_munk", wind, 1.34, FI, 1.0),
        "ross_li": ("ross_li", FI + 0.05, np.linspace(0.02, 0.32, B), np.linspace(0.001, 0.051, B)),
        "lambertian, grd_alb = f_iso + 0.05": "lambertian",
    }
    out = {}
    for name, brdf in grounds.items():
        call = lambda: SOS_Aer_batch(M0, TA, FI + 0.05 if brdf == "lambertian" else 1.0, nb_layers=200, nb_angles=N, atm_phase_fun="rayleigh",
                                     aer_phase_fun="hg", g_aer=0.7, alb_aer=0.95, surface="brdf", brdf=brdf, raise_on_error=False)
        r = call()
        t = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(ms=t, bounces=int(r.bounces.max()), orders=int(r.bounce_orders.max(axis=1).sum()), status=bool(r.status.any()))
    return out


def child(argv, what, n):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(n)], capture_output=True, text=True, timeout=600)
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit("the %s process failed (exit %d):\n%s" % (what, r.returncode, r.stderr[-2000:]))
    return json.loads(res[0][7:])


def main(argv):
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    if "--child" in argv:
        what, n = argv[argv.index("--child") + 1], int(argv[argv.index("--child") + 2])
        print("RESULT " + json.dumps(builders(n) if what == "builders" else whole_calls(n)), flush=True)
        return
    import numpy as np
    reps, rounds, calls = int(opt("--reps", "10")), int(opt("--rounds", "3")), int(opt("--calls", "10"))
    stat = lambda t: (float(np.median(t)), float(np.min(t)), float(np.max(t)))
    pooled = {}
    for _ in range(rounds):
        for k, t in child(argv, "builders", reps).items():
            pooled.setdefault(k, []).extend(t)
    lines = ["# tools/time_ocean_ground.py: builders at N=%d B=%d V=%d, %d azimuth nodes, modes %d..%d, %d azimuths; device events around the "
             "call, us: median (min max) of %d calls in each of %d fresh processes"
             % (N, B, V, NPHI, MODES[0], MODES[0] + MODES[1] - 1, NAZ, reps, rounds)]
    lines += ["%-52s %9.1f (%9.1f %9.1f)" % (k, *stat(t)) for k, t in pooled.items()]
    lines.append("# whole SOS_Aer_batch calls, 512 columns (8 mu0 x 8 tau*_aer x 8 f_iso), L=200, N=%d, host clock around a device "
                 "synchronize, ms: median (min max) of %d calls after one warm-up" % (N, calls))
    for k, v in child(argv, "calls", calls).items():
        lines.append("%-52s %9.1f (%9.1f %9.1f)   reflections %d, their orders %d, any status %s" % (k, *stat(v["ms"]), v["bounces"], v["orders"], v["status"]))
    print("\n".join(lines), flush=True)
    out_path = opt("--out", None)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
