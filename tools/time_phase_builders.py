#!/usr/bin/env python3
"""Time of each of the nine phase-builder entries of the C ABI (csrc/phase.hip), one by one, on a shape a user runs: N = 128,
B = 512 columns, V = 64 view cosines (128 lanes), modes 1..16 on 33 nodes, 36 azimuths, Henyey-Greenstein and the tabulated function.

    python3 tools/time_phase_builders.py [--reps 10]                          one library (SOSRT_LIB, default the tree's)
    python3 tools/time_phase_builders.py --against PARENT.so [--rounds 2] [--out profiles/phase_builders_timing.txt]

An entry is timed with device events on the handle's stream around the call, after one warm-up call: the median, minimum and
maximum of `reps` calls, in microseconds.  (A mode entry uploads its table of azimuth weights inside the call: that copy is in
its time, with either library.)  --against alternates fresh processes on PARENT.so and on the tree's library, `rounds` times
each, pools each library's samples and writes both columns; a builder whose median lies above the other library's maximum is
marked.  A process that fails ends the run: nothing is started on the device after it."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))

N, B, V, MODES, NPHI, NAZ = 128, 512, 64, (1, 16), 33, 36
KINDS = (("hg", 0.7), ("table", 0.0))


def measure(reps):
    """{entry/kind: [microseconds] * reps}"""
    import numpy as np
    import torch
    from sosrt import inputs
    from sosrt.solver import Solver
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    buf = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    s = Solver(4, N, max_batch=B)
    stream = torch.cuda.Stream(device=dev)
    s.set_stream(stream.cuda_stream)
    s.set_grid(inputs.direction_grid(N))
    s.set_phase_table(*inputs.fwc_table())
    D, V2, (mf, mc) = 2 * N, 2 * V, MODES
    vmu = np.linspace(0.05, 1.0, V)
    sgn = np.concatenate((-vmu, vmu))
    d_mu0, d_phi = up(np.linspace(0.2, 1.0, B)), up(np.linspace(0, 2 * np.pi, NAZ + 1)[:NAZ])
    o_P, o_P0, o_Pm, o_P0m = buf(D, D), buf(B, D), buf(mc, D, D), buf(mc, B, D)
    o_r, o_p0r, o_rm, o_p0rm, o_az = buf(V2, D), buf(B, V2), buf(mc, V2, D), buf(mc, B, V2), buf(NAZ, B, V2)
    entries = {
        "phase_matrix_dev": lambda k, g: s.phase_matrix_device(k, o_P.data_ptr(), g),
        "phase_p0_dev": lambda k, g: s.phase_p0_device(k, d_mu0.data_ptr(), o_P0.data_ptr(), B, g),
        "phase_modes_dev": lambda k, g: s.phase_modes_device(k, o_Pm.data_ptr(), mf, mc, NPHI, g, sign_odd=True),
        "phase_p0_modes_dev": lambda k, g: s.phase_p0_modes_device(k, d_mu0.data_ptr(), o_P0m.data_ptr(), B, mf, mc, NPHI, g),
        "phase_rows_dev": lambda k, g: s.phase_rows_device(k, sgn, o_r.data_ptr(), g),
        "phase_p0_rows_dev": lambda k, g: s.phase_p0_rows_device(k, d_mu0.data_ptr(), sgn, o_p0r.data_ptr(), B, g),
        "phase_rows_modes_dev": lambda k, g: s.phase_rows_modes_device(k, sgn, o_rm.data_ptr(), mf, mc, NPHI, g, sign_odd=True),
        "phase_p0_rows_modes_dev": lambda k, g: s.phase_p0_rows_modes_device(k, d_mu0.data_ptr(), sgn, o_p0rm.data_ptr(), B, mf, mc, NPHI, g),
        "phase_p0_rows_azimuth_dev": lambda k, g: s.phase_p0_rows_azimuth_device(k, d_mu0.data_ptr(), sgn, d_phi.data_ptr(), NAZ,
                                                                                 o_az.data_ptr(), B, g),
    }
    torch.cuda.synchronize()
    out = {}
    for name, f in entries.items():
        for kind, g in KINDS:
            f(kind, g)
            s.synchronize()
            t = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f(kind, g)
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3)
            out["%s/%s" % (name, kind)] = t
    s.close()
    return out


def main(argv):
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    reps = int(opt("--reps", "10"))
    if "--child" in argv:
        print("RESULT " + json.dumps(measure(reps)), flush=True)
        return
    import numpy as np
    stat = lambda t: (float(np.median(t)), float(np.min(t)), float(np.max(t)))
    head = "# tools/time_phase_builders.py: N=%d B=%d V=%d modes %d..%d on %d nodes, %d azimuths; device events around the call, us: " \
           "median (min max)" % (N, B, V, MODES[0], MODES[0] + MODES[1] - 1, NPHI, NAZ)
    parent = opt("--against", None)
    if not parent:
        lines = [head + " of %d calls" % reps] + ["%-36s %9.1f (%9.1f %9.1f)" % (k, *stat(t)) for k, t in measure(reps).items()]
    else:
        rounds = int(opt("--rounds", "2"))
        tree = os.path.join(ROOT, "sos-radiative-transfer_amd", "libsosrt.so")
        pooled = {"parent": {}, "new": {}}
        for _ in range(rounds):
            for label, lib in (("parent", os.path.abspath(parent)), ("new", tree)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)],
                                   env=dict(os.environ, SOSRT_LIB=lib), capture_output=True, text=True, timeout=300)
                res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    sys.exit("the process on %s failed (exit %d):\n%s" % (lib, r.returncode, r.stderr[-2000:]))
                for k, t in json.loads(res[0][7:]).items():
                    pooled[label].setdefault(k, []).extend(t)
        lines = [head + " of %d calls in each of %d fresh processes per library, alternating" % (reps, rounds),
                 "%-36s %-32s %-32s" % ("entry/phase function", "parent", "new")]
        for k in pooled["parent"]:
            p, n = stat(pooled["parent"][k]), stat(pooled["new"][k])
            mark = "   ABOVE THE PARENT'S MAXIMUM" if n[0] > p[2] else ""
            lines.append("%-36s %9.1f (%9.1f %9.1f)   %9.1f (%9.1f %9.1f)%s" % (k, *p, *n, mark))
    print("\n".join(lines), flush=True)
    out_path = opt("--out", None)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
