#!/usr/bin/env python3
"""Where does the chunk-parallel kernel's moment mode pay?  ms per solve of columns of the headline sweep with SOSRT_SCAN_MOMENTS=0
and with the mode on, alternating handles on one box, `pairs` pairs per point; the orders that ran in the mode; whether the bits
agree.  Two tables (profiles/r08_scan_moments_threshold.txt):
  tools/ab_scan_moments.py batch [pairs [B ...]]       B columns, the mode on in every order (SOSRT_SCAN_MOMENTS_MIN=1)
  tools/ab_scan_moments.py threshold [pairs [t ...]]   the 512 columns, the mode on in the orders with at least t planned live columns
The second is the one the default of SOSRT_SCAN_MOMENTS_MIN comes from: a solve of B columns spends most of its orders far below B
live columns, so the first says what the mode costs or saves over a whole small solve, not at a live count."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np
import torch

import bench


def run(w, on, min_live=1, steps=20, reps=3):
    os.environ["SOSRT_SCAN_MOMENTS"] = "1" if on else "0"
    os.environ["SOSRT_SCAN_MOMENTS_MIN"] = str(min_live)
    dev = torch.device("cuda", 0)
    ln = bench.Lane(w, dev, 0, 256)
    best = 1e9
    try:
        ln.solve(); torch.cuda.synchronize(dev)
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(steps):
                ln.solve()
            torch.cuda.synchronize(dev)
            best = min(best, (time.perf_counter() - t0) / steps)
        return best * 1e3, ln.I.clone(), ln.s.scan_moments_stats(), ln.s.ring_moments_stats()
    finally:
        ln.close()


def point(label, w, pairs, min_live):
    off, on, same, stats, ring = [], [], True, None, None
    for i in range(pairs):
        # (the second handle of a pair measured 15-20 us faster than the first whatever it ran: the pairs take turns)
        if i % 2 == 0:
            a, Ia, _, _ = run(w, False)
            b, Ib, stats, ring = run(w, True, min_live)
        else:
            b, Ib, stats, ring = run(w, True, min_live)
            a, Ia, _, _ = run(w, False)
        off.append(a); on.append(b); same = same and bool(torch.equal(Ia, Ib))
    slower = sum(b > a for a, b in zip(off, on))
    print("%s: rows %s ms, records %s ms, records slower in %d of %d pairs, median gain %+.1f us; orders in the mode %d of %d (ring's: %d), same bits %s" % (
        label, " / ".join("%.3f" % x for x in off), " / ".join("%.3f" % x for x in on), slower, pairs,
        (np.median(off) - np.median(on)) * 1e3, stats[0], stats[1], ring[0], same), flush=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "threshold"
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    vals = [int(x) for x in sys.argv[3:]] or [8, 32, 64, 96, 128, 160, 200]
    import __graft_entry__ as ge
    ge.build()
    os.environ["SOSRT_GROUPS"] = "1"                       # one column group, as the headline runs
    w4 = bench.build_sweep(512, 200, 128, 0, 1, aerosol="eva")
    for v in vals:
        if what == "batch":
            point("B=%4d" % v, bench.take(w4, np.linspace(0, 511, v).astype(int)), pairs, 1)
        else:
            point("B= 512, records from %3d live columns up" % v, w4, pairs, v)


if __name__ == "__main__":
    main()
