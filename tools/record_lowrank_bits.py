#!/usr/bin/env python3
"""Record the bits that tests/test_gpu_lowrank_stream.py compares against, with the PARENT commit's library:

    SOSRT_LIB=$PWD/sos-radiative-transfer_amd/libsosrt_parent.so python3 tools/record_lowrank_bits.py [out.json]

on an MI355X (default out: tests/golden/lowrank_stream_bits.json).  SHA-256 digests of Solver.source(X) and of whole solves (I, n)
for the cases of tests/lowrank_stream_cases.py -- inputs from fixed seeds.  The digests must come from a build of the commit BEFORE
the change under test: the tool refuses to run on the in-tree library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("sos-radiative-transfer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lowrank_stream_bits.json")
    lib = os.environ.get("SOSRT_LIB", "")
    if not lib or os.path.realpath(lib) == os.path.realpath(os.path.join(ROOT, "sos-radiative-transfer_amd", "libsosrt.so")):
        sys.exit("set SOSRT_LIB to a build of the parent commit (not the in-tree libsosrt.so)")
    import lowrank_stream_cases as C
    for k in C.KNOBS:
        os.environ.pop(k, None)
    bits = {"library": os.path.basename(lib), "source": {}, "conv": {}, "tilings": {}}
    for shape in C.SOURCE_SHAPES:
        bits["source"][shape] = {atm: C.source_case(shape, atm) for atm in C.ATMOSPHERES}
        print("source", shape, flush=True)
    for key, env in (("moments", {}), ("moments_0", {"SOSRT_RING_MOMENTS": "0"})):
        os.environ.update(env)
        C.fresh()
        r = C.conv_solve()
        bits["conv"][key] = dict(C.solve_digests(r), orders=[int(x) for x in r.n])
        C.fresh()
        for k in env:
            os.environ.pop(k)
        print("conv", key, bits["conv"][key]["orders"], flush=True)
    for atm in C.ATMOSPHERES:
        C.fresh()
        r = C.tilings_solve(atm)
        bits["tilings"][atm] = dict(C.solve_digests(r), orders=[int(r.n.min()), int(r.n.max())])
        C.fresh()
        print("tilings", atm, bits["tilings"][atm]["orders"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
