#!/usr/bin/env python3
"""Record the bits that tests/test_gpu_driver_bits.py compares against, with the Python package of an EARLIER commit on the
in-tree library (the drivers are host code; the library is the same on both sides):

    git archive <commit> sos-radiative-transfer_amd/sosrt | tar -x -C <dir>
    SOSRT_LIB=$PWD/sos-radiative-transfer_amd/libsosrt.so python3 tools/record_driver_bits.py \\
        <dir>/sos-radiative-transfer_amd <commit hash> [out.json]

on an MI355X (default out: tests/golden/driver_bits.json).  Where the commit under test changes the library too (the cases that
call the `Solver` stages directly check it, not a driver), take a full export of the earlier commit built with its own build(), its
package as <dir> and its library as SOSRT_LIB: the digests of the cases recorded before must come out unchanged.  SHA-256 digests of every output of the cases of tests/driver_cases.py.
The tool refuses to write when the package it imported is the in-tree one, or when a column of any case has a non-zero status
(it names the cases: shrink their optical depth until the earlier commit converges)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    package_dir, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden", "driver_bits.json")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, package_dir)
    import sosrt
    in_tree = os.path.realpath(os.path.join(ROOT, "sos-radiative-transfer_amd", "sosrt"))
    if os.path.realpath(os.path.dirname(sosrt.__file__)) == in_tree:
        sys.exit("sosrt was imported from the in-tree package: give the directory of an earlier commit's export")
    import driver_cases as C
    bits = {"commit": commit, "cases": {}}
    bad = []
    for name in C.CASES:
        try:
            bits["cases"][name], status = C.run(name)
        except (IndexError, RuntimeError) as e:      # (what the flux drivers raise for a status of their own; anything else ends the run)
            if isinstance(e, RuntimeError) and "did not converge" not in str(e):
                raise
            status = [repr(e)]
        print(name, "status", status if any(status) else "0", flush=True)
        if any(status):
            bad.append(name)
    if bad:
        sys.exit("not written: a non-zero status in %s" % ", ".join(bad))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
