#!/usr/bin/env python3
"""Record the bits that tests/test_gpu_phase_builder_bits.py compares against, with the PARENT commit's library:

    SOSRT_LIB=/path/to/parent/libsosrt.so python3 tools/record_phase_builder_bits.py <parent commit> [out.json]

on an MI355X (default out: tests/golden/phase_builder_bits.json).  SHA-256 digests of the outputs of every phase-builder entry for
the cases of tests/phase_builder_cases.py.  The digests must come from a build of the commit BEFORE the change under test: the
tool refuses to run on the in-tree library, and writes the commit it was given into the file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("sos-radiative-transfer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    if len(sys.argv) < 2 or len(sys.argv[1]) != 40:
        sys.exit("usage: record_phase_builder_bits.py <40-digit commit of the library in SOSRT_LIB> [out.json]")
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "phase_builder_bits.json")
    lib = os.environ.get("SOSRT_LIB", "")
    if not lib or os.path.realpath(lib) == os.path.realpath(os.path.join(ROOT, "sos-radiative-transfer_amd", "libsosrt.so")):
        sys.exit("set SOSRT_LIB to a build of the parent commit (not the in-tree libsosrt.so)")
    import phase_builder_cases as C
    bits = {"commit": commit, "library": os.path.basename(lib), "cases": {}}
    for name in C.CASES:
        bits["cases"][name] = C.run(name)
        print(name, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
