"""The Python drivers (sosrt.main, forcing, thermal, bands) against the bits of an earlier commit's package on the same library:
SHA-256 digests of every output of the cases of tests/driver_cases.py, recorded by tools/record_driver_bits.py
(tests/golden/driver_bits.json).  The drivers decide what is uploaded, which library calls run in which order and what is put back
on the cached handle -- not a column's arithmetic: every digest must be the recorded one."""
import json
import os
import subprocess

import pytest

import driver_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "driver_bits.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recorded_bits_are_complete_and_an_earlier_commits():
    """(no GPU) The golden file holds every case and names the commit of the package that gave the bits: not the one under test."""
    g = _golden()
    assert set(g["cases"]) == set(C.CASES)
    assert all(len(d) == 64 for case in g["cases"].values() for d in case.values()) and all(g["cases"].values())
    commit = g["commit"]
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef")
    git = lambda *a: subprocess.run(("git",) + a, cwd=HERE, capture_output=True, text=True)
    head = git("rev-parse", "HEAD")
    if head.returncode == 0:                                  # (an export without history has no HEAD to compare with)
        # (with uncommitted edits to the package, what is under test is not HEAD either)
        dirty = git("status", "--porcelain", "--", os.path.join(os.pardir, "sos-radiative-transfer_amd", "sosrt")).stdout.strip()
        assert dirty or commit != head.stdout.strip()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(C.CASES))
def test_driver_has_the_recorded_bits(case):
    digests, status = C.run(case)
    assert not any(status), status
    assert digests == _golden()["cases"][case]
