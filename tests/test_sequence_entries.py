"""The argument errors of the five sequence-model entry points, replayed: tests/sequence_entry_cases.py's matrix of bad calls
(single faults and two at once) against tests/golden/sequence_entry_errors.json, the status and the text of
hssfsst_last_error() of every case as the library gave them before the entries shared their checks (recorded from the library
built at commit 91d5c27).  Equality, character for character; no device needed.  And csrc/sequence_args.hpp, where the decisions
behind those errors live, in a program of its own under sanitizers (tests/native/sequence_args_check.cpp)."""
import json
import os
import shutil
import subprocess

import pytest

from tests import sequence_entry_cases as sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")


@pytest.fixture(scope="module")
def recorded():
    with open(sec.GOLDEN) as fh:
        return json.load(fh)


def test_the_matrix_is_the_recorded_one(built_lib, recorded):
    """Same (entry, case) pairs in the same order: no case was dropped from the matrix or from the record."""
    want = [(r["entry"], r["case"]) for r in recorded]
    assert [(e, c) for e, c, _ in sec.matrix(sec.limits(built_lib))] == want
    assert {e for e, _ in want} == set(sec.ORDER) and len(want) >= 400
    assert sum(c.startswith("two:") for _, c in want) >= 150
    assert all(r["code"] != 0 or r["message"] == "" for r in recorded)


@pytest.mark.parametrize("entry", sorted(sec.ORDER))
def test_codes_and_messages_are_the_recorded_ones(built_lib, recorded, entry):
    cases = {c: kw for e, c, kw in sec.matrix(sec.limits(built_lib)) if e == entry}
    bad = []
    for r in recorded:
        if r["entry"] != entry:
            continue
        rc, msg = sec.call(built_lib, entry, cases[r["case"]])
        if (rc, msg) != (r["code"], r["message"]):
            bad.append((r["case"], (rc, msg), (r["code"], r["message"])))
    assert not bad, bad[:5]


def test_sequence_args_under_sanitizers(tmp_path):
    """csrc/sequence_args.hpp in a program of its own built with -fsanitize=address,undefined: the list check at its limits and
    with two faults at once, the table checks on NaN, -inf and clamped values in both diagonal modes, the pointer scans."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "sequence_args_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "sequence_args_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "sequence args check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
