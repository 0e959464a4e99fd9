"""superplus_amd/csrc/dfk_offsets.h -- the C++ restatement of GetOffsets1, its table of log binomial sums, the tail, the plan of its device
version and the layout of a.close.offsets -- against tests/offsets_oracle.py: tests/cpp/test_offsets.cc (its own main) built plain and
under -fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/offsets_cases.txt, on the larger seeded
cases and on the four fixtures' consensus written out in the same form.  It checks that the header's table equals the Python's bit for
bit in every cell, the literal transcription, and that the device-order form (candidates by bitmap, bad_window from prefix sums, a
start's last n) gives the same bytes in batches of 1, 37 and 2^30 pairs.  CPU only."""
import os
import subprocess

import pytest

from tests import offsets_cases, offsets_oracle
from tests.test_offsets_oracle import TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in offsets_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in offsets_cases.seeded() if not rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/offsets_cases.txt is offsets_cases.text(): regenerate it (python -m tests.offsets_cases) when the oracle or the generator changes"""
    assert open(offsets_cases.FILE).read() == offsets_cases.text()
    assert N_RECORDED == 8 and N_LARGER == 7 and os.path.getsize(offsets_cases.FILE) < 100000


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded cases and the four fixtures in the form of offsets_cases.txt; the Python's table as 401 x 401 doubles"""
    out = offsets_cases.text(recorded=False).splitlines()
    for case, K, which, _ in TABLE:
        r = offsets_oracle.fixture_offsets(golden_dir, case, K, which)
        out += offsets_cases.case_text(case, r["seqs"], r)
    d = tmp_path_factory.mktemp("offsets")
    (d / "more_cases.txt").write_text("\n".join(out) + "\n")
    (d / "table.bin").write_bytes(offsets_oracle.table().astype("<f8").tobytes())
    return str(d / "more_cases.txt"), str(d / "table.bin")


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_offsets")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_offsets.cc")])
    for cases, n in ((offsets_cases.FILE, N_RECORDED), (more_cases[0], N_LARGER + len(TABLE))):
        out = subprocess.run([exe, cases, more_cases[1]], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout and "401 x 401 cells equal bit for bit" in out.stdout
