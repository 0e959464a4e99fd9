"""superplus_amd/csrc/dfk_patch.h -- the C++ restatement of the patched graph (BuildAll, kmerize, BigKEdgeBuilder as written, the Pather
loop), the device version's order of work and the layout of a.patch.to3 -- against tests/patch_oracle.py: tests/cpp/test_patch.cc (its own
main) built plain and under -fsanitize=address,undefined and run directly on the cases recorded in tests/cpp/patch_cases.txt.  Nothing is
loaded into python under a sanitizer.  CPU only."""
import os
import subprocess

import pytest

from tests import patch_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def test_recorded_cases_are_what_the_oracle_says_now(oracle):
    """tests/cpp/patch_cases.txt is patch_cases.text(): regenerate it (python -m tests.patch_cases) when the oracle or the generator changes"""
    assert open(patch_cases.FILE).read() == patch_cases.text(oracle)
    assert os.path.getsize(patch_cases.FILE) < 100000


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, build):
    exe = os.path.join(tmp_path, "test_patch")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_patch.cc")])
    out = subprocess.run([exe, patch_cases.FILE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "13 recorded cases agree, 6 refusals refused" in out.stdout
