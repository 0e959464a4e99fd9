"""superplus_amd/csrc/dfk_translate.h -- the C++ restatement of TranslatePaths (the rule as written, the pieces host and kernels share, the
bound, the refusals) -- against tests/translate_oracle.py: tests/cpp/test_translate.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly on the cases recorded in tests/cpp/translate_cases.txt.  Nothing is loaded into python under a
sanitizer.  CPU only."""
import os
import subprocess

import pytest

from tests import translate_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/translate_cases.txt is translate_cases.text(): regenerate it (python -m tests.translate_cases) when the oracle or the
    generator changes"""
    assert open(translate_cases.FILE).read() == translate_cases.text()
    assert os.path.getsize(translate_cases.FILE) < 100000


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, build):
    exe = os.path.join(tmp_path, "test_translate")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_translate.cc")])
    out = subprocess.run([exe, translate_cases.FILE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "12 recorded cases agree, 12 refusals refused" in out.stdout
