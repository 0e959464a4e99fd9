"""superplus_amd/csrc/dfk_closer.h -- the C++ restatement of the closers' read sets per edge, the plan of its device version and the
layouts of the four files a.close.* -- against tests/closer_oracle.py: tests/cpp/test_closer.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/closer_cases.txt, on the larger seeded cases and
on graph_pathy2_k48 and graph_frag_k48 written out in the same form.  It checks the literal transcription, the per-pair composition
identity, and that the device version's order of work gives the same tables under every range cap.  CPU only."""
import os
import subprocess

import pytest

from tests import closer_cases, closer_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in closer_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in closer_cases.seeded() if not rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/closer_cases.txt is closer_cases.text(): regenerate it (python -m tests.closer_cases) when the oracle or the generator changes"""
    assert open(closer_cases.FILE).read() == closer_cases.text()
    assert N_RECORDED == 7 and N_LARGER == 2 and os.path.getsize(closer_cases.FILE) < 100000


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded cases, and pathy2 and frag -- the index and the marks the reference's own -- in the form of closer_cases.txt"""
    out = closer_cases.text(recorded=False).splitlines()
    for case, K, which in (("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag")):
        i = closer_oracle.fixture_inputs(golden_dir, case, K, which)
        assert i["reference_index"] and i["reference_dup"]
        assert i["index"] == closer_oracle.make_index(i["paths"], len(i["inv"]))         # the header builds its own index: the same lists
        out += closer_cases.case_text(case, i, closer_oracle.fixture_closer(golden_dir, case, K, which))
    path = tmp_path_factory.mktemp("closer") / "more_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_closer")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_closer.cc")])
    for cases, n in ((closer_cases.FILE, N_RECORDED), (more_cases, N_LARGER + 2)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
