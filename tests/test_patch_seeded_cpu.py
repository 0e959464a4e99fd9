"""tests/patch_seeded.py held to tests/patch_oracle.py before it judges the device: check_invariants (an old edge read back off hb3 along
to3 from left3, hb3 holding together) on every case of tests/patch_cases.py, on the seeded zoo at K = 40, 48 and 60 and on the aligned
cases; that the zoo's plants fire and the aligned cases reach the lanes and blocks they are made for; that check_invariants refuses a
result that is wrong; and superplus_amd/csrc/dfk_patch.h (tests/cpp/test_patch.cc, its own main, built plain and under
-fsanitize=address,undefined and run directly) on the seeded and aligned cases written out with patch_cases.case_text.  CPU only."""
import os
import subprocess

import pytest

from tests import patch_cases, patch_oracle as po, patch_seeded as ps
from tests.test_patch_cpu import BUILDS, ROOT

ZOO = [(K, seed) for K in ps.KS for seed in ps.SEEDS]
ALIGNED = [(K, v) for K in ps.KS for v in ps.VARIANTS]


@pytest.fixture(scope="module")
def zoo():
    out = {}
    for K, seed in ZOO:
        g, cl = ps.seeded_case(K, seed)
        out[K, seed] = (g, cl, po.run(g, cl))
    return out


@pytest.fixture(scope="module")
def aligned():
    out = {}
    for K, v in ALIGNED:
        g, cl = ps.aligned_case(K, v)
        out[K, v] = (g, cl, po.run(g, cl))
    return out


def test_invariants_hold_on_the_hand_made_cases(oracle):
    for name, g, cl in patch_cases.all_cases(oracle):
        ps.invariants_of_result(g, cl, po.run(g, cl), name)


@pytest.mark.parametrize("K,seed", ZOO)
def test_invariants_hold_on_the_zoo_and_its_plants_fire(zoo, K, seed):
    g, cl, r = zoo[K, seed]
    what = f"zoo K={K} seed={seed}"
    ps.invariants_of_result(g, cl, r, what)
    E = len(g["edges"])
    c = r["counters"]
    assert sum(1 for e in range(E) if g["inv"][e] == e) > 0, what + ": no self-inverse old edge"
    assert sum(1 for e in range(E) if g["to_left"][e] == g["to_right"][e]) > 0, what + ": no old edge from a vertex to itself"
    assert c["short"] >= 3 and c["bits_added"] > 0 and c["single3"] > 0, what
    assert any(len(p) >= 2 for p in r["to3"]) and any(r["left3"]), what
    assert any(len(s) == K for s in g["edges"]), what + ": no one-K-mer old edge"
    # the circles: hb3 closes them (an edge from a vertex to itself that no other edge touches) and starts them elsewhere than the old edge does
    L3, R3 = r["to_left3"], r["to_right3"]
    alone = [i for i in range(len(L3)) if L3[i] == R3[i] and L3.count(L3[i]) + R3.count(L3[i]) == 2]
    assert len(alone) >= 10, what + ": hb3 has no branch-free cycles"
    assert any(len(r["to3"][e]) == 2 and r["to3"][e][0] == r["to3"][e][1] and r["to3"][e][0] in alone for e in range(E)), what + ": no old edge goes round a cycle twice"
    # cfirst: runs of equal values at both ends and inside
    assert cl[0] == b"" and cl[-1] == b"" and any(cl[i] == b"" and cl[i + 1] == b"" for i in range(1, len(cl) - 2)), what


@pytest.mark.parametrize("K,variant", ALIGNED)
def test_aligned_cases_reach_the_lanes_and_blocks(aligned, K, variant):
    g, cl, r = aligned[K, variant]
    what = f"aligned K={K} {variant}"
    ps.invariants_of_result(g, cl, r, what)
    ps.assert_coverage(g, cl, r, variant, what)
    heads = ps.head_slots(g, r)[0]
    assert set(ps.AFTER) | set(ps.BEFORE) <= set(heads), f"{what}: the long contig's heads are {heads}"


def test_invariants_refuse_what_is_wrong(zoo):
    """each a result the consumer would trip over; check_invariants must say so"""
    g, cl, r = zoo[48, 1]
    args = lambda **kw: {**dict(edges3=r["hbv"].edges, inv3=r["inv3"], to_left3=r["to_left3"], to_right3=r["to_right3"], to3=r["to3"], left3=r["left3"]), **kw}
    ps.check_invariants(g, cl, **args())
    e = next(e for e in range(len(g["edges"])) if len(r["to3"][e]) >= 2 and r["inv3"][r["to3"][e][0]] != r["to3"][e][0])
    z = next(e for e in range(len(g["edges"])) if r["left3"][e] == 0 and len(r["hbv"].edges[r["to3"][e][0]]) > 48)
    setat = lambda a, i, v: list(a[:i]) + [v] + list(a[i + 1:])
    i = r["to3"][e][0]
    wrong = {
        "left3 off by one": args(left3=setat(r["left3"], z, 1)),
        "a path cut short": args(to3=setat(r["to3"], e, r["to3"][e][:-1])),
        "a path through the inverse": args(to3=setat(r["to3"], e, setat(r["to3"][e], 0, r["inv3"][i]))),
        "an edge of hb3 changed": args(edges3=setat(r["hbv"].edges, i, r["hbv"].edges[i][:-1] + bytes([r["hbv"].edges[i][-1] ^ 1]))),
        "inv3 no involution": args(inv3=setat(r["inv3"], i, i)),
        "an end moved": args(to_right3=setat(r["to_right3"], i, r["to_left3"][i] if r["to_left3"][i] != r["to_right3"][i] else (r["to_right3"][i] + 1) % max(r["to_right3"]))),
        "a closure forgotten": None,
    }
    for name, a in wrong.items():
        with pytest.raises(AssertionError):
            if a is None: ps.check_invariants(g, cl + [patch_cases.rnd(77, 60)], **args())
            else: ps.check_invariants(g, cl, **a)
            pytest.fail("check_invariants accepts: " + name, pytrace=False)


@pytest.fixture(scope="module")
def seeded_file(zoo, aligned, tmp_path_factory):
    path = os.path.join(tmp_path_factory.mktemp("patch_seeded"), "seeded_cases.txt")
    lines = []
    for (K, seed), (g, cl, r) in zoo.items():
        lines += patch_cases.case_text(f"zoo_k{K}_s{seed}", g, cl, r)
    for (K, v), (g, cl, r) in aligned.items():
        lines += patch_cases.case_text(f"aligned_k{K}_{v}", g, cl, r)
    open(path, "w").write("\n".join(lines) + "\n")
    return path


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_on_the_seeded_cases(tmp_path, seeded_file, build):
    exe = os.path.join(tmp_path, "test_patch")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_patch.cc")])
    out = subprocess.run([exe, seeded_file], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(ZOO) + len(ALIGNED)} recorded cases agree, 0 refusals refused" in out.stdout

