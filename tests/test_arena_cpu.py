"""The device arena and the pass planner (superplus_amd/csrc/dfk_arena.h) are host code that never touches device
memory: they run here, on a CPU, against a backing store that only counts.  So do the decisions of the count stage's
hot-bucket fallback (superplus_amd/csrc/dfk_fallback.h): plain arithmetic over instance counts.  And so does the plan of
the counting scan (superplus_amd/csrc/dfk_scan_plan.h): plain arithmetic over read and byte counts.  And so do the plans of
the steps after the count -- pathing, the paths index, the duplicate marks (superplus_amd/csrc/dfk_paths_plan.h)."""
import os
import subprocess

import pytest


def test_cpp_arena_and_planner(tmp_path):
    """tests/cpp/test_arena.cc: placement, coalescing, shrink, the journal, pass blocks, budget and growth, adopted
    chunks, 10^5 random operations with the invariants checked after each, and one step of the default benchmark
    replayed in a 180-GB arena against the ranges the code planned before it moved into the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_arena")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_arena.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count(": ok") == 9, out.stdout + out.stderr


def test_cpp_fallback_planner(tmp_path):
    """tests/cpp/test_fallback.cc: the route of every overflowed bucket (halved, split by k-mer hash, sub-passes, HBM
    table), sub-pass words and their refinement, split groups, HBM table sizes, chunk prefixes and the hole moves of a
    part -- against tables recorded from the code before it moved into the header (instance counts on both sides of
    every threshold, four values of distinct k-mers per instance, the three switch settings, K = 40, 48, 60), and the
    properties of each over 10^4 seeded random cases."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_fallback")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_fallback.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count(": ok") == 10, out.stdout + out.stderr


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_cpp_scan_plan(tmp_path, flags):
    """tests/cpp/test_scan_plan.cc: whether the counting scan builds run keys, their classes and sub-slices, the room of a
    class slice and the scratch sizes, the pieces of a range with their halving tail, grids, LDS bytes, the number of fine
    buckets, the upload's pieces and the reads a piece completes -- against tables recorded from the code before it moved
    into the header (tests/cpp/scan_plan_expected.h: K = 40, 48, 60, bucket counts on both sides of every threshold, 1 to
    1.8x10^9 reads, every switch; the default benchmark's nine pieces among them), the properties of each over 10^4 seeded
    random cases, and the per-piece step replayed over two key slices.  A stand-alone program, also under the sanitizers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_scan_plan")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_scan_plan.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count(": ok") == 8, out.stdout + out.stderr


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_cpp_paths_plan(tmp_path, flags):
    """tests/cpp/test_paths_plan.cc: the reads a pathing batch may hold, the k-mer filter's decision, a batch's room, reads,
    need and scratch sizes, the feudal control block, the index's tail thread, range cap, ranges, key bits and mapping, the
    duplicate table's passes, the ranks' edge ranges -- against tables recorded from the code before it moved into the header
    (tests/cpp/paths_plan_expected.h: K = 40, 48, 60, both sides of every threshold, the default benchmark's figures among
    them), the properties of batches, ranges, passes, file pieces and the sharded index over 10^4 seeded random cases each, and
    the batch planner replayed over 6000 reads in 24 batches.  A stand-alone program, also under the sanitizers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_paths_plan")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_paths_plan.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count(": ok") == 16, out.stdout + out.stderr
