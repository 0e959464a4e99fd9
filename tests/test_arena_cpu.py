"""The device arena and the pass planner (superplus_amd/csrc/dfk_arena.h) are host code that never touches device
memory: they run here, on a CPU, against a backing store that only counts.  So do the decisions of the count stage's
hot-bucket fallback (superplus_amd/csrc/dfk_fallback.h): plain arithmetic over instance counts."""
import os
import subprocess


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
