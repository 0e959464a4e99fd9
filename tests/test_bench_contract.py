"""bench.py's command line (the driver's contract) and its refusal to run without a GPU: the library has no CPU path
and the bench must say so instead of measuring something else.  --dump-outputs: what the timed path computed, exactly,
the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_the_driver_passes_exist():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in out.stdout


@pytest.mark.skipif(torch.cuda.is_available(), reason="this is the no-GPU behaviour")
def test_refuses_to_run_without_a_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "needs a GPU" in (out.stderr + out.stdout)
    assert "{" not in out.stdout                                    # no JSON line: nothing was measured


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True,
                         timeout=300, env=env)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


class _Counted:
    """What dump_outputs reads from a context, with a dictionary held in a given order."""

    def __init__(self, n_solid, n_reads, order_seed=None):
        from superplus_amd.dfk import ENTRY_DTYPE
        rng = np.random.default_rng(5)
        e = np.zeros(n_solid, ENTRY_DTYPE)
        e["w0"] = rng.integers(0, 2 ** 64 - 1, n_solid, dtype=np.uint64, endpoint=True)
        e["w1"] = rng.integers(0, 2 ** 32, n_solid, dtype=np.uint64)
        e["count_ctx"] = rng.integers(0, 2 ** 32, n_solid, dtype=np.uint64)
        e["bc"] = rng.integers(-9, 9, n_solid)                                   # (unspecified after a count: not dumped)
        self.entries = e if order_seed is None else e[np.random.default_rng(order_seed).permutation(n_solid)]
        self.lens = rng.integers(0, 152, n_reads).astype(np.uint32)
        self.hist = np.zeros(4000, np.int64); self.hist[[3, 4, 77, 3999]] = [10 ** 15, 5, 1, 2]

    def stats(self):
        return dict(n_reads=len(self.lens), n_inst=2 ** 52 + 1, n_distinct=3 * len(self.entries), n_solid=len(self.entries))

    def spectrum(self):
        return self.hist

    def digest(self):
        return 2 ** 64 - 3, 0x0123456789ABCDEF

    def solid_unsorted(self):
        return self.entries.copy()

    def good_lens(self):
        return self.lens


def _dump(ctx, d):
    import bench
    bench.dump_outputs(ctx, str(d))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}, sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def _u64(lo, hi):
    return lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))


@pytest.mark.parametrize("n_solid,n_reads", [(5000, 7000), (3_000_000, 2_500_000)])
def test_dump_outputs_is_exact_bounded_and_independent_of_the_device_order(tmp_path, n_solid, n_reads):
    got, nbytes = _dump(_Counted(n_solid, n_reads), tmp_path / "a")
    again, _ = _dump(_Counted(n_solid, n_reads, order_seed=1), tmp_path / "b")
    assert nbytes <= 64 << 20
    assert got.keys() == again.keys() == {"counts", "spectrum", "solid_digest", "solid_sample", "good_lens"}
    for k in got:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], again[k]), k
    ctx = _Counted(n_solid, n_reads)
    assert got["counts"].tolist() == [n_reads, 2 ** 52 + 1, 3 * n_solid, n_solid]
    assert got["spectrum"].tolist() == [[3, 10 ** 15], [4, 5], [77, 1], [3999, 2]]
    dg = got["solid_digest"]
    assert (int(_u64(dg[0], dg[1])), int(_u64(dg[2], dg[3]))) == ctx.digest()
    s = got["solid_sample"]
    assert len(s) == min(n_solid, 1 << 19)
    w0, w1 = _u64(s[:, 0], s[:, 1]), _u64(s[:, 2], s[:, 3])
    assert np.all((w0[1:] > w0[:-1]) | ((w0[1:] == w0[:-1]) & (w1[1:] > w1[:-1])))           # ascending (w0, w1)
    e = np.sort(ctx.entries, order=("w0", "w1"))
    at = np.searchsorted(e["w0"], w0)
    assert np.array_equal(e["w0"][at], w0) and np.array_equal(e["w1"][at], w1) and np.array_equal(e["count_ctx"][at], s[:, 4])
    g = got["good_lens"]
    idx = g[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and len(idx) == min(n_reads, 1 << 20)
    assert np.array_equal(ctx.lens[idx], g[:, 1])


def test_full_is_an_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_dumped_outputs_repeat_and_steps_are_the_timed_steps(tmp_path):
    """Two runs with other --steps / --warmup: the timed loop runs --steps times, and what the last step computed is the same."""
    small = ["--genome-mb", "2", "--pairs", "200000", "--no-cpu-baseline", "--no-extras"]
    runs = []
    for steps, warmup in ((1, 0), (3, 1)):
        d = tmp_path / f"s{steps}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                              *small, "--dump-outputs", str(d)], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and len(line["step_ms_each_rank0"]) == steps
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert got["counts"][1] == line["counts_rank0"]["n_inst"] and got["counts"][3] == line["counts_rank0"]["n_solid"] > 0
        assert got["spectrum"][:, 1].sum() == line["counts_rank0"]["n_solid"]
        assert len(got["solid_sample"]) == min(line["counts_rank0"]["n_solid"], 1 << 19)
        runs.append(got)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


@pytest.mark.gpu
def test_a_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """Without --full the line carries the headline figure and what the timed steps report; --full adds the CPU baseline
    with its parity check and the reported-only legs asked for."""
    small = ["--gpus", "1", "--steps", "1", "--warmup", "0", "--genome-mb", "2", "--pairs", "200000"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--legs", "ksweep", "--extra-steps", "1", "--cpu-sample-reads", "20000"])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *small, *extra], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        lines[name] = json.loads(out.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["unit"] == "k-mers/s" and line["higher_is_better"] is True and line["dtype"] == "u64" and line["steps"] == 1
        assert line["value"] > 0 and line["ms_per_step"] > 0
    for k in ("n_reads", "n_inst", "n_records", "n_buckets", "n_distinct", "n_solid", "n_passes"):
        assert plain["counts_rank0"][k] == full["counts_rank0"][k], k
    assert not {"cpu_baseline", "cpu_baseline_error", "parity_check", "extra", "df_stage"} & plain.keys()
    assert full["cpu_baseline"]["value"] > 0 and full["parity_check"]["status"] == "ok"
    sweep = full["extra"]["k_sweep"]
    assert sorted(sweep) == ["40", "48", "60"] and all("error" not in v for v in sweep.values())
    assert "error" in full["df_stage"]                                             # (not among the legs asked for)
