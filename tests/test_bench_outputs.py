"""bench.py --dump-outputs / --full.  CPU tests: the dump's sampling (fixed positions, both
ends kept, exact values, the element budget).  GPU tests: a plain run honours --steps, prints
only the headline's fields and dumps the sorted keys; --full adds the checks and the legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_mod():
    import bench
    return bench


def test_dump_small_array_is_whole_and_exact(tmp_path):
    import torch
    b = _bench_mod()
    words = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    t = torch.from_numpy(words.view(np.int32).copy())
    b.dump_outputs(torch, str(tmp_path / "d"), {"keys": t})
    got = np.load(tmp_path / "d" / "keys.npy")
    assert got.dtype == np.float64
    assert np.array_equal(got, words.astype(np.float64))  # uint32 values, not the int32 view


def test_dump_large_array_is_a_fixed_sample(tmp_path):
    import torch
    b = _bench_mod()
    n = b.DUMP_ELEMS + 12345
    t = torch.arange(n, dtype=torch.int32)  # value == position: the dump shows the positions
    for d in ("a", "b"):
        b.dump_outputs(torch, str(tmp_path / d), {"keys": t, "values": t})
    ka, va = np.load(tmp_path / "a" / "keys.npy"), np.load(tmp_path / "a" / "values.npy")
    assert ka.size == va.size == b.DUMP_ELEMS // 2  # the budget is shared by the arrays
    assert ka.nbytes + va.nbytes <= 64 * 10**6
    assert ka[0] == 0 and ka[-1] == n - 1 and bool((np.diff(ka) >= 0).all())
    assert np.array_equal(ka, va)  # the same positions in every array of a run
    assert np.array_equal(ka, np.load(tmp_path / "b" / "keys.npy"))  # and in every run


def test_dump_budget_is_shared_by_the_ranks(tmp_path):
    """8 ranks, one array each: every file holds an eighth of the budget, 32 MiB in all"""
    import torch
    b = _bench_mod()
    t = torch.arange(b.DUMP_ELEMS, dtype=torch.int32)
    for r in range(8):
        b.dump_outputs(torch, str(tmp_path), {f"keys_rank{r}": t}, world=8)
    files = [np.load(tmp_path / f"keys_rank{r}.npy") for r in range(8)]
    assert all(f.size == b.DUMP_ELEMS // 8 and f[0] == 0 and f[-1] == b.DUMP_ELEMS - 1 for f in files)
    assert sum(f.nbytes for f in files) <= 64 * 10**6


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def _run(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"merge", "config1", "config2", "pairs", "host_path"}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_sorted_keys(tmp_path, oracle):
    """2^23 keys (above the dump's budget: the sampled path), 3 timed steps"""
    import torch
    b = _bench_mod()
    lg, steps = 23, 3
    line = _run(["--steps", str(steps), "--warmup", "1", "--log2n", str(lg), "--dump-outputs", str(tmp_path)])
    assert HEADLINE <= set(line) and not (FULL_ONLY & set(line))
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mkeys/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["value"] == pytest.approx((1 << lg) / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    # the timed region ran exactly `steps` sorts: four 8-bit passes each, every pass one launch of the dominant kernel
    assert line["roofline"]["launches"] == 4 * steps
    assert line["cpu_baseline"] is None and line["verified"] is None and "copy_ceiling" not in line["roofline"]
    assert sorted(os.listdir(tmp_path)) == ["keys.npy"]
    got = np.load(tmp_path / "keys.npy")
    assert got.dtype == np.float64 and got.size == b.DUMP_ELEMS
    expect = oracle.sort_u32(oracle.gen(1 << lg, b.SEED + 3, "u32"))
    b.dump_outputs(torch, str(tmp_path / "pos"), {"keys": torch.arange(1 << lg, dtype=torch.int32)})
    pos = np.load(tmp_path / "pos" / "keys.npy").astype(np.int64)  # value == position: the sampled positions
    assert pos[0] == 0 and pos[-1] == (1 << lg) - 1
    assert np.array_equal(got, expect[pos].astype(np.float64))


@pytest.mark.gpu
def test_plain_pairs_run_dumps_keys_and_values(tmp_path, oracle):
    b = _bench_mod()
    lg = 16
    _run(["--steps", "1", "--warmup", "0", "--log2n", str(lg), "--algo", "pairs", "--dump-outputs", str(tmp_path)])
    k, v = np.load(tmp_path / "keys.npy"), np.load(tmp_path / "values.npy")
    src = oracle.gen(1 << lg, b.SEED + 3, "u32")
    ek, ev = oracle.stable_sort_pairs(src, np.arange(1 << lg, dtype=np.uint32), "u32")
    assert np.array_equal(k, ek.astype(np.float64)) and np.array_equal(v, ev.astype(np.float64))


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_legs(tmp_path):
    line = _run(["--full", "--no-host-path", "--no-cpu-baseline", "--steps", "2", "--warmup", "1", "--log2n", "22",
                 "--dump-outputs", str(tmp_path)])
    assert HEADLINE <= set(line) and {"merge", "config1", "config2", "pairs"} <= set(line)
    assert line["verified"].startswith("sorted permutation") and line["steps"] == 2
    assert line["roofline"]["copy_ceiling"]["verified"] is True
    assert line["merge"]["verified"] and line["config1"]["verified"] == "fixture"
    assert np.load(tmp_path / "keys.npy").size == 1 << 22
