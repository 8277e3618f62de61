"""CPU test of labsort_radix_counting (include/labsort.h): exported, listed, bound, and 0 without a
workspace.  No kernel is launched and no device is touched: the call returns before its first HIP call."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAME = "labsort_radix_counting"


def test_symbol_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAME in ls.C_SYMBOLS
    assert NAME + "(" in open(os.path.join(REPO, "include", "labsort.h")).read()
    assert callable(ls.radix_counting)


def test_null_workspace_is_full_count(ls):
    L = ls.lib
    for n in (0, 1, 32768, 32769, 1 << 20, 1 << 28, 1 << 40):
        assert L.labsort_radix_counting(None, n, None) == 0
    assert L.labsort_radix_counting(1 << 40, 0, None) == 0  # no keys
    assert L.labsort_radix_counting(1 << 40, 32768, None) == 0  # one tile: no counting launches
