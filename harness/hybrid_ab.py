#!/usr/bin/env python3
"""A/B of whole bench.py runs for the hybrid radix path (output kept as
profiles/hybrid_ab.txt).

Each variant is a set of environment variables for a plain `python bench.py <args>` child
(LABSORT_LIBRARY=<another build of liblabsort.so> for the parent commit, LABSORT_RADIX_HYBRID=0/2
for the classic / hybrid path of this build).  The variants run in turn, repetition by
repetition, in one session; the result line's ms_per_step, median [min, max] over the
repetitions, and the timed pass class's time per launch.

  python harness/hybrid_ab.py --reps 5 --variant parent:LABSORT_LIBRARY=/path/liblabsort.so \\
      --variant new: -- --dist mod1000"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], help="name:VAR=value,VAR=value")
    ap.add_argument("--out", default="")
    ap.add_argument("bench_args", nargs="*")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else sys.stdout
    variants = {}
    for v in a.variant:
        name, _, envs = v.partition(":")
        variants[name] = dict(e.split("=", 1) for e in envs.split(",") if e)
    ms = {k: [] for k in variants}
    kern = {k: [] for k in variants}
    for _ in range(a.reps):
        for name, env in variants.items():
            r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *a.bench_args], env={**os.environ, **env},
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"hybrid_ab: {name}: bench.py exited {r.returncode}\n{r.stderr[-2000:]}")
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            ms[name].append(line["ms_per_step"])
            kern[name].append(line.get("kernel_ms"))
    print(f"# bench.py {' '.join(a.bench_args) or '(plain)'}: ms_per_step, {a.reps} alternating runs, median [min, max]; "
          f"last run's kernel_ms", file=out)
    for name in variants:
        t = ms[name]
        print(f"{name:>10}  {statistics.median(t):8.4f} [{min(t):8.4f}, {max(t):8.4f}]  spread {max(t) - min(t):.4f}  "
              f"kernel_ms {kern[name][-1]}", file=out)
    out.flush()


if __name__ == "__main__":
    main()
