#!/usr/bin/env python3
"""asm_same.py [--allow-new] OLD.s NEW.s -- are the kernels of two device-only assembly listings of kth.hip
(hipcc --cuda-device-only -S, the Makefile's flags) the same instruction streams?  Comments,
directives and block labels are dropped, the function number in a branch target too; what is
left is compared line by line, kernel by kernel, and one `same` or `DIFFERS` line is printed for
each.  Names are compared demangled, the old k_tkm_short<KT, B, S> as k_kth_short<KT, B, S, true>
the old k_kth_short<KT, B, S> as <KT, B, S, false> and the old k_tkm_apply<KT> as
k_tkm_apply<KT, false>.  Exit status 1 unless every kernel of either file is in the
other and the same; with --allow-new a kernel that only NEW has is listed as `new` and does not count
(a feature adds kernels and must leave the others alone)."""
import re
import subprocess
import sys


def kernels(path):
    body, name = {}, None
    for line in open(path):
        code = line.split(";")[0].rstrip()
        word = code.strip()
        if not word or word.startswith(".") or word.startswith("//"):
            continue  # blank, comment, directive or block label (.LBB3_7:)
        if word.endswith(":") and not code[0].isspace():
            name = word[:-1]
            body[name] = []
        elif name:
            body[name].append(re.sub(r"\.LBB\d+_", ".LBB_", word))
    plain = subprocess.run(["c++filt"], input="\n".join(body), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, long_name in zip(body, plain):
        found = re.search(r"(k_\w+)(?:<([^>]*)>)?\(", long_name)
        if not found:
            continue  # (a data label)
        kernel, targs = found.groups()
        if kernel == "k_tkm_short":
            kernel, targs = "k_kth_short", targs + ", true"
        elif kernel == "k_kth_short" and targs.count(",") == 2:
            targs += ", false"
        elif kernel == "k_tkm_apply" and "," not in targs:
            targs += ", false"
        out[f"{kernel}<{targs}>" if targs else kernel] = body[mangled]
    return out


allow_new = "--allow-new" in sys.argv[1:]
paths = [a for a in sys.argv[1:] if a != "--allow-new"]
old, new = kernels(paths[0]), kernels(paths[1])
bad = 0
for k in sorted(set(old) | set(new)):
    if allow_new and k not in old:
        print(f"new  {k}  ({len(new[k])} instructions)")
        continue
    if k not in old or k not in new:
        print(f"ONLY IN {'OLD' if k in old else 'NEW'}  {k}")
    elif old[k] != new[k]:
        at = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
        print(f"DIFFERS  {k}  ({len(old[k])} / {len(new[k])} instructions, first at {at})")
    else:
        print(f"same  {k}  ({len(new[k])} instructions)")
        continue
    bad += 1
print(f"{len(set(old) | set(new))} kernels, {bad} not the same")
sys.exit(1 if bad else 0)
