#!/usr/bin/env python3
"""Compare the device code two source trees generate, kernel by kernel.

    python scripts/isa_parity.py BEFORE_TREE AFTER_TREE [--only capi.hip ...] [--jobs N]

Every entry of build.SOURCES of each tree is compiled with build.py's flags plus
`--cuda-device-only -S` into a temporary directory.  Lines naming the per-compilation
`__hip_cuid_<hash>` symbol are dropped (the hash covers the source text).  Per translation unit
the report says "identical", or lists the kernels whose text differs with their register,
scratch and code-size figures before -> after.  Exit status 1 if anything differs.

A refactor of device source that only moves statements into __forceinline__ functions leaves
every unit identical; a different formulation of the same arithmetic usually does not.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FIGURES = (("NumVgprs", r"^; NumVgprs: (\d+)"), ("NumSgprs", r"^; (?:Total)?NumSgprs: (\d+)"),
           ("ScratchSize", r"^; ScratchSize: (\d+)"), ("codeLenInByte", r"^; codeLenInByte = (\d+)"))


def load_build(tree: str):
    path = os.path.join(tree, "project_morpheus_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(build, flags, src: str, out: str) -> str:
    cmd = [build._hipcc()] + flags + ["--cuda-device-only", "-S",
                                      os.path.join(build.CSRC, src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")
    with open(out) as f:
        return "".join(line for line in f if "__hip_cuid_" not in line)


def functions(text: str) -> dict:
    """name -> text, split at the `.type NAME,@function` lines; what precedes the first function
    and the metadata block at the end are kept under names of their own."""
    parts = {}
    head, _, meta = text.partition("\t.amdgpu_metadata")
    parts["(metadata)"] = meta
    pieces = re.split(r"^\t\.type\t(\S+),@function.*$", head, flags=re.M)
    parts["(file scope)"] = pieces[0]
    for name, body in zip(pieces[1::2], pieces[2::2]):
        parts[name] = body
    return parts


def figures(body: str) -> dict:
    out = {}
    for key, pat in FIGURES:
        m = re.search(pat, body, flags=re.M)
        out[key] = m.group(1) if m else "-"
    return out


def demangle(names: list) -> dict:
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
        return dict(zip(names, r.stdout.splitlines()))
    except OSError:
        return {n: n for n in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--only", nargs="*", default=None, help="translation units to compare")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()

    own = load_build(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    trees = [load_build(os.path.abspath(t)) for t in (args.before, args.after)]
    # a tree from before build.compile_flags existed is compiled with this tree's flags
    flags = [getattr(b, "compile_flags", own.compile_flags)() for b in trees]
    units = [s for s in trees[1].SOURCES if args.only is None or s in args.only]
    differing = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(args.jobs) as pool:
        jobs = {}
        for s in units:
            for i, b in enumerate(trees):
                if s in b.SOURCES:
                    out = os.path.join(tmp, f"{i}_{s}.s")
                    jobs[s, i] = pool.submit(assemble, b, flags[i], s, out)
        print(f"flags: {' '.join(flags[1])} --cuda-device-only -S")
        for s in units:
            if (s, 0) not in jobs:
                print(f"{s}: only in the second tree")
                differing += 1
                continue
            before, after = functions(jobs[s, 0].result()), functions(jobs[s, 1].result())
            kernels = sum(1 for n in after if not n.startswith("("))
            names = [n for n in dict.fromkeys(list(before) + list(after))
                     if before.get(n) != after.get(n)]
            if not names:
                print(f"{s}: identical ({kernels} functions)")
                continue
            differing += 1
            print(f"{s}: {len(names)} of {kernels} functions differ")
            pretty = demangle(names)
            for n in names:
                if n not in before or n not in after:
                    print(f"  {pretty[n]}: only {'after' if n in after else 'before'}")
                    continue
                fb, fa = figures(before[n]), figures(after[n])
                print(f"  {pretty[n]}: " +
                      ", ".join(f"{k} {fb[k]} -> {fa[k]}" for k, _ in FIGURES))
    print("verdict: " + ("every translation unit identical" if not differing
                         else f"{differing} translation unit(s) differ"))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
