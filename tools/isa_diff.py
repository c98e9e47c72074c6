#!/usr/bin/env python3
"""Device-code identity check between two trees: are the gfx950 kernels of OLD and NEW the same, instruction for instruction?

  python tools/isa_diff.py HEAD~1 . chromegcn_amd/csrc/cgcn_kernels.hip chromegcn_amd/csrc/cgcn_head.hip \\
      -DCGCN_EXPERIMENT_BUILD -DKT_TIMING --rename 'k_layer_dense<(\\d+), 128, 1, =>k_layer_dense<\\1, ' \\
      --allow-only-old 'k_some_retired_kernel<'

OLD and NEW are directories (checkouts) or git revisions; a revision is materialised with `git worktree add` in a
temporary directory and removed afterwards.  Files are given relative to the tree root (default: every file of
_build.SRC).  Each file is compiled with the project's BASE_FLAGS (read from the NEW tree's chromegcn_amd/_build.py)
plus the given -D flags and `--cuda-device-only -S`.  Per function the whole instruction stream and the kernel's
.amdhsa_* descriptor block are compared after: comments dropped, symbols demangled, the caller's --rename substitutions
(regex=>replacement, applied to both sides: a removed template argument changes the mangled name), local labels
renumbered in order of appearance.  Exit status 1 when a kernel differs, is new, or is missing from NEW without matching
--allow-only-old.  Needs neither a GPU nor torch; minutes of compiler time, so it is a tool and not a test."""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_cgcn_build", os.path.join(tree, "chromegcn_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # stdlib imports only
    return mod


def compile_asm(hipcc, flags, tree, rel, out):
    cmd = [hipcc] + flags + ["-I" + os.path.join(tree, "include"), "--cuda-device-only", "-S", os.path.join(tree, rel), "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if res.returncode != 0:
        sys.exit("isa_diff: %s failed:\n%s" % (" ".join(cmd), "\n".join(
            ln for ln in res.stderr.splitlines() if "remark:" not in ln)[-4000:]))
    return out


def kernels_of(path, cxxfilt, renames):
    """assembly file -> {demangled, renamed function name: [normalised lines of its body and descriptor]}"""
    with open(path) as f:
        text = re.sub(r";[^\n]*", "", f.read())
    text = subprocess.run([cxxfilt], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
    for pat, repl in renames:
        text = re.sub(pat, repl, text)
    funcs, cur, desc = {}, None, None
    for ln in text.splitlines():
        ln = " ".join(ln.split())
        if not ln:
            continue
        m = re.match(r"\.type (.+),@function$", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif ln.startswith(".amdhsa_kernel "):
            desc = funcs.setdefault(ln[len(".amdhsa_kernel "):], [])
            desc.append(".amdhsa_kernel")
        elif ln == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc.append(ln)
        elif ln.startswith(".size ") and cur is not None:
            cur = None
        elif cur is not None and not ln.startswith((".section", ".text")):
            cur.append(ln)
    for body in funcs.values():
        labels = {}
        body[:] = [re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln) for ln in body]
    return funcs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old", help="directory or git revision")
    ap.add_argument("new", help="directory or git revision")
    ap.add_argument("files", nargs="*", help=".hip files relative to the tree root (default: all of _build.SRC)")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=V]")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=>REPL", help="applied to demangled text of both trees")
    ap.add_argument("--allow-only-old", metavar="REGEX", help="kernels that may be missing from NEW")
    ap.add_argument("--show", action="store_true", help="print the first differing line of each differing kernel")
    ap.add_argument("-j", type=int, default=os.cpu_count() or 4)
    a = ap.parse_intermixed_args()   # options may stand between the trees and the files
    renames = [tuple(r.split("=>", 1)) for r in a.rename]
    tmp = tempfile.mkdtemp(prefix="isa_diff.")
    worktrees = []
    try:
        trees = []
        for side, t in (("old", a.old), ("new", a.new)):
            if not os.path.isdir(t):
                d = os.path.join(tmp, "tree_" + side)
                subprocess.run(["git", "worktree", "add", "--detach", "-q", d, t], check=True)
                worktrees.append(d)
                t = d
            trees.append(os.path.abspath(t))
        build = load_build(trees[1])
        hipcc = build.hipcc_path() or sys.exit("isa_diff: hipcc not found")
        cxxfilt = shutil.which("llvm-cxxfilt") or os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
        if not os.path.exists(cxxfilt):
            cxxfilt = shutil.which("c++filt") or sys.exit("isa_diff: no llvm-cxxfilt / c++filt")
        flags = [f for f in build.BASE_FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("-Rpass")] + ["-D" + d for d in a.defines]
        files = a.files or [os.path.relpath(s, build.ROOT) for s in build.SRC]
        with concurrent.futures.ThreadPoolExecutor(a.j) as ex:
            jobs = {(i, rel): ex.submit(compile_asm, hipcc, flags, trees[i], rel, os.path.join(tmp, "%d_%s.s" % (i, os.path.basename(rel))))
                    for rel in files for i in (0, 1)}
            asm = {k: j.result() for k, j in jobs.items()}
        bad = False
        for rel in files:
            old, new = (kernels_of(asm[(i, rel)], cxxfilt, renames) for i in (0, 1))
            differ = sorted(k for k in old if k in new and old[k] != new[k])
            only_old = sorted(k for k in old if k not in new)
            only_new = sorted(k for k in new if k not in old)
            print("%s: %d identical, %d differ, %d only in old, %d only in new"
                  % (rel, len(old) - len(differ) - len(only_old), len(differ), len(only_old), len(only_new)))
            for tag, names in (("differs", differ), ("only in old", only_old), ("only in new", only_new)):
                for k in names:
                    print("  %s: %s" % (tag, k))
                    if a.show and tag == "differs":
                        i = next((i for i, (x, y) in enumerate(zip(old[k], new[k])) if x != y), min(len(old[k]), len(new[k])))
                        print("    line %d of %d/%d:\n    - %s\n    + %s" % (i, len(old[k]), len(new[k]), "".join(old[k][i:i + 1]), "".join(new[k][i:i + 1])))
            unexpected = [k for k in only_old if not (a.allow_only_old and re.search(a.allow_only_old, k))]
            bad = bad or bool(differ or only_new or unexpected)
        return 1 if bad else 0
    finally:
        for d in worktrees:
            subprocess.run(["git", "worktree", "remove", "--force", d])
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
