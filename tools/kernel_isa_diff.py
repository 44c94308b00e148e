#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two trees, kernel by kernel.

  tools/kernel_isa_diff.py OLD_TREE NEW_TREE [--allow NAME ...] [--only FILE.hip ...] [--differing]

Every storage-benchmarks_amd/csrc/*.hip of both trees is compiled with that
tree's Makefile flags plus --cuda-device-only -S (no GPU needed).  Generated
.inc files are taken from each tree's storage-benchmarks_amd/build/, so both
trees must have been built once.  Before the comparison .file and .ident
lines, comments and the per-build __hip_cuid_* symbol are dropped and the
numbers of local labels (.LBBn_m and friends) normalised.

Prints `same` or `differs` per device function (kernels with their
descriptors; the rest of a file, data and metadata, as one more entry) and
exits non-zero when anything differs that no --allow NAME covers.  NAME is a
substring of the (mangled) symbol, e.g. k_scrub_finalise.  --differing prints
only the entries that differ, and per file how many are the same.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ENGINE = "storage-benchmarks_amd"


def make_var(text, name):
    m = re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M)
    if not m:
        sys.exit(f"no {name} in the Makefile")
    return m.group(1).strip()


def compile_asm(tree, hip, out):
    eng = os.path.join(tree, ENGINE)
    with open(os.path.join(eng, "Makefile")) as f:
        mk = f.read()
    flags = make_var(mk, "HIPFLAGS").replace("$(ARCH)", make_var(mk, "ARCH")).split()
    cmd = [os.environ.get("HIPCC", make_var(mk, "HIPCC")), *flags, "-Ibuild", "--cuda-device-only", "-S",
           os.path.join("csrc", hip), "-o", out]
    r = subprocess.run(cmd, cwd=eng, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {hip} does not compile (is the tree built? the .inc files come from its build/)\n"
                 + r.stderr[-2000:])
    with open(out) as f:
        return f.read()


LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def normalise(asm):
    """Lines without what differs from build to build; the indentation stays
    (the metadata is YAML), other runs of blanks become one."""
    out = []
    for line in asm.splitlines():
        s = line.strip()
        if not s or s.startswith((";", "//", ".file", ".ident")) or "__hip_cuid_" in s:
            continue
        if '"' not in s:
            s = s.split(";", 1)[0].rstrip()
        s = LOCAL.sub(lambda m: f".L{m.group(1)}{m.group(2) or ''}", s)
        out.append(line[: len(line) - len(line.lstrip())] + " ".join(s.split()))
    return out


def split(lines):
    """{symbol: [lines]}: a function from its label to its .size line, with its
    `.set symbol.*` resource lines and, for a kernel, its .amdhsa_kernel block
    and its entry in the metadata; everything else under ''."""
    parts = {"": []}
    funcs = {ln.split()[1].split(",")[0] for ln in lines
             if ln.lstrip().startswith(".type") and ln.endswith("@function")}
    cur, entry = "", None  # entry: the lines of a metadata entry whose kernel is not known yet
    for ln in lines:
        s = ln.lstrip()
        if entry is not None:  # inside amdhsa.kernels
            if ln.startswith("  - ") or not ln.startswith("  "):
                parts.setdefault(cur, []).extend(entry)
                cur, entry = "", [] if ln.startswith("  - ") else None
            if entry is not None:
                entry.append(ln)
                if s.startswith(".name:"):
                    cur = s.split()[1]
                continue
        if ln == "amdhsa.kernels:":
            entry = []
        elif cur == "" and s.endswith(":") and s[:-1] in funcs:
            cur = s[:-1]
        elif cur == "" and s.startswith(".amdhsa_kernel "):
            cur = s.split()[1]
        own = s.split()[1].split(".")[0] if s.startswith(".set ") and s.split()[1].split(".")[0] in funcs else cur
        parts.setdefault(own, []).append(ln)
        if s.startswith(".size " + cur + ",") or s == ".end_amdhsa_kernel":
            cur = ""
    return parts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--allow", nargs="*", default=[], metavar="NAME", help="symbols that may differ")
    ap.add_argument("--only", nargs="*", metavar="FILE", help="compare these .hip files only (default: all)")
    ap.add_argument("--differing", action="store_true", help="print only what differs, and a count of the rest")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()

    def hips(tree):
        return sorted(f for f in os.listdir(os.path.join(tree, ENGINE, "csrc")) if f.endswith(".hip"))

    files = hips(args.old_tree)
    if hips(args.new_tree) != files:
        sys.exit(f"the trees hold different .hip files: {files} / {hips(args.new_tree)}")
    if args.only:
        files = [f for f in files if f in args.only]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {(side, f): pool.submit(compile_asm, os.path.abspath(tree), f, os.path.join(tmp, f"{side}_{f}.s"))
                for side, tree in (("old", args.old_tree), ("new", args.new_tree)) for f in files}
        for f in files:
            old, new = (split(normalise(jobs[(side, f)].result())) for side in ("old", "new"))
            nsame = 0
            for sym in sorted(set(old) | set(new)):
                same = old.get(sym) == new.get(sym)
                allowed = not same and any(a in sym for a in args.allow if sym)
                bad += not same and not allowed
                nsame += same
                if same and args.differing:
                    continue
                print(f"{f}: {sym or '(data and metadata)'}: "
                      f"{'same' if same else 'differs (allowed)' if allowed else 'differs'}")
            if args.differing:
                print(f"{f}: {nsame} entries the same")
    print("no unexpected difference" if not bad else f"{bad} unexpected difference(s)", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
