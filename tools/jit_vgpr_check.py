#!/usr/bin/env python3
"""Do the generated kernels' compiler-allocated instructions keep out of the
accumulators?

  tools/jit_vgpr_check.py [TREE]

k_rs_jit* (accumulators v64..v127), k_rs_jitw* (v40..v40+8R-1) and k_rs_kara
(v40..v167) hand the compiler v0..v63 and v0..v39 with amdgpu_num_vgpr, and
only asm and generated code may touch the accumulators.  The attribute is no
hard limit on gfx950: a request below what the most waves per SIMD leave each
wave (64 registers) is raised to that, so a kernel that needs more than its
share gets it, silently, inside the accumulators.  This compiles
csrc/rs_jit.hip of TREE (default: this one; its build/ must hold the generated
.inc files) to gfx950 assembly with the Makefile's flags (no GPU needed) and
lists, per kernel, every instruction outside an asm statement that names an
accumulator register.  Exits non-zero when there is one, when no kernel was
seen, or when one of the kernel families above is missing from the assembly.
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_isa_diff as kid  # noqa: E402

# the templates' symbols go on with I<arguments>, k_rs_kara's (no template)
# with E<parameter types>
KERNEL = re.compile(r"^(_ZN5rsgpu4jitk\d+k_rs_(?:jit(w?)(?:_scrub|_locate|_repair|_correct|_degraded|_batch)?I|karaE)\S*):")
FAMILIES = ("k_rs_jitI", "k_rs_jitwI", "k_rs_karaE")  # each must be seen at least once
WIDE_R = re.compile(r"WideILi(\d+)E")


def accumulators(sym, wide):
    if "k_rs_kara" in sym:  # three role waves in the 16-row contract
        return range(40, 168)
    if not wide:
        return range(64, 128)
    return range(40, 40 + 8 * int(WIDE_R.search(sym).group(1)))


def main():
    tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    with tempfile.TemporaryDirectory() as tmp:
        asm = kid.compile_asm(tree, "rs_jit.hip", os.path.join(tmp, "rs_jit.s"))
    cur, acc, in_asm, bad, seen = None, None, False, 0, 0
    names = []
    for ln in asm.splitlines():
        m = KERNEL.match(ln)
        if m:
            cur, acc, hits = m.group(1), accumulators(m.group(1), m.group(2) == "w"), []
            continue
        if cur is None:
            continue
        if ln.lstrip().startswith(".size") and cur in ln:
            print(f"{cur}: {'clean' if not hits else f'{len(hits)} instruction(s), first: ' + hits[0]}")
            seen += 1
            names.append(cur)
            bad += bool(hits)
            cur = None
        elif ";;#ASMSTART" in ln:
            in_asm = True
        elif ";;#ASMEND" in ln:
            in_asm = False
        elif not in_asm:
            code = ln.split(";")[0]
            regs = [int(r) for r in re.findall(r"\bv(\d+)\b", code)]
            regs += [r for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", code) for r in range(int(a), int(b) + 1)]
            if any(r in acc for r in regs):
                hits.append(code.strip())
    print(f"{seen} kernels, {bad} with compiler code in the accumulators", file=sys.stderr)
    missing = [f for f in FAMILIES if not any(f in n for n in names)]
    if missing:
        print("no kernel seen of: " + ", ".join(missing), file=sys.stderr)
    return 1 if bad or not seen or missing else 0


if __name__ == "__main__":
    sys.exit(main())
