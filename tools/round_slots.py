#!/usr/bin/env python3
"""Issue slots per barrier segment of one kernel, from the device assembly `make -C solver2d_amd/csrc resources` leaves behind:

    python tools/round_slots.py "wideStepKernel<2, 3, 2, 0, 0, 0, 0>" [solver2d_amd/csrc/build/asm_wide_kernel.s]

A segment is the kernel's text between two `s_barrier`s (the first starts at the kernel's label, the last ends at s_endpgm), in the
order of the listing.  Per segment: the instructions whose mnemonic starts with v_ (VALU; of which v_pk_*: packed), with s_ (SALU:
scalar arithmetic, branches, s_waitcnt and s_nop alike -- everything the wave's one in-order stream issues besides the barrier itself; of
which s_nop: the hazard padding the compiler puts where no independent instruction is left to fill a dependence),
with ds_ (LDS) and with global_ / flat_ / buffer_ / scratch_ (memory).  Text order is not execution order: a segment that holds a branch
around half of its text (the chain in one half of the workgroup, the prep in the other) shows the sum of both sides, and a loop body
counts once.  The tool counts instruction classes and checks nothing (profiles/issue_slots_asm.txt is its output for two builds)."""
import re
import subprocess
import sys

DEFAULT_ASM = "solver2d_amd/csrc/build/asm_wide_kernel.s"


def kernel_text(path, wanted):
    """The instruction lines of the kernel whose demangled name (without return type and arguments) is `wanted`."""
    labels = []
    with open(path, errors="replace") as f:
        lines = f.readlines()
    for n, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            labels.append((m.group(1), n))
    names = subprocess.run(["c++filt"] + [l for l, _ in labels], capture_output=True, text=True, check=True).stdout.splitlines()
    for (label, start), name in zip(labels, names):
        if re.sub(r"\(.*", "", name.replace("void ", "")) == wanted:
            end = next(n for n in range(start, len(lines)) if lines[n].startswith(".Lfunc_end"))
            return lines[start + 1:end]
    sys.exit("%s: no kernel %r" % (path, wanted))


def segments(text):
    rows = [dict(valu=0, packed=0, salu=0, nop=0, ds=0, mem=0)]
    for line in text:
        word = line.split(";")[0].split()
        if not word or word[0].endswith(":") or word[0].startswith("."):
            continue
        op = word[0]
        if op == "s_barrier":
            rows.append(dict(valu=0, packed=0, salu=0, nop=0, ds=0, mem=0))
        elif op.startswith("v_"):
            rows[-1]["valu"] += 1
            rows[-1]["packed"] += op.startswith("v_pk_")
        elif op.startswith("s_"):
            rows[-1]["salu"] += 1
            rows[-1]["nop"] += op == "s_nop"
        elif op.startswith("ds_"):
            rows[-1]["ds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            rows[-1]["mem"] += 1
    return rows


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    rows = segments(kernel_text(argv[2] if len(argv) == 3 else DEFAULT_ASM, argv[1]))
    print("%s: %d barrier segments" % (argv[1], len(rows)))
    cols = ("valu", "packed", "salu", "nop", "ds", "mem")
    print("%4s %6s %7s %6s %6s %4s %4s" % ("seg", "VALU", "packed", "SALU", "s_nop", "DS", "mem"))
    for i, r in enumerate(rows):
        print("%4d %6d %7d %6d %6d %4d %4d" % ((i,) + tuple(r[c] for c in cols)))
    print("%4s %6d %7d %6d %6d %4d %4d" % (("sum",) + tuple(sum(r[c] for r in rows) for c in cols)))


if __name__ == "__main__":
    main(sys.argv)
