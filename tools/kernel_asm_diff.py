"""Do two builds hold the same kernels, instruction for instruction?  The proof a refactor of the kernel files owes:

    make -C solver2d_amd/csrc -j8 resources RES_FILES="wide_kernel strip_kernel pair_kernel generic_kernel group_kernel"

on both trees, then  python tools/kernel_asm_diff.py <old>/solver2d_amd/csrc/build <new>/solver2d_amd/csrc/build
(or two asm_<file>.s).  Per asm_<file>.s present on both sides: every kernel's text from its label to .Lfunc_end, keyed by its demangled
name, with what is a name and not an instruction normalised -- the kernel's own mangled name, the per-function numbers of local labels
(.LBB<n>_<m>, .Lfunc_end<n>: they move when the order of instantiation does) and comment lines.  Prints the counts and the names that are
on one side only or whose bodies differ; exit status 1 if there are any.
Names of the old side go through RENAMES first (a refactor may rename a kernel): extend it as kernels are renamed."""
import os
import re
import subprocess
import sys

# old demangled name -> new: wideIslandKernel<R, S, P> became wideIslandKernel<0, R, S, P>, wideIslandKernelOf<K, ...> wideIslandKernel<K, ...>
RENAMES = [(re.compile(r"^wideIslandKernel<(\d+, (?:true|false), \d+)>$"), r"wideIslandKernel<0, \1>"),
           (re.compile(r"^wideIslandKernelOf<"), "wideIslandKernel<")]


def kernels(path, renames=()):
    """{demangled name: normalised body} of the global functions of one assembly file"""
    bodies, cur, lines = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, lines = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            bodies[cur] = lines
            cur = None
            continue
        text = line.split(";")[0].rstrip()  # (comments: the compiler's notes, among them mangled names and block numbers)
        if text:
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", text.replace(cur, "<self>")))
    mangled = sorted(bodies)
    names = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    short = [re.sub(r"\(.*", "", n.replace("void ", "")) for n in names]
    for m, n, s in zip(mangled, names, short):
        # (library kernels whose template arguments hold a parenthesis -- rocPRIM's sort kernels -- keep their whole name)
        n = s if short.count(s) == 1 else n
        for pattern, to in renames:
            n = pattern.sub(to, n)
        assert n not in out, n
        out[n] = bodies[m]
    return out


def files(path):
    if os.path.isdir(path):
        return {f: os.path.join(path, f) for f in sorted(os.listdir(path)) if f.startswith("asm_") and f.endswith(".s")}
    return {"": path}


def main(old, new):
    a, b = files(old), files(new)
    bad = 0
    for f in sorted(set(a) | set(b)):
        if f not in a or f not in b:
            print("%s: on one side only" % f)
            bad += 1
            continue
        ka, kb = kernels(a[f], RENAMES), kernels(b[f])
        gone, added = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
        print("%s: %d kernels old, %d new, %d only old, %d only new, %d bodies differ" % (f or new, len(ka), len(kb), len(gone), len(added), len(differ)))
        for tag, names in (("only old", gone), ("only new", added), ("differs", differ)):
            for n in names:
                print("  %s: %s" % (tag, n))
        bad += len(gone) + len(added) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
