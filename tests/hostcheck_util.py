"""The four recipes of the tests that need no GPU (tests/test_*_host.py), each in one place: the header's struct layout against the
wire dtypes, the header's declarations and #defines against the bindings, hipcc's resource report of a file's kernels, and a stand-alone
program of tests/hostcheck compiled and run under ASan + UBSan on the stand-in HIP runtime.  A test passes what is its own -- the
records, the calls, the kernel names, the occupancy floor with its reason -- and keeps the checks only it makes."""
import difflib
import glob
import os
import re
import subprocess
import sys

import pytest

from solver2d_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
CSRC = os.path.join(ROOT, "solver2d_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "solver2d_amd.h")
HIPCC = "/opt/rocm/bin/hipcc"


def asan_runtime():
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return hits[-1] if hits else None


needs_sanitizers = pytest.mark.skipif(not os.path.exists(HIPCC) or asan_runtime() is None, reason="needs hipcc and clang's ASan runtime")


def assert_struct_layout(tmp_path, records):
    """{struct of the header: wire dtype}: sizeof and the offsetof of every field of the dtype, as gcc sees the header"""
    lines = ['#include "solver2d_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    want = []
    for struct, dtype in records.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % struct)
        want.append(("sizeof(%s)" % struct, dtype.itemsize))
        for name in dtype.names:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (struct, name))
            want.append(("offsetof(%s, %s)" % (struct, name), dtype.fields[name][1]))
    lines.append("return 0;}")
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert len(got) == len(want)
    wrong = [(what, g, w) for g, (what, w) in zip(got, want) if g != w]
    assert not wrong, "(what, the header, the dtype): %s" % wrong


def assert_header_and_bindings(calls, defines=None, methods=False, argtypes=False):
    """Every call declared in the header as `int <call>(s2amdSolver*` and listed in hip.EXPORTS; every `#define <name> <value>` of
    `defines` there with that value.  methods: hip.Solver has a callable of each call's name less "s2amd_".  argtypes: where both
    libraries are built, each binds every call with its argument types.  Returns the header's text for the caller's own checks."""
    header = open(HEADER).read()
    for call in calls:
        assert re.search(r"\bint %s\(s2amdSolver\*" % call, header), call
        assert call in hip.EXPORTS, call
    for name, value in (defines or {}).items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), (name, value)
    if methods:
        for call in calls:
            assert callable(getattr(hip.Solver, call[len("s2amd_"):])), call
    if argtypes and os.path.exists(hip.LIB_PATH) and os.path.exists(hip.FAST_LIB_PATH):
        for fast in (False, True):
            lib = hip.load(fast=fast)
            for call in calls:
                assert getattr(lib, call).argtypes is not None, call
    return header


def kernel_rows(target, report):
    """hipcc's resource report through tools/kernel_resources.py: `make <target>` in csrc, then the report's rows.  The three ways
    the Makefile offers a report: target "resources-<file>" with report "resources_<file>.txt"; target None, which makes the
    report file itself; target "resources" with report None, the whole library's report."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tools import kernel_resources
    path = os.path.join(CSRC, "build", report) if report else None
    jobs = ["-j4"] if target == "resources" else []
    subprocess.check_call(["make", "-s"] + jobs + ["-C", CSRC, target or path])
    return kernel_resources.parse(path) if path else kernel_resources.parse()


def assert_kernel_resources(target, report, kernels, floor, every_row=False, total=None):
    """kernel_rows(target, report), and every `kernels` {fragment of the mangled name: copies} is there that often, has no private
    frame, spills no register and keeps `floor` waves a SIMD or more.  every_row: no row of the report, whatever its name, has a
    frame or a spill.  total: how many kernels the report holds.  Returns the rows."""
    rows = kernel_rows(target, report)
    names = [r["mangled"] for r in rows if "Kernel" in r["mangled"]]

    def clean(r):
        return r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0

    for kernel, copies in kernels.items():
        found = [r for r in rows if kernel in r["mangled"]]
        assert len(found) == copies, (kernel, len(found), "the report's kernels%s: %s" % (" (the last 40)" if len(names) > 40 else "", names[-40:]))
        for r in found:
            assert clean(r), r
            assert r["Occupancy"] >= floor, r
    if every_row:
        for r in rows:
            assert clean(r), r
    if total is not None:
        assert len(names) == total, names
    return rows


def run_sanitized(tmp_path, source, marker, timeout=600, trace_calls=False):
    """tests/hostcheck/<source> as a stand-alone program under ASan + UBSan on the stand-in HIP runtime: built, run, and clean --
    exit code 0, `marker` in its output, no sanitizer report, nothing leaked.  trace_calls: the stand-in's call trace on, and stderr kept apart so
    that stdout is the program's transcript.  Returns stdout's bytes."""
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    build = os.path.join(HOSTCHECK, "_build")
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-Wno-unused-function", "-Wno-unused-value",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-shared-libsan",
                           "-x", "hip", os.path.join(HOSTCHECK, source), "-o", exe, "-L", build, "-ls2amd_hostcheck",
                           "-Wl,-rpath," + build, "-Wl,-rpath," + os.path.dirname(asan_runtime())])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    if trace_calls:
        env["S2_HOSTCHECK_TRACE_CALLS"] = "1"
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE if trace_calls else subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors="replace")
    err = p.stderr.decode(errors="replace") if trace_calls else ""
    tail = (out[-2000:], err[-4000:]) if trace_calls else out[-4000:]
    assert p.returncode == 0 and marker in out, tail
    assert "AddressSanitizer" not in out + err and "LeakSanitizer" not in out + err and "runtime error" not in out + err, tail
    return p.stdout


def assert_transcript(stdout, name, whose):
    """A traced program's stdout against tests/hostcheck/<name>, byte for byte; the failure shows the diff"""
    with open(os.path.join(HOSTCHECK, name), "rb") as f:
        want = f.read()
    if stdout != want:
        diff = difflib.unified_diff(want.decode().splitlines(), stdout.decode(errors="replace").splitlines(), name, "this tree", lineterm="", n=4)
        pytest.fail("%s host side no longer does what the transcript records:\n" % whose + "\n".join(list(diff)[:120]))
