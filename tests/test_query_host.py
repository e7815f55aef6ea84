"""The host side of the eight queries on the resident world without a GPU: tests/hostcheck/query_main.cpp, a stand-alone program compiled
with ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (nothing preloaded), run with the stand-in's call trace on.  Its output --
every return code with its text, what became of every caller buffer, the size of the query block, and the launches, copies, memsets and
waits of every call -- is compared byte for byte with tests/hostcheck/query_transcript.txt, which was recorded before the four query
files were moved onto csrc/query_host.h: a change to that header, or a new query built on it, that alters what an existing call
enqueues, answers or touches shows here as a diff."""
import difflib
import os
import subprocess

import pytest

from tests.test_hostcheck import HERE as HOSTCHECK, _asan_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or _asan_runtime() is None, reason="needs hipcc and clang's ASan runtime")
def test_query_host_code_under_asan_and_ubsan_reproduces_the_transcript(tmp_path):
    """All eight calls: every argument refusal and the calls without a world -> a world without shape slots (count == 0 touches nothing;
    the list calls zero their offsets without a launch, the single-answer calls skip the candidates pass) -> a world of two shape tiles:
    one invalid record first and last, 1, 256, 257 and 600 queries with ample room, 257 with a capacity of 0 and 1, shapes in range with
    and without distances, totals beyond the capacity, the batch limits -> a smaller world in the block the larger ones left -> destroy;
    every caller buffer a heap block of exactly the size passed."""
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    build = os.path.join(HOSTCHECK, "_build")
    exe = str(tmp_path / "query_main")
    csrc = os.path.join(ROOT, "solver2d_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-unused-function", "-Wno-unused-value",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-shared-libsan",
                           "-x", "hip", os.path.join(HOSTCHECK, "query_main.cpp"), "-o", exe, "-L", build, "-ls2amd_hostcheck",
                           "-Wl,-rpath," + build, "-Wl,-rpath," + os.path.dirname(_asan_runtime())])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    env["S2_HOSTCHECK_TRACE_CALLS"] = "1"
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "QUERY MAIN OK" in out, (out[-2000:], err[-4000:])
    assert "AddressSanitizer" not in out + err and "runtime error" not in out + err, err[-4000:]
    with open(os.path.join(HOSTCHECK, "query_transcript.txt"), "rb") as f:
        want = f.read()
    if p.stdout != want:
        diff = difflib.unified_diff(want.decode().splitlines(), out.splitlines(), "query_transcript.txt", "this tree", lineterm="", n=4)
        pytest.fail("the queries' host side no longer does what the transcript records:\n" + "\n".join(list(diff)[:120]))
