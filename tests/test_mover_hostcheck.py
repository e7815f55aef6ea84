"""The host side of s2amd_world_move_shapes without a GPU: tests/hostcheck/mover_main.cpp, a stand-alone program compiled with ASan +
UBSan on the stand-in HIP runtime of tests/hostcheck (nothing preloaded), run with the stand-in's call trace on.  Its output -- every
return code with its text, what became of every caller buffer, the size of the query block, and the launches, copies, memsets and waits
of every call -- is compared byte for byte with tests/hostcheck/mover_transcript.txt."""
import difflib
import os
import subprocess

import pytest

from tests.test_hostcheck import HERE as HOSTCHECK, _asan_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or _asan_runtime() is None, reason="needs hipcc and clang's ASan runtime")
def test_mover_host_code_under_asan_and_ubsan_reproduces_the_transcript(tmp_path):
    """Every argument refusal and the call without a world -> a world without shape slots (count == 0 touches nothing; the candidates
    pass is skipped, the advance pass runs) -> a world of two shape tiles: every rule of the validation in the first and in the last
    record, with and without a plane array; 1, 128, 129, 256 and 600 movers; one, eight and mixed iteration limits; the batch limit ->
    a smaller world in the block the larger one left -> destroy; every caller buffer a heap block of exactly the size passed."""
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    build = os.path.join(HOSTCHECK, "_build")
    exe = str(tmp_path / "mover_main")
    csrc = os.path.join(ROOT, "solver2d_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-unused-function", "-Wno-unused-value",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-shared-libsan",
                           "-x", "hip", os.path.join(HOSTCHECK, "mover_main.cpp"), "-o", exe, "-L", build, "-ls2amd_hostcheck",
                           "-Wl,-rpath," + build, "-Wl,-rpath," + os.path.dirname(_asan_runtime())])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    env["S2_HOSTCHECK_TRACE_CALLS"] = "1"
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "MOVER MAIN OK" in out, (out[-2000:], err[-4000:])
    assert "AddressSanitizer" not in out + err and "runtime error" not in out + err, err[-4000:]
    # what the transcript must show whatever else it holds: the refusals enqueue nothing, and a call of r rounds is one upload, two
    # memsets, the init kernel, r candidates and r advance launches, one copy back and one wait
    assert out.count("RC -1 ") >= 2 * 18 + 8 and out.count("RC -4 ") >= 2
    with open(os.path.join(HOSTCHECK, "mover_transcript.txt"), "rb") as f:
        want = f.read()
    if p.stdout != want:
        diff = difflib.unified_diff(want.decode().splitlines(), out.splitlines(), "mover_transcript.txt", "this tree", lineterm="", n=4)
        pytest.fail("the movers' host side no longer does what the transcript records:\n" + "\n".join(list(diff)[:120]))
