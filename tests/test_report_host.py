"""The host sides of the contact report and the joint report without a GPU: tests/hostcheck/contact_joint_report_main.cpp runs clean
under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded), as the shape report's,
the body report's and the step metrics' programs do (tests/test_shape_report_host.py)."""
import os
import subprocess

import pytest

from tests.test_hostcheck import HERE as HOSTCHECK, _asan_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or _asan_runtime() is None, reason="needs hipcc and clang's ASan runtime")
def test_contact_and_joint_report_host_code_under_asan_and_ubsan(tmp_path):
    """Upload -> every flag combination 0..7 of both reports -> every getter with too-small, exact and ample heap buffers of exactly the
    size passed -> uploads with other capacities, worlds without contact slots and without joint slots among them -> destroy, on the
    sanitizer build of tests/test_hostcheck.py (kernels never run there: the program writes the heads through the report states' head
    offsets, and what is checked is that the host code touches only memory it owns)."""
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    build = os.path.join(HOSTCHECK, "_build")
    exe = str(tmp_path / "contact_joint_report_main")
    csrc = os.path.join(ROOT, "solver2d_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-unused-function", "-Wno-unused-value",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-shared-libsan",
                           "-x", "hip", os.path.join(HOSTCHECK, "contact_joint_report_main.cpp"), "-o", exe, "-L", build, "-ls2amd_hostcheck",
                           "-Wl,-rpath," + build, "-Wl,-rpath," + os.path.dirname(_asan_runtime())])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "CONTACT JOINT REPORT MAIN OK" in out and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
