"""The 512-thread resident-island kernel for s2Solve_SoftStep and s2Solve_PGS_Soft (wide_kernel.hip: wideIslandKernel<KIND, ...>), as far
as it can be checked without a GPU:

  * the host's choice of kernel for a world of resident islands only, on the stand-in HIP runtime of tests/hostcheck (kernels never
    run; launch counts, group tables and s2amd_get_resident_kernel are host state): all three soft solvers take the world in ONE launch
    per step from the second step on (kernel 4), and option "wide" = 0 puts all three back on islandStepKernel between the body
    prologue and epilogue (kernel 2, three launches) -- and, from the stand-in runtime's launch trace, WHICH instantiation each of
    those launches picked;
  * the compiler's register report: every instantiation the launch can pick exists, has no scratch and keeps two waves per SIMD,
    and the eight TGS_Soft instantiations are there beside them (KIND 0 of the same template).

tests/test_gpu_wide_island_kinds.py checks what the kernels compute."""
import glob
import json
import os
import subprocess
import sys

import pytest

from tests import hostcheck_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")

# launch.h: SOFT_TGS 0, SOFT_PGS 1, SOFT_FIXED 3 -- as the demangled names print them.  (kind, rounds) of every form that exists:
# s2Solve_SoftStep has the six-round form only (wide_kernel.hip: wideIslandVariants)
NEW_FORMS = [(3, 6), (1, 6), (1, 8)]
KIND = {"TGS_Soft": 0, "PGS_Soft": 1, "SoftStep": 3}
WARM = {"TGS_Soft": 0, "PGS_Soft": 0, "SoftStep": 1}  # launch.h: WARM_CURRENT 0, WARM_FIXED 1


def _asan_runtime():
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return hits[-1] if hits else None


@pytest.fixture(scope="module")
def cases():
    if not os.path.exists("/opt/rocm/bin/hipcc") or _asan_runtime() is None:
        pytest.skip("needs hipcc and clang's ASan runtime")
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    env = dict(os.environ)
    env["LD_PRELOAD"] = _asan_runtime()
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    env["S2AMD_LIB"] = os.path.join(HOSTCHECK, "_build", "libs2amd_hostcheck.so")
    env["S2_HOSTCHECK_TRACE_LAUNCHES"] = "1"  # hip_stub.cpp: one "LAUNCH <symbol> grid <n> block <n> lds <bytes>" line per launch
    p = subprocess.run([sys.executable, os.path.join(HOSTCHECK, "drive_island_kinds.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=900)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "ISLAND KINDS DRIVER OK" in out and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    found, launches = [], []
    for line in out.splitlines():
        if line.startswith("LAUNCH "):
            launches.append(line.split()[1])
        elif line.startswith("CASE "):
            found.append(json.loads(line[5:]))
            found[-1]["launches"], launches = launches, []  # (the driver prints a case's line behind its steps)
    assert len(found) == 2 * 3 * 2, out[-4000:]
    symbols = sorted({sym for case in found for sym in case["launches"]})
    names = subprocess.run(["c++filt"] + symbols, capture_output=True, text=True, check=True).stdout.splitlines()
    demangled = {sym: name.replace("void ", "").split("(")[0] for sym, name in zip(symbols, names)}
    for case in found:
        case["launches"] = [demangled[sym] for sym in case["launches"]]
    return found


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "SoftStep", "PGS_Soft"])
@pytest.mark.parametrize("world", ["pyramid10x8", "pyramid40x4"])
def test_an_islands_only_world_is_one_launch_per_step(cases, world, solver_name):
    (case,) = [c for c in cases if c["world"] == world and c["solver"] == solver_name and c["wide"] == 1]
    print(case)
    for step in case["steps"][1:]:  # (the first step builds the structure and runs with the body prologue and epilogue)
        assert step["kernelLaunches"] == 1 and step["groupCount"] == 4 and step["stripCount"] == 0, case
        assert step["kernel"] == 4 and step["rounds"] in (6, 8), case
    # the launches of the three steps by name: body prologue, island kernel, body epilogue in the first, then the self-contained form
    # alone (the pyramids' manifolds all have two points, their groups six colour rounds)
    islands = [n for n in case["launches"] if "sland" in n]
    between = "wideIslandKernel<%d, 6, false, 2>" % KIND[solver_name]
    alone = "wideIslandKernel<%d, 6, true, 2>" % KIND[solver_name]
    assert islands == [between, alone, alone], case["launches"]


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "SoftStep", "PGS_Soft"])
@pytest.mark.parametrize("world", ["pyramid10x8", "pyramid40x4"])
def test_option_wide_off_keeps_the_256_thread_island_kernel(cases, world, solver_name):
    (case,) = [c for c in cases if c["world"] == world and c["solver"] == solver_name and c["wide"] == 0]
    print(case)
    for step in case["steps"]:
        assert step["kernelLaunches"] == 3 and step["groupCount"] == 4 and step["stripCount"] == 0, case
        assert step["kernel"] == 2, case
    islands = [n for n in case["launches"] if "sland" in n]
    assert islands == ["islandStepKernel<%d, %d, 6, 512>" % (KIND[solver_name], WARM[solver_name])] * 3, case["launches"]


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    return hostcheck_util.kernel_rows("resources", None)


def test_every_form_the_island_launch_can_pick_is_register_resident(rows):
    by_name = {r["name"]: r for r in rows}
    for kind, rounds in NEW_FORMS:
        for self_contained in ("false", "true"):
            for points in (0, 2):
                name = "wideIslandKernel<%d, %d, %s, %d>" % (kind, rounds, self_contained, points)
                assert name in by_name, name
                r = by_name[name]
                print("%s: %d VGPRs, %d B scratch, %d waves/SIMD" % (name, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
                assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Occupancy"] >= 2, r
                assert not r.get("scratch_instructions"), r  # (counted only for a kernel that declares a frame)
    # nothing but those: an instantiation the launch cannot pick is compile time for nothing
    # (... and s2Solve_TGS_Soft's eight, KIND 0, which tests/test_kernel_resources.py looks up)
    for rounds in (6, 8):
        for self_contained in ("false", "true"):
            for points in (0, 2):
                assert "wideIslandKernel<0, %d, %s, %d>" % (rounds, self_contained, points) in by_name
    assert len([n for n in by_name if n.startswith("wideIslandKernel<")]) == 4 * (len(NEW_FORMS) + 2)
