"""What becomes of created, destroyed and flipped contacts on the host, without a GPU: tests/hostcheck/placement_main.cpp, a stand-alone
program compiled with ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (nothing preloaded), run with the stand-in's call trace
on.  Its output -- per call the return code, the structure's counters, hashes of the sweep order and of the host shadows (a line only
where it changed), the patch list with every address resolved to its block, and the launches, copies, memsets and waits of every
upload and s2amd_world_set_contacts -- is compared byte for byte with tests/hostcheck/placement_transcript.txt, which was recorded before the four sites that decide about such a
contact were given one front (solver_incremental.cpp)."""
import re

from tests import hostcheck_util


@hostcheck_util.needs_sanitizers
def test_placement_host_code_under_asan_and_ubsan_reproduces_the_transcript(tmp_path):
    """A scripted churn through the host-array route and through the world route in a scene per placement route: colour batches, no free
    colour -> one rebuild -> spare colours, the sequential tail of a hub (defer, then flip), s2Solve_Jacobi, strips under TGS_Soft (strip
    and seam rounds, extended seams, opened spare rounds, adopted bodies), strips under the op interpreter (which refuses all but a free
    position), strips built by a worker thread (replay and adoption)."""
    stdout = hostcheck_util.run_sanitized(tmp_path, "placement_main.cpp", "PLACEMENT MAIN OK", timeout=600, trace_calls=True)
    out = stdout.decode(errors="replace")
    # whatever else the transcript holds, it reaches every route it is there for: the counters say so
    most = {}
    for line in out.splitlines():
        if line.startswith("inc valid") or line.startswith("strips valid"):
            for name, value in re.findall(r"(inserted|removed|tail|placed|rounds|adopted|seam bodies) (\d+)", line):
                most[name] = max(most.get(name, 0), int(value))
    assert all(most.get(name, 0) > 0 for name in ("inserted", "removed", "tail", "placed", "rounds", "adopted", "seam bodies")), most
    assert "(no free colour)" in out and "(body owned by a group or strip)" in out and "requested 3 adopted 1" in out
    assert "COPY HostToDevice" in out and "LAUNCH" in out  # (the stand-in's call trace is on)
    hostcheck_util.assert_transcript(stdout, "placement_transcript.txt", "the placement's")
