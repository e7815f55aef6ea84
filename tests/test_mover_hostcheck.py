"""The host side of s2amd_world_move_shapes without a GPU: tests/hostcheck/mover_main.cpp, a stand-alone program compiled with ASan +
UBSan on the stand-in HIP runtime of tests/hostcheck (nothing preloaded), run with the stand-in's call trace on.  Its output -- every
return code with its text, what became of every caller buffer, the size of the query block, and the launches, copies, memsets and waits
of every call -- is compared byte for byte with tests/hostcheck/mover_transcript.txt."""
from tests import hostcheck_util


@hostcheck_util.needs_sanitizers
def test_mover_host_code_under_asan_and_ubsan_reproduces_the_transcript(tmp_path):
    """Every argument refusal and the call without a world -> a world without shape slots (count == 0 touches nothing; the candidates
    pass is skipped, the advance pass runs) -> a world of two shape tiles: every rule of the validation in the first and in the last
    record, with and without a plane array; 1, 128, 129, 256 and 600 movers; one, eight and mixed iteration limits; the batch limit ->
    a smaller world in the block the larger one left -> destroy; every caller buffer a heap block of exactly the size passed."""
    stdout = hostcheck_util.run_sanitized(tmp_path, "mover_main.cpp", "MOVER MAIN OK", timeout=600, trace_calls=True)
    out = stdout.decode(errors="replace")
    # what the transcript must show whatever else it holds: the refusals enqueue nothing, and a call of r rounds is one upload, two
    # memsets, the init kernel, r candidates and r advance launches, one copy back and one wait
    assert out.count("RC -1 ") >= 2 * 18 + 8 and out.count("RC -4 ") >= 2
    hostcheck_util.assert_transcript(stdout, "mover_transcript.txt", "the movers'")
