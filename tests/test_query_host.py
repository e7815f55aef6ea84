"""The host side of the eight queries on the resident world without a GPU: tests/hostcheck/query_main.cpp, a stand-alone program compiled
with ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (nothing preloaded), run with the stand-in's call trace on.  Its output --
every return code with its text, what became of every caller buffer, the size of the query block, and the launches, copies, memsets and
waits of every call -- is compared byte for byte with tests/hostcheck/query_transcript.txt, which was recorded before the four query
files were moved onto csrc/query_host.h: a change to that header, or a new query built on it, that alters what an existing call
enqueues, answers or touches shows here as a diff."""
from tests import hostcheck_util


@hostcheck_util.needs_sanitizers
def test_query_host_code_under_asan_and_ubsan_reproduces_the_transcript(tmp_path):
    """All eight calls: every argument refusal and the calls without a world -> a world without shape slots (count == 0 touches nothing;
    the list calls zero their offsets without a launch, the single-answer calls skip the candidates pass) -> a world of two shape tiles:
    one invalid record first and last, 1, 256, 257 and 600 queries with ample room, 257 with a capacity of 0 and 1, shapes in range with
    and without distances, totals beyond the capacity, the batch limits -> a smaller world in the block the larger ones left -> destroy;
    every caller buffer a heap block of exactly the size passed."""
    stdout = hostcheck_util.run_sanitized(tmp_path, "query_main.cpp", "QUERY MAIN OK", timeout=600, trace_calls=True)
    hostcheck_util.assert_transcript(stdout, "query_transcript.txt", "the queries'")
