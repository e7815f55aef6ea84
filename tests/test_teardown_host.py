"""What a solver owns and gives back, without a GPU: tests/hostcheck/teardown_main.cpp runs clean under ASan + UBSan with the leak check
on, on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded), as the reports' programs do
(tests/test_report_host.py)."""
from tests import hostcheck_util


@hostcheck_util.needs_sanitizers
def test_teardown_host_code_under_asan_ubsan_and_the_leak_check(tmp_path):
    """For worlds of 0, 40 and 700 bodies: create -> upload -> every list set and every report on -> two steps -> each staged writer
    (s2amd_world_edit, s2amd_world_apply_fields, s2amd_world_set_actions, s2amd_world_reset_agents with a list) twice in a row -> one
    asynchronous export per slot -> a tree set -> a world of another size -> destroy.  On the stand-in runtime a device block, a pinned
    block, an event and a stream are heap blocks: one the destroy forgets is a leak, one it gives back twice an ASan report, and the
    program ends with neither.  The first run of the edit path's host side there as well."""
    hostcheck_util.run_sanitized(tmp_path, "teardown_main.cpp", "TEARDOWN MAIN OK", timeout=600)
