"""The host sides of the contact report and the joint report without a GPU: tests/hostcheck/contact_joint_report_main.cpp runs clean
under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded), as the shape report's,
the body report's and the step metrics' programs do (tests/test_shape_report_host.py)."""
from tests import hostcheck_util


@hostcheck_util.needs_sanitizers
def test_contact_and_joint_report_host_code_under_asan_and_ubsan(tmp_path):
    """Upload -> every flag combination 0..7 of both reports -> every getter with too-small, exact and ample heap buffers of exactly the
    size passed -> uploads with other capacities, worlds without contact slots and without joint slots among them -> destroy, on the
    sanitizer build of tests/test_hostcheck.py (kernels never run there: the program writes the heads through the report states' head
    offsets, and what is checked is that the host code touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "contact_joint_report_main.cpp", "CONTACT JOINT REPORT MAIN OK", timeout=600)
