"""The joint report without a GPU: the three new structs of include/solver2d_amd.h have the sizes of their wire dtypes, the reference
statement the GPU tests compare against (tests/joint_report_ref.py) gives, on a world small enough to work out by hand, the values
written out here, and the host side of the report runs clean under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck."""
import os
import subprocess
import sys

import numpy as np

from solver2d_amd import wire
from tests import hostcheck_util, joint_report_ref as ref
from tests.hostcheck_util import HOSTCHECK, asan_runtime as _asan_runtime

f32 = np.float32


def test_joint_report_struct_sizes_match_header(tmp_path):
    hostcheck_util.assert_struct_layout(tmp_path, {"s2amdJointState": wire.joint_state_dtype, "s2amdBodyJointSum": wire.body_joint_sum_dtype,
                                                   "s2amdJointSummary": wire.joint_summary_dtype})
    assert [wire.joint_state_dtype.itemsize, wire.body_joint_sum_dtype.itemsize, wire.joint_summary_dtype.itemsize] == [64, 16, 32]


def test_joint_report_exports_and_flags():
    hostcheck_util.assert_header_and_bindings(("s2amd_world_set_joint_report", "s2amd_world_joint_states", "s2amd_world_joint_limit_events",
                                               "s2amd_world_body_joint_sums", "s2amd_world_joint_summary"))
    assert (wire.JOINT_REPORT_STATES, wire.JOINT_REPORT_LIMITS, wire.JOINT_REPORT_BODY_SUMS, wire.JOINT_REPORT_ALL) == (1, 2, 4, 7)
    assert wire.REPORT_ALL == 7 and wire.API_VERSION == 5  # the contact report's flag space and the API version are untouched


def three_joint_slot_world():
    """Bodies 0, 1, 2; joint slot 0 revolute (1 -> 2), slot 1 free, slot 2 mouse (0 -> 1): body 1, turned by 90 degrees, is bodyA of one
    joint and bodyB of another.  Every number is a small dyadic fraction: the float32 results are exact."""
    bodies = np.zeros(3, dtype=wire.body_dtype)
    bodies["rot"] = [(0.0, 1.0), (1.0, 0.0), (0.0, 1.0)]  # {s, c}
    bodies["angularVelocity"] = [0.125, 0.5, -0.25]
    origins = np.array([(1.0, 2.0), (0.5, -1.0), (4.0, 0.0)], dtype=np.float32)
    joints = np.zeros(3, dtype=wire.joint_dtype)
    joints["type"] = [wire.JOINT_REVOLUTE, wire.JOINT_FREE, wire.JOINT_MOUSE]
    joints["bodyA"], joints["bodyB"] = [1, -1, 0], [2, -1, 1]
    r = joints[0]
    r["enableLimit"], r["enableMotor"] = 1, 1
    r["localOriginAnchorA"], r["localOriginAnchorB"] = (2.0, 1.0), (-0.5, 0.25)
    r["impulse"], r["motorImpulse"], r["lowerImpulse"], r["upperImpulse"] = (0.5, -2.0), 0.25, 1.5, 0.5
    r["referenceAngle"], r["lowerAngle"], r["upperAngle"] = 0.5, -1.0, 1.0
    # what a free slot holds is not reported
    joints[1]["impulse"], joints[1]["lowerImpulse"], joints[1]["enableLimit"] = (9.0, 9.0), 9.0, 1
    m = joints[2]
    m["localOriginAnchorA"], m["localOriginAnchorB"] = (7.0, 7.0), (2.0, -1.0)
    m["impulse"], m["motorImpulse"] = (-1.0, 0.75), 0.125
    m["lowerImpulse"], m["upperImpulse"], m["enableLimit"], m["referenceAngle"] = 99.0, 77.0, 1, 3.0  # junk: a mouse joint has none of them
    m["targetA"], m["hertz"], m["dampingRatio"] = (5.0, 1.0), 5.0, 0.7
    return {"bodies": bodies, "contacts": np.zeros(0, dtype=wire.contact_dtype), "joints": joints, "shapes": np.zeros(0, dtype=wire.shape_dtype),
            "pairs": np.zeros(0, dtype=wire.pair_state_dtype), "origins": origins}


def test_reference_statement_on_a_hand_written_world():
    w = three_joint_slot_world()
    s = ref.states(w)
    assert s.dtype == wire.joint_state_dtype and len(s) == 2
    assert s["slot"].tolist() == [0, 2] and s["type"].tolist() == [0, 1]
    assert s["bodyA"].tolist() == [1, 0] and s["bodyB"].tolist() == [2, 1]
    # revolute: body 1 (s = 1, c = 0, origin (0.5, -1)): x = (0 * 2 - 1 * 1) + 0.5, y = (1 * 2 + 0 * 1) - 1; body 2: identity at (4, 0)
    # mouse: anchorA is targetA; anchorB on body 1: x = (0 * 2 - 1 * -1) + 0.5, y = (1 * 2 + 0 * -1) - 1
    assert s["anchorA"].tolist() == [[-0.5, 1.0], [5.0, 1.0]]
    assert s["anchorB"].tolist() == [[3.5, 0.25], [1.5, 1.0]]
    assert s["impulse"].tolist() == [[0.5, -2.0], [-1.0, 0.75]]
    assert s["motorImpulse"].tolist() == [0.25, 0.125]
    assert s["axialImpulse"].tolist() == [1.25, 0.125]  # (0.25 + 1.5) - 0.5; the mouse joint's motorImpulse
    # s2RelativeAngle(rotB, rotA): s = 0 * 0 - 1 * 1 = -1, c = 1 * 0 + 0 * 1 = 0: atan2f(-1, 0) = -pi/2 in float32, less referenceAngle
    assert s["angle"][0] == f32(f32(-1.5707963705062866) - f32(0.5)) and s["angle"][0] == f32(-2.0707963705062866)
    assert s["angle"][1].tobytes() == f32(0.0).tobytes()
    assert s["angularSpeed"].tolist() == [-0.75, 0.5]  # wB - wA; the mouse joint: wB
    assert s["lowerImpulse"].tolist() == [1.5, 0.0] and s["upperImpulse"].tolist() == [0.5, 0.0]
    assert s["lowerImpulse"][1].tobytes() == s["upperImpulse"][1].tobytes() == f32(0.0).tobytes()

    assert ref.limit_mask(w["joints"]).tolist() == [True, True, False, False, False, False]
    began, ended = ref.events(np.zeros(6, dtype=bool), w)
    assert began.tolist() == [0, 1] and ended.tolist() == [] and began.dtype == np.int32
    began, ended = ref.events([False, True, False, False, True, False], w)
    assert began.tolist() == [0] and ended.tolist() == [4]
    began, ended = ref.events(ref.limit_mask(w["joints"]), w)
    assert began.tolist() == [] and ended.tolist() == []

    # body 0 is the mouse joint's bodyA: nothing; body 1: -(0.5, -2), -1.25 as bodyA of slot 0, then +(-1, 0.75), +0.125 as bodyB of slot 2
    b = ref.body_sums(w)
    assert b.dtype == wire.body_joint_sum_dtype
    assert b["impulse"].tolist() == [[0.0, 0.0], [-1.5, 2.75], [0.5, -2.0]]
    assert b["axialImpulse"].tolist() == [0.0, -1.125, 1.25]
    assert b["joints"].tolist() == [0, 2, 1]
    assert b[0].tobytes() == bytes(16)  # +0, not -0

    # d = (3.5 + 0.5, 0.25 - 1): g = 16 + 0.5625
    m = ref.summary(w)
    assert m.dtype == wire.joint_summary_dtype
    assert [int(m[k]) for k in ("liveJoints", "revoluteJoints", "atLower", "atUpper", "maxGapSlot")] == [2, 1, 1, 1, 0]
    assert m["maxGapSquared"] == f32(16.5625) and m["pad"].tolist() == [0, 0]


def test_limits_need_the_flag_and_the_gap_its_rules():
    w = three_joint_slot_world()
    w["joints"]["enableLimit"][0] = 0
    assert not ref.limit_mask(w["joints"]).any()
    assert [int(ref.summary(w)[k]) for k in ("atLower", "atUpper")] == [0, 0]
    # a tie goes to the lowest slot: slot 1 becomes a copy of slot 0
    w["joints"][1] = w["joints"][0]
    m = ref.summary(w)
    assert (int(m["revoluteJoints"]), int(m["maxGapSlot"]), float(m["maxGapSquared"])) == (2, 0, 16.5625)
    # a NaN never wins
    w["origins"][1] = (np.nan, 0.0)
    m = ref.summary(w)
    assert (int(m["maxGapSlot"]), float(m["maxGapSquared"])) == (-1, -1.0)
    # no revolute joint
    w["joints"]["type"][:2] = wire.JOINT_FREE
    m = ref.summary(w)
    assert (int(m["liveJoints"]), int(m["revoluteJoints"]), int(m["maxGapSlot"]), float(m["maxGapSquared"])) == (1, 0, -1, -1.0)


@hostcheck_util.needs_sanitizers
def test_joint_report_host_code_under_asan_and_ubsan():
    """upload -> set_joint_report(all) -> step -> the four getters -> capacity errors -> upload again, on the sanitizer build of
    tests/test_hostcheck.py (kernels never run there: what is checked is that the host code touches only memory it owns)."""
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    env = dict(os.environ)
    env["LD_PRELOAD"] = _asan_runtime()
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    env["S2AMD_LIB"] = os.path.join(HOSTCHECK, "_build", "libs2amd_hostcheck.so")
    p = subprocess.run([sys.executable, os.path.join(HOSTCHECK, "drive_joint_report.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "JOINT REPORT DRIVER OK" in out and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
