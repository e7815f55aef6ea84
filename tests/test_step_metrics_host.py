"""The step metrics without a GPU: s2amdStepMetrics of include/solver2d_amd.h has the size and field offsets of its wire dtype, the
reference statement the GPU tests compare against (tests/step_metrics_ref.py) gives, on a world small enough to work out by hand, the
values written out here, its one summation shape is pinned on a vector on which left-to-right summation gives other bits, the statement
separates the solvers on the CPU oracle chain as the samples are meant to show, the host side runs clean under ASan + UBSan on the
stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded), and the new kernels use no scratch."""
import os

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import hostcheck_util, step_metrics_ref as ref, world_chain
from tests.world_chain import golden

f32 = np.float32
NAMES = ("s2amd_world_set_metrics", "s2amd_world_metrics", "s2amd_world_metrics_history")
# the golden worlds tests/test_gpu_step_metrics.py steps
GPU_WORLDS = ("far_ragdoll_pile0_PGS_Soft", "high_mass_ratio1_PGS_NGS", "tumbler60_TGS_Soft", "mixed24_Jacobi", "circle_pile20_XPBD", "joint_grid6_TGS_NGS")
FLOAT_SUMS = ("sumPenetration", "sumNormalImpulse", "kineticEnergy", "potentialEnergy", "momentum", "spin", "sumJointGapSquared")


def test_step_metrics_struct_size_and_offsets_match_header(tmp_path):
    dtype = wire.step_metrics_dtype
    hostcheck_util.assert_struct_layout(tmp_path, {"s2amdStepMetrics": dtype})
    assert dtype.itemsize == 128 and len(dtype.names) == 24
    assert [dtype.fields[n][1] for n in ("touchingContacts", "minGap", "sumPenetration", "energyBodies", "potentialEnergy", "momentum", "spin",
                                         "revoluteJoints", "sumJointGapSquared", "pad")] == [16, 32, 48, 56, 64, 68, 76, 80, 92, 96]


def test_step_metrics_exports_and_flags():
    hostcheck_util.assert_header_and_bindings(NAMES, {"S2AMD_METRICS_CONTACTS": 1, "S2AMD_METRICS_BODIES": 2, "S2AMD_METRICS_JOINTS": 4, "S2AMD_API_VERSION": 5})
    assert (wire.METRICS_CONTACTS, wire.METRICS_BODIES, wire.METRICS_JOINTS, wire.METRICS_ALL, wire.METRICS_MAX_HISTORY) == (1, 2, 4, 7, 4096)
    # the four reports' flag spaces and the API version are untouched
    assert wire.REPORT_ALL == 7 and wire.JOINT_REPORT_ALL == 7 and wire.SHAPE_REPORT_ALL == 7 and wire.BODY_REPORT_ALL == 15 and wire.API_VERSION == 5
    if os.path.exists(hip.LIB_PATH):
        lib = hip.load()
        for name in NAMES:
            assert getattr(lib, name) is not None


def hand_world():
    """Body 0 static at the origin; body 1 dynamic with origin (0, 1), unrotated, its centre of mass at local (0, 0.5), mass 2, I 0.5,
    v = (0.5, -1), w = 2.  Contact slots: 0 has a point but a free pair slot, 1 is the two-point contact 0-1 with normal (0, 1), 2 names a
    body outside the array.  Joint slots: 0 a mouse joint, 1 free, 2 the revolute joint 0-1.  Every number is a small dyadic fraction."""
    bodies = np.zeros(2, dtype=wire.body_dtype)
    bodies["type"] = [wire.BODY_STATIC, wire.BODY_DYNAMIC]
    bodies["rot"] = (0.0, 1.0)
    b = bodies[1]
    b["localCenter"], b["position"] = (0.0, 0.5), (0.0, 1.5)
    b["linearVelocity"], b["angularVelocity"] = (0.5, -1.0), 2.0
    b["mass"], b["invMass"], b["I"], b["invI"], b["gravityScale"] = 2.0, 0.5, 0.5, 2.0, 1.0
    origins = np.array([(0.0, 0.0), (0.0, 1.0)], dtype=f32)
    contacts = np.zeros(3, dtype=wire.contact_dtype)
    pairs = np.zeros(3, dtype=wire.pair_state_dtype)
    pairs["shapeA"], pairs["shapeB"] = [-1, 0, 0], [-1, 1, 1]
    contacts["bodyA"], contacts["bodyB"], contacts["pointCount"] = [0, 0, 0], [1, 1, 99], [1, 2, 1]
    contacts["normal"] = (0.0, 1.0)
    contacts["points"]["normalImpulse"] = 64.0  # (of the slots that do not touch: in no sum)
    c = contacts[1]
    c["points"][0]["localAnchorA"], c["points"][0]["localAnchorB"] = (-1.0, 0.5), (-1.0, -0.53125)
    c["points"][0]["separation"], c["points"][0]["normalImpulse"] = -0.0625, 1.5
    c["points"][1]["localAnchorA"], c["points"][1]["localAnchorB"] = (1.0, 0.5), (1.0, -0.25)
    c["points"][1]["separation"], c["points"][1]["normalImpulse"] = 0.125, 0.25
    joints = np.zeros(3, dtype=wire.joint_dtype)
    joints["type"] = [wire.JOINT_MOUSE, wire.JOINT_FREE, wire.JOINT_REVOLUTE]
    joints["bodyA"], joints["bodyB"] = [0, 0, 0], [1, 1, 1]
    joints["localOriginAnchorA"], joints["localOriginAnchorB"] = (0.5, 1.0), (0.25, 0.5)
    joints["localOriginAnchorB"][0] = (8.0, 8.0)  # the mouse joint's: in no sum
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": np.zeros(0, dtype=wire.shape_dtype), "pairs": pairs, "origins": origins}


def test_reference_statement_on_a_hand_worked_world():
    w = hand_world()
    params = wire.StepParams.make("TGS_Soft", 0.25, 4, 2, True, gravity=(0.0, -10.0))
    # point 0: T(A) = (-1, 0.5), T(B) = (-1, 1 - 0.53125) = (-1, 0.46875), d = (0, -0.03125), gap = -0.03125 - 0.0625 = -0.09375;
    #          a = (-1, -0.53125 - 0.5) = (-1, -1.03125) = r, u_B = (0.5 + 2 * 1.03125, -1 - 2) = (2.5625, -3), vn = -3
    # point 1: T(B) = (1, 0.75), d = (0, 0.25), gap = 0.25 + 0.125 = 0.375; a = (1, -0.75), u_B = (0.5 + 1.5, -1 + 2) = (2, 1), vn = 1
    slot, point, gap, vn, impulse = ref.contact_points(w)
    assert slot.tolist() == [1, 1] and point.tolist() == [0, 1]
    assert gap.tolist() == [-0.09375, 0.375] and vn.tolist() == [-3.0, 1.0] and impulse.tolist() == [1.5, 0.25]
    r = ref.record(w, params, wire.METRICS_ALL, 3)
    assert r.dtype == wire.step_metrics_dtype
    assert [int(r[k]) for k in ("step", "flags", "solverType")] == [3, 7, wire.SOLVER_ID["TGS_Soft"]] and float(r["dt"]) == 0.25
    assert [int(r[k]) for k in ("touchingContacts", "touchingPoints", "penetratingPoints", "approachingPoints")] == [1, 2, 1, 1]
    assert (float(r["minGap"]), int(r["minGapSlot"]), float(r["maxApproachSpeed"]), int(r["maxApproachSlot"])) == (-0.09375, 1, 3.0, 1)
    assert float(r["sumPenetration"]) == 0.09375 and float(r["sumNormalImpulse"]) == 1.75
    # kinetic (0.5 * 2) * (0.25 + 1) + (0.5 * 0.5) * 4 = 2.25; potential -((2 * 1) * (0 * 0 + -10 * 1.5)) = 30
    assert int(r["energyBodies"]) == 1 and float(r["kineticEnergy"]) == 2.25 and float(r["potentialEnergy"]) == 30.0
    assert r["momentum"].tolist() == [1.0, -2.0] and float(r["spin"]) == 1.0
    # joint: T(A) = (0.5, 1), T(B) = (0.25, 1.5), d = (-0.25, 0.5), g = 0.0625 + 0.25
    assert (int(r["revoluteJoints"]), int(r["maxJointGapSlot"]), float(r["maxJointGapSquared"]), float(r["sumJointGapSquared"])) == (1, 2, 0.3125, 0.3125)
    assert r["pad"].tolist() == [0] * 8
    # each flag alone: the other sections are zero bytes
    whole = r.tobytes()
    sections = {wire.METRICS_CONTACTS: (16, 56), wire.METRICS_BODIES: (56, 80), wire.METRICS_JOINTS: (80, 96)}
    for flag, (lo, hi) in sections.items():
        one = ref.record(w, params, flag, 3).tobytes()
        assert one[lo:hi] == whole[lo:hi] and one[96:] == bytes(32)
        assert one[16:lo] == bytes(lo - 16) and one[hi:96] == bytes(96 - hi)
    # a quarter turn of body 1 (rot = {1, 0}): T(B, p) = (-p.y, p.x) + o and r = (-a.y, a.x)
    w["bodies"]["rot"][1] = (1.0, 0.0)
    slot, point, gap, vn, impulse = ref.contact_points(w)
    # point 0: T(B) = (0.53125, 1 - 1) = (0.53125, 0), d.y = -0.5, gap = -0.5625; r = (1.03125, -1), u_B = (0.5 + 2, -1 + 2.0625), vn = 1.0625
    # point 1: T(B) = (0.25, 2), d.y = 1.5, gap = 1.625; r = (0.75, 1), u_B = (0.5 - 2, -1 + 1.5), vn = 0.5
    assert gap.tolist() == [-0.5625, 1.625] and vn.tolist() == [1.0625, 0.5]
    r = ref.record(w, params, wire.METRICS_CONTACTS, 0)
    assert (int(r["approachingPoints"]), float(r["maxApproachSpeed"]), int(r["maxApproachSlot"])) == (0, 0.0, -1)
    assert not np.signbit(r["maxApproachSpeed"])
    # nothing touching, nobody to count, no revolute joint: the sentinels
    w["contacts"]["pointCount"] = 0
    w["bodies"]["type"] = wire.BODY_STATIC
    w["joints"]["type"][2] = wire.JOINT_MOUSE
    r = ref.record(w, params, wire.METRICS_ALL, 0)
    assert (float(r["minGap"]), int(r["minGapSlot"]), float(r["maxApproachSpeed"]), int(r["maxApproachSlot"])) == (0.0, -1, 0.0, -1)
    assert (int(r["revoluteJoints"]), int(r["maxJointGapSlot"]), float(r["maxJointGapSquared"])) == (0, -1, -1.0)
    assert r.tobytes()[16:32] == bytes(16) and r.tobytes()[48:80] == bytes(32)
    # equal gaps: the lowest slot; a NaN never wins, and a NaN sum is a NaN
    w = hand_world()
    w["contacts"][2] = w["contacts"][1]
    w["contacts"][0] = w["contacts"][1]
    w["pairs"]["shapeA"][0] = 0
    w["contacts"]["points"]["separation"][0, 0] = np.nan
    r = ref.record(w, params, wire.METRICS_CONTACTS, 0)
    assert (int(r["touchingContacts"]), int(r["touchingPoints"]), int(r["penetratingPoints"])) == (3, 6, 2)
    assert (float(r["minGap"]), int(r["minGapSlot"]), int(r["maxApproachSlot"])) == (-0.09375, 1, 0)
    assert float(r["sumPenetration"]) == 0.1875 and float(r["sumNormalImpulse"]) == 5.25
    w["contacts"]["points"]["normalImpulse"][2, 1] = np.nan
    assert np.isnan(ref.record(w, params, wire.METRICS_CONTACTS, 0)["sumNormalImpulse"])


def tree_sum(x):
    """the pairwise tree over a power-of-two block, written as the recursion it is"""
    if len(x) == 1:
        return f32(x[0])
    half = len(x) // 2
    return f32(tree_sum(x[:half]) + tree_sum(x[half:]))


def test_psum_is_pinned_on_600_terms():
    """t[0] = 2^24, every other term 1: left to right every + 1 is rounded away; the tree adds 1 + 1 first, and every partial sum is an even
    number below 2^25, so PSUM is exact: tile 0 = 2^24 + 254, tile 1 = 256, tile 2 = 88 (padded with +0), in that order."""
    terms = np.ones(600, dtype=f32)
    terms[0] = 2.0 ** 24
    left_to_right = f32(0)
    for t in terms:
        left_to_right = f32(left_to_right + t)
    assert float(left_to_right) == 2.0 ** 24  # (2^24 + 1 rounds to even, 600 times)
    got = ref.psum(terms)
    assert got.dtype == f32 and float(got) == 2.0 ** 24 + 598 and got.tobytes() != left_to_right.tobytes()
    # ... and on random terms of mixed magnitude: the tile tree by recursion, the tiles left to right; other bits than a plain loop
    rng = np.random.default_rng(7)
    terms = (rng.standard_normal(600) * 10.0 ** rng.integers(-3, 4, 600)).astype(f32)
    padded = np.zeros(768, dtype=f32)
    padded[:600] = terms
    want = f32(0)
    for tile in padded.reshape(3, 256):
        want = f32(want + tree_sum(tile))
    plain = f32(0)
    for t in terms:
        plain = f32(plain + t)
    assert ref.psum(terms).tobytes() == want.tobytes() and want.tobytes() != plain.tobytes()
    assert ref.psum(np.zeros(0, dtype=f32)).tobytes() == f32(0).tobytes() and ref.psum(np.array([-0.0], dtype=f32)).tobytes() == f32(0).tobytes()
    assert ref.psum(terms[:256]).tobytes() == tree_sum(terms[:256]).tobytes()


def chain_records(name, steps=3):
    params, world = golden(name)
    out = []
    for step in range(steps):
        world_chain.oracle_world_step(params, world)
        out.append(ref.record(world, params, wire.METRICS_ALL, step))
    return out


def test_the_statement_separates_the_solvers_on_the_oracle_chain():
    """Pool order, three steps.  Measured on the CPU oracle: pyramid8_TGS_Soft minGap -0.0012 with 0 penetrating points,
    high_mass_ratio1_PGS_NGS -0.338 with 512."""
    r = chain_records("pyramid8_TGS_Soft")[-1]
    print("pyramid8_TGS_Soft", r)
    assert float(r["minGap"]) >= -0.005 and int(r["penetratingPoints"]) == 0 and int(r["touchingPoints"]) > 0
    r = chain_records("high_mass_ratio1_PGS_NGS")[-1]
    print("high_mass_ratio1_PGS_NGS", r)
    assert float(r["minGap"]) <= -0.1 and int(r["penetratingPoints"]) >= 100


@pytest.mark.parametrize("name", GPU_WORLDS + ("pyramid8_TGS_Soft",))
def test_all_sums_are_finite_on_the_worlds_used(name):
    for r in chain_records(name):
        for field in FLOAT_SUMS:
            assert np.isfinite(r[field]).all(), (name, field, r)
        assert int(r["energyBodies"]) > 0


@hostcheck_util.needs_sanitizers
def test_step_metrics_host_code_under_asan_and_ubsan(tmp_path):
    """tests/hostcheck/step_metrics_main.cpp, a program of its own: every flag combination -> lengths 1, 5 and 4096 -> more steps than the
    ring holds -> both getters with too-small, exact and ample buffers -> restarts by the setter and by an upload -> uploads with other
    capacities -> destroy, on the sanitizer build of tests/test_hostcheck.py (kernels never run there: what is checked is that the host
    code, the wrap split of the history copy included, touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "step_metrics_main.cpp", "STEP METRICS MAIN OK", timeout=600)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch():
    """hipcc's own report for step_metrics.hip (`make resources` compiles it with the files tests/test_kernel_resources.py reads), through
    tools/kernel_resources.py: both kernels are there, neither has a private frame."""
    # (the kernels live in an unnamed namespace: told by their mangled names; the report file itself is the make target)
    kernels = {"metricsGatherKernel": 1, "metricsFinishKernel": 1}
    hostcheck_util.assert_kernel_resources(None, "resources_step_metrics.txt", kernels, floor=4)  # (nothing here needs many registers: 256 threads, a few dozen VGPRs)
