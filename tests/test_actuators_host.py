"""The actuators without a GPU: the interface as declared and bound with the header's sizes and offsets, the statement
(tests/actuator_ref.py) on hand-made cases -- the clamp's edges, values that are not finite, every status --, the servo's sign pinned
against the solver itself on a motorised pendulum stepped by the oracle chain, the compiler's resource report of the new kernels, and the
host side under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded)."""
import re

import numpy as np

from solver2d_amd import synthetic, wire
from tests import actuator_ref as ref, hostcheck_util, world_chain

CALLS = ("s2amd_world_set_actuators", "s2amd_world_set_actions", "s2amd_world_import_actions", "s2amd_world_actuator_states",
         "s2amd_world_actuator_counts", "s2amd_device_write")
F = np.float32
INF = F(np.inf)


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    records = {"s2amdActuator": wire.actuator_dtype, "s2amdActuatorState": wire.actuator_state_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, records)
    assert (wire.ACTUATOR_SIZE, wire.ACTUATOR_STATE_SIZE) == (64, 48)


def test_header_defines_and_bindings():
    defines = {"S2AMD_MAX_ACTUATORS": wire.MAX_ACTUATORS, "S2AMD_MAX_ACTION_CHANNELS": wire.MAX_ACTION_CHANNELS,
               "S2AMD_ACTUATOR_BODY_FORCE": wire.ACTUATOR_BODY_FORCE, "S2AMD_ACTUATOR_BODY_THRUST": wire.ACTUATOR_BODY_THRUST,
               "S2AMD_ACTUATOR_BODY_LINEAR_VELOCITY": wire.ACTUATOR_BODY_LINEAR_VELOCITY,
               "S2AMD_ACTUATOR_BODY_ANGULAR_VELOCITY": wire.ACTUATOR_BODY_ANGULAR_VELOCITY,
               "S2AMD_ACTUATOR_REVOLUTE_MOTOR_SPEED": wire.ACTUATOR_REVOLUTE_MOTOR_SPEED, "S2AMD_ACTUATOR_REVOLUTE_SERVO": wire.ACTUATOR_REVOLUTE_SERVO,
               "S2AMD_ACTUATOR_MOUSE_TARGET": wire.ACTUATOR_MOUSE_TARGET, "S2AMD_ACTUATOR_DISABLED": wire.ACTUATOR_DISABLED,
               "S2AMD_ACTUATOR_STATUS_APPLIED": ref.APPLIED, "S2AMD_ACTUATOR_STATUS_DISABLED": ref.DISABLED,
               "S2AMD_ACTUATOR_STATUS_SKIPPED": ref.SKIPPED, "S2AMD_ACTUATOR_STATUS_NONFINITE": ref.NONFINITE, "S2AMD_API_VERSION": 5}
    header = hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_ACTUATORS, wire.MAX_ACTION_CHANNELS, wire.API_VERSION) == (16384, 65536, 5)
    assert wire.ACTUATOR_WIDTH == {1: 2, 2: 1, 3: 2, 4: 1, 5: 1, 6: 1, 7: 2}
    # the notes under the edits and the fields point here for values in device memory
    assert len(re.findall(r"lists in device memory \([^)]*s2amd_world_set_actuators", header)) == 2


# ---- the statement on hand-made cases ----
def tiny_world():
    """bodies: 0 static, 1 dynamic rotated by 90 degrees, 2 free, 3 dynamic; joints: 0 revolute between 1 and 3, 1 mouse on 3, 2 free"""
    bodies = np.zeros(4, dtype=wire.body_dtype)
    bodies["rot"] = (0.0, 1.0)
    bodies["type"] = (wire.BODY_STATIC, wire.BODY_DYNAMIC, wire.BODY_FREE, wire.BODY_DYNAMIC)
    bodies["rot"][1] = (1.0, 0.0)
    bodies["force"][1] = (0.5, 0.25)
    joints = np.zeros(3, dtype=wire.joint_dtype)
    joints["type"] = (wire.JOINT_REVOLUTE, wire.JOINT_MOUSE, wire.JOINT_FREE)
    joints["bodyA"], joints["bodyB"] = (1, 3, 0), (3, 3, 0)
    joints["referenceAngle"][0] = 0.25
    return {"bodies": bodies, "joints": joints}


def one(kind, target, actions, **kw):
    world = tiny_world()
    actuators = wire.actuator_list([wire.actuator(kind, target, 0, **kw)])
    assert ref.valid(actuators, len(actions), len(world["bodies"]), len(world["joints"])) == -1
    edits, states, counts = ref.apply(world, actuators, np.array(actions, dtype=F))
    return world, edits, states[0], counts


def bits(x):
    return np.array(x, dtype=F).view(np.uint32).tolist()


def test_clamp_edges():
    # t exactly at a bound is not replaced by it: -0.0 at lower = +0.0 keeps its sign, as the two comparisons say (the bias is -0.0
    # too: -0.0 + +0.0 would be +0.0)
    assert bits(ref.command(F(-0.0), 1.0, -0.0, 0.0, 1.0)) == bits(F(-0.0)) and bits(ref.command(F(-0.0), 1.0, 0.0, 0.0, 1.0)) == bits(F(0.0))
    assert ref.command(F(2.0), 0.5, 0.0, 1.0, 3.0) == F(1.0) and ref.command(F(2.0), 0.5, 2.0, 1.0, 3.0) == F(3.0)
    assert ref.command(F(2.0), 0.5, 2.5, 1.0, 3.0) == F(3.0) and ref.command(F(-9.0), 0.5, 0.0, 1.0, 3.0) == F(1.0)
    # one rounding per operation: 1/3 * 3 is 1 in float32, and 2^24 + 1 is 2^24
    assert ref.command(F(3.0), F(1.0) / F(3.0), 0.0, -INF, INF) == F(F(1.0 / 3.0) * F(3.0))
    assert ref.command(F(1.0), F(2.0 ** 24), 1.0, -INF, INF) == F(2.0 ** 24)
    # infinite bounds let everything through, an overflowing product included ...
    big = F(3.0e38)
    assert ref.command(big, 2.0, 0.0, -INF, INF) == INF and ref.command(big, -2.0, 0.0, -INF, INF) == -INF
    # ... and finite bounds catch it
    assert ref.command(big, 2.0, 0.0, -5.0, 7.0) == F(7.0) and ref.command(big, -2.0, 0.0, -5.0, 7.0) == F(-5.0)
    # through the whole statement: the force a BODY_FORCE adds is the command
    world, edits, st, counts = one(wire.ACTUATOR_BODY_FORCE, 1, [3.0e38, -1.0], gain=2.0, bias=0.5, lower=-0.25, upper=8.0)
    assert st["status"] == ref.APPLIED and st["command"].tolist() == [8.0, -0.25] and st["output"].tolist() == [8.0, -0.25]
    assert world["bodies"]["force"][1].tolist() == [8.5, 0.0] and counts.tolist() == [1, 0, 0, 0]
    assert len(edits) == 1 and edits[0]["kind"] == wire.EDIT_BODY_APPLY_FORCE_TO_CENTER


def test_values_that_are_not_finite_yield_no_term():
    for bad in (np.nan, np.inf, -np.inf):
        for actions in ([bad, 1.0], [1.0, bad]):
            for kind, target in ((wire.ACTUATOR_BODY_FORCE, 1), (wire.ACTUATOR_BODY_LINEAR_VELOCITY, 3), (wire.ACTUATOR_MOUSE_TARGET, 1)):
                world, edits, st, counts = one(kind, target, actions, lower=-1.0, upper=1.0)
                before = tiny_world()
                assert st["status"] == ref.NONFINITE and len(edits) == 0 and counts.tolist() == [0, 0, 0, 1], (bad, actions, kind)
                assert bits(st["action"]) == bits(actions) and not st["command"].any() and not st["output"].any()
                assert world["bodies"].tobytes() == before["bodies"].tobytes() and world["joints"].tobytes() == before["joints"].tobytes()
        # a width-1 actuator reads one channel: its neighbour may hold anything
        world, edits, st, counts = one(wire.ACTUATOR_BODY_ANGULAR_VELOCITY, 1, [2.0, bad])
        assert st["status"] == ref.APPLIED and world["bodies"]["angularVelocity"][1] == 2.0 and st["action"].tolist() == [2.0, 0.0]
        assert one(wire.ACTUATOR_REVOLUTE_SERVO, 0, [bad], kp=1.0, max_speed=1.0)[2]["status"] == ref.NONFINITE


def test_every_kind_and_every_status_on_the_tiny_world():
    # the thrust of a body rotated by 90 degrees: its x axis points along +y
    world, edits, st, _ = one(wire.ACTUATOR_BODY_THRUST, 1, [3.0], axis=(1.0, 0.0), gain=2.0)
    assert st["output"].tolist() == [0.0, 6.0] and world["bodies"]["force"][1].tolist() == [0.5, 6.25]
    world, _, st, _ = one(wire.ACTUATOR_BODY_LINEAR_VELOCITY, 0, [1.0, -2.0])
    assert world["bodies"]["linearVelocity"][0].tolist() == [1.0, -2.0]  # whatever the body's type is, as the edit
    world, _, st, _ = one(wire.ACTUATOR_REVOLUTE_MOTOR_SPEED, 0, [1.5], bias=0.25)
    assert world["joints"]["motorSpeed"][0] == 1.75
    world, _, st, _ = one(wire.ACTUATOR_MOUSE_TARGET, 1, [1.0, 2.0])
    assert world["joints"]["targetA"][1].tolist() == [1.0, 2.0]
    # the servo: rot(bodyB) is the identity, rot(bodyA) a quarter turn: the relative angle is -pi/2, minus the reference angle 0.25
    world, _, st, _ = one(wire.ACTUATOR_REVOLUTE_SERVO, 0, [0.0], kp=2.0, max_speed=10.0)
    angle = F(F(-np.pi / 2) - F(0.25))
    assert st["angle"] == angle and st["output"][0] == F(F(2.0) * F(F(0.0) - angle)) and world["joints"]["motorSpeed"][0] == st["output"][0]
    assert one(wire.ACTUATOR_REVOLUTE_SERVO, 0, [0.0], kp=2.0, max_speed=1.5)[2]["output"][0] == F(1.5)
    assert one(wire.ACTUATOR_REVOLUTE_SERVO, 0, [-9.0], kp=2.0, max_speed=1.5)[2]["output"][0] == F(-1.5)
    # skipped: a free body, a free joint, a joint of the other type; disabled reads nothing
    for kind, target in ((wire.ACTUATOR_BODY_FORCE, 2), (wire.ACTUATOR_REVOLUTE_SERVO, 2), (wire.ACTUATOR_REVOLUTE_SERVO, 1), (wire.ACTUATOR_MOUSE_TARGET, 0)):
        world, edits, st, counts = one(kind, target, [1.0, np.nan])
        assert st["status"] == ref.SKIPPED and len(edits) == 0 and counts.tolist() == [0, 0, 1, 0] and not st["command"].any()
        assert world["joints"].tobytes() == tiny_world()["joints"].tobytes() and world["bodies"].tobytes() == tiny_world()["bodies"].tobytes()
    world, edits, st, counts = one(wire.ACTUATOR_BODY_FORCE, 1, [1.0, 2.0], flags=wire.ACTUATOR_DISABLED)
    assert st["status"] == ref.DISABLED and counts.tolist() == [0, 1, 0, 0] and not st["action"].any() and len(edits) == 0


def test_validation_rules_of_the_statement():
    good = wire.actuator_list([wire.actuator(wire.ACTUATOR_BODY_FORCE, 1, 2), wire.actuator(wire.ACTUATOR_REVOLUTE_SERVO, 0, 0, kp=1.0, max_speed=1.0, lower=-1.0, upper=1.0)])
    assert ref.valid(good, 4, 4, 3) == -1 and ref.valid(good, 3, 4, 3) == 0 and ref.valid(good, 4, 1, 3) == 0 and ref.valid(good, 4, 4, 0) == 1
    for name, value in (("kind", 0), ("kind", 8), ("target", -1), ("channel", -1), ("channel", 4), ("flags", 2), ("gain", np.nan), ("bias", np.inf),
                        ("kp", np.nan), ("lower", np.nan), ("upper", np.nan), ("upper", -2.0), ("lower", 2.0), ("lower", np.inf), ("maxSpeed", -1.0), ("maxSpeed", np.nan)):
        wrong = good.copy()
        wrong[name][1] = value
        assert ref.valid(wrong, 4, 4, 3) == 1, (name, value)
    for name in ("axis", "reserved"):
        wrong = good.copy()
        wrong[name][1][1] = 1 if name == "reserved" else np.nan
        assert ref.valid(wrong, 4, 4, 3) == 1, name
    allowed = good.copy()
    allowed["lower"], allowed["upper"], allowed["maxSpeed"][1] = (np.inf, -np.inf), (np.inf, -np.inf), np.inf  # lower == upper, infinities
    assert ref.valid(allowed, 4, 4, 3) == -1
    assert ref.valid(good, 0) == 0 and ref.valid(good, wire.MAX_ACTION_CHANNELS + 1) == 0 and ref.valid(good[:0], 0) == -1


# ---- the servo's sign, against the solver itself ----
def pendulum_world(max_torque):
    """A static hub at the origin and one box whose centre hangs 1 m to its right, pinned to the hub by a motorised revolute joint."""
    bodies = np.zeros(2, dtype=wire.body_dtype)
    synthetic._static_body(bodies[0], 0.0, 0.0)
    synthetic._dynamic_body(bodies[1], 1.0, 0.0, synthetic.BOX_MASS, synthetic.BOX_I)
    joints = np.zeros(1, dtype=wire.joint_dtype)
    j = joints[0]
    j["type"], j["bodyA"], j["bodyB"] = wire.JOINT_REVOLUTE, 0, 1
    j["localOriginAnchorA"], j["localOriginAnchorB"] = (0.0, 0.0), (-1.0, 0.0)
    j["enableMotor"], j["maxMotorTorque"] = 1, max_torque
    shapes = np.zeros(2, dtype=wire.shape_dtype)
    synthetic._box_shape(shapes[0], 0, wire.BODY_STATIC, 0.1, 0.1, 0.0, 0.0, 0)
    synthetic._box_shape(shapes[1], 1, wire.BODY_DYNAMIC, 0.5, 0.5, 1.0, 0.0, 1)
    return {"bodies": bodies, "contacts": np.zeros(0, dtype=wire.contact_dtype), "joints": joints, "shapes": shapes,
            "pairs": np.zeros(0, dtype=wire.pair_state_dtype), "origins": np.ascontiguousarray(bodies["position"]).copy()}


def test_servo_sign_against_the_solver():
    """The servo turns the joint towards its target: in every one of 60 steps the speed has the sign of target - angle, and the error
    after the last step is smaller than before the first -- for a target on either side, under gravity, with a torque the motor can
    hold the box with (m g r = 10 N m)."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    for target in (0.8, -0.6):
        world = pendulum_world(200.0)
        actuators = wire.actuator_list([wire.actuator(wire.ACTUATOR_REVOLUTE_SERVO, 0, 0, kp=6.0, max_speed=2.0)])
        actions = np.array([target], dtype=F)
        errors = []
        for step in range(60):
            _, states, counts = ref.apply(world, actuators, actions)
            assert counts.tolist() == [1, 0, 0, 0]
            error = F(target) - states[0]["angle"]
            errors.append(abs(float(error)))
            speed = states[0]["output"][0]
            assert error != 0 and np.sign(speed) == np.sign(error), (target, step, speed, error)
            assert world["joints"]["motorSpeed"][0] == speed
            world_chain.oracle_world_step(params, world)
        last = abs(float(F(target) - ref.servo_angle(world, 0)))
        assert last < errors[0], (target, errors[0], last)
        print("servo to %+.1f: |error| %.4f -> %.4f" % (target, errors[0], last))


def test_kernels_use_no_scratch():
    """hipcc's own report for actuators.hip (make resources-actuators), through tools/kernel_resources.py: every kernel of the file is
    there, none has a private frame or spills."""
    kernels = dict.fromkeys(("actuatorTermsKernelILb1E", "actuatorTermsKernelILb0E", "actuatorWalkKernel", "reportBodyRangesKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-actuators", "resources_actuators.txt", kernels, floor=4)


@hostcheck_util.needs_sanitizers
def test_actuator_host_code_under_asan_and_ubsan(tmp_path):
    """Every validation rule with and without a world -> the list held across uploads with other capacities -> the grouping's verdict
    (a target twice or not) -> both writers on whole and partial ranges, twice in a row, past the end -> the getters with too-small,
    exact and ample heap buffers of exactly the size passed, before a step, after it, after the list was replaced, refused and cleared
    -> destroy, for 0, 1, 65, 257, 1,000 and 16,384 actuators, on the sanitizer build of tests/test_hostcheck.py (kernels never run
    there)."""
    hostcheck_util.run_sanitized(tmp_path, "actuators_main.cpp", "ACTUATORS MAIN OK", timeout=600)
