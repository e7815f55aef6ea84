"""Actuators on the resident world (s2amd_world_set_actuators / _set_actions / _import_actions / _actuator_states / _actuator_counts;
solver2d_amd/csrc/actuators.hip) against their statement (tests/actuator_ref.py: numpy float32, the servo's angle through glibc's
atan2f, the terms through the statement of s2amd_world_edit), byte for byte.  The pass runs at the head of s2amd_world_step, so every
case steps: the device's world after the step equals the oracle chain of tests/world_chain.py with the statement applied in front of
the step, the states and the counts equal the statement's, and the route through s2amd_world_edit gives the same bytes.  The worlds are
the committed tests/golden/world_*_step*.npz; the sizes need more than 1,024 body slots and take a synthetic pyramid.  Every case
asserts on the statement's own output that its actuators act."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import actuator_ref as ref, force_field_ref, ray_report_ref, ray_report_world as rw, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, OTHER_KEYS, assert_same_world, download, motorised, refuses, slots_of, step_both, upload
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 12
F = np.float32
FORCE, THRUST, LINEAR, ANGULAR, MOTOR, SERVO, MOUSE = range(1, 8)


def assert_states(got, want, what):
    assert got.dtype == wire.actuator_state_dtype and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))


def pass_and_step(s, params, ref_world, actuators, actions, what, world=None):
    """The statement on `ref_world`, one step of both, the states and the counts compared (and the world, given the uploaded arrays to
    download into) -> the statement's (edits, states, counts)"""
    edits, states, counts = ref.apply(ref_world, actuators, actions)
    step_both(s, params, ref_world)
    assert_states(s.world_actuator_states(), states, what)
    assert s.world_actuator_counts().tolist() == counts.tolist(), what
    if world is not None:
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, what)
    return edits, states, counts


def seven_kinds(world):
    at = slots_of(world)
    d = at["dynamic"]
    actuators = wire.actuator_list([
        wire.actuator(SERVO, at["revolute"][0], 0, gain=0.5, kp=4.0, max_speed=3.0), wire.actuator(FORCE, d[0], 1, gain=30.0, bias=1.0),
        wire.actuator(MOUSE, at["mouse"][0], 3, bias=2.0), wire.actuator(THRUST, d[1], 5, gain=25.0, axis=(0.6, 0.8), lower=-10.0, upper=10.0),
        wire.actuator(LINEAR, at["kinematic"][0], 6, gain=2.0), wire.actuator(MOTOR, at["revolute"][1], 8, gain=-3.0),
        wire.actuator(ANGULAR, d[2], 9, bias=-0.5)])
    actions = np.array([0.9, 0.5, -0.25, 1.5, 0.75, 0.7, 0.125, -0.375, 0.6, 1.25], dtype=F)
    return actuators, actions


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
def test_every_kind_once_on_distinct_targets(fast):
    """mixed24_PGS with its motors on: the seven kinds on seven targets.  After the step the world, the states and the counts are the
    statement's; the statement's terms through s2amd_world_edit on a second solver give the same bytes.  Both libraries: the pass is
    the same bits in the tolerance-mode library, whose step is not the oracle's -- there the world is compared with the edit route's
    alone."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    actuators, actions = seven_kinds(world)
    assert sorted(actuators["kind"].tolist()) == list(range(1, 8))
    with hip.Solver(0, fast=fast) as s, hip.Solver(0, fast=fast) as route:
        s.world_set_actuators(actuators, len(actions))
        s.world_set_actions(actions)
        upload(s, world), upload(route, world)
        assert_same_world(download(s, world)[0], world, "upload")  # (the writers touch no world array)
        ref_world, plain = world_chain.copy_world(world), world_chain.copy_world(world)
        before = world_chain.copy_world(world)
        edits, states, counts = pass_and_step(s, params, ref_world, actuators, actions, "mixed24", None if fast else world)
        assert counts.tolist() == [7, 0, 0, 0] and (states["status"] == ref.APPLIED).all() and len(edits) == 7
        # the statement alone changed both arrays, and the step went elsewhere because of it
        alone = world_chain.copy_world(world)
        ref.apply(alone, actuators, actions)
        assert alone["bodies"].tobytes() != before["bodies"].tobytes() and alone["joints"].tobytes() != before["joints"].tobytes()
        assert_same_world(alone, before, "the statement", OTHER_KEYS)
        world_chain.oracle_world_step(params, plain)
        assert plain["bodies"].tobytes() != ref_world["bodies"].tobytes()
        # the route it replaces
        assert route.world_edit(edits) == 0
        route.world_step(params)
        assert_same_world(download(route, world)[0], download(s, world)[0], "the edit route")


def test_order_on_one_target():
    """ragdoll0: 200 actuators of kinds 1-4 on three bodies, interleaved -- every segment of the grouping is longer than a wave and
    starts at an arbitrary lane.  The reversed list gives other bytes for those bodies, so an order error cannot pass."""
    params, world = golden("ragdoll0_PGS_NGS_Block")
    rng = np.random.RandomState(5)
    bodies = slots_of(world)["dynamic"][[1, 4, 7]]
    records, channel = [], 0
    which = rng.permutation(np.arange(200) % 3)  # 67, 67 and 66 to a body, shuffled
    for k in range(200):
        kind = int(rng.choice([FORCE, FORCE, THRUST, THRUST, LINEAR, ANGULAR]))
        records.append(wire.actuator(kind, bodies[which[k]], channel, gain=rng.uniform(-30.0, 30.0), bias=rng.uniform(-1.0, 1.0),
                                     axis=rng.uniform(-1.0, 1.0, 2), lower=-20.0, upper=20.0))
        channel += wire.ACTUATOR_WIDTH[kind]
    actuators = wire.actuator_list(records)
    actions = rng.uniform(-1.0, 1.0, channel).astype(F)
    assert np.bincount(actuators["target"])[bodies].min() > 64 and set(actuators["kind"].tolist()) == {1, 2, 3, 4}
    with hip.Solver(0) as s:
        s.world_set_actuators(actuators, channel)
        s.world_set_actions(actions)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        _, states, counts = pass_and_step(s, params, ref_world, actuators, actions, "ragdoll0, 200 on three bodies", world)
        assert counts.tolist() == [200, 0, 0, 0]
    forward, backward = world_chain.copy_world(world), world_chain.copy_world(world)
    ref.apply(forward, actuators, actions)
    ref.apply(backward, actuators[::-1].copy(), actions)
    assert all(forward["bodies"][b].tobytes() != backward["bodies"][b].tobytes() for b in bodies)


def test_sizes():
    """A base-45 pyramid (1,036 body slots): 1, 63, 64, 65, 257 and 1,024 actuators on distinct bodies -- the one-kernel path across the
    wave, the workgroup and four full workgroups -- and S2AMD_MAX_ACTUATORS on all of them, sixteen to a body -- the walk.  The last
    actuator of every list reads the last channel."""
    world = synthetic.pyramid_world(45)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    live = np.flatnonzero(world["bodies"]["type"] != wire.BODY_FREE)
    assert len(world["bodies"]) > 1024 and len(live) >= 1024
    rng = np.random.RandomState(9)
    with hip.Solver(0) as s:
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        for count in (1, 63, 64, 65, 257, 1024, wire.MAX_ACTUATORS):
            targets = rng.permutation(live)[:count] if count <= len(live) else live[rng.randint(len(live), size=count)]
            kinds = rng.choice([FORCE, THRUST, LINEAR, ANGULAR], size=count, p=[0.4, 0.3, 0.15, 0.15])
            kinds[-1] = FORCE
            starts = np.concatenate([[0], np.cumsum([wire.ACTUATOR_WIDTH[int(k)] for k in kinds])])
            channels = int(starts[-1])
            actuators = np.zeros(count, dtype=wire.actuator_dtype)
            actuators["kind"], actuators["target"], actuators["channel"] = kinds, targets, starts[:-1]
            actuators["gain"], actuators["bias"] = rng.uniform(-2.0, 2.0, count), rng.uniform(-0.1, 0.1, count)
            actuators["lower"], actuators["upper"], actuators["axis"] = -1.0, 1.0, rng.uniform(-1.0, 1.0, (count, 2))
            assert actuators["channel"][-1] + 2 == channels and ref.valid(actuators, channels, len(world["bodies"]), 0) == -1
            assert (len(np.unique(targets)) == count) == (count <= 1024)
            actions = rng.uniform(-1.0, 1.0, channels).astype(F)
            s.world_set_actuators(actuators, channels)
            s.world_set_actions(actions)
            _, states, counts = pass_and_step(s, params, ref_world, actuators, actions, "%d actuators" % count, world)
            assert counts.tolist() == [count, 0, 0, 0] and states["action"][-1].tolist() == actions[-2:].tolist()


def test_hold_and_writers():
    """set_actions on a sub-range leaves the other channels alone; device_write + import_actions give what set_actions gives; two
    steps without a write apply the same actions twice; replacing the list zeroes the buffer."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    actuators, actions = seven_kinds(world)
    n = len(actions)
    with hip.Solver(0) as s:
        s.world_set_actuators(actuators, n)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        held = np.zeros(n, dtype=F)
        _, states, _ = pass_and_step(s, params, ref_world, actuators, held, "the zeroed buffer", world)
        assert not states["action"].any()
        s.world_set_actions(actions)
        held[:] = actions
        pass_and_step(s, params, ref_world, actuators, held, "all channels", world)
        s.world_set_actions(np.array([-0.5, 0.25, 2.0], dtype=F), first=4)
        held[4:7] = (-0.5, 0.25, 2.0)
        _, states, _ = pass_and_step(s, params, ref_world, actuators, held, "a sub-range", world)
        assert states["action"][0][0] == actions[0] and states["action"][3][0] == F(0.25)
        # no write: the same actions again (zero-order hold)
        _, again, _ = pass_and_step(s, params, ref_world, actuators, held, "held", world)
        assert again["action"].tobytes() == states["action"].tobytes()
        # through a caller's device buffer
        buf = s.device_alloc(4 * n)
        try:
            fresh = (actions[::-1] * F(0.5)).astype(F)
            s.device_write(buf, fresh)
            assert s.device_read(buf, (n,), np.float32).tobytes() == fresh.tobytes()
            s.world_import_actions(buf, n)
            pass_and_step(s, params, ref_world, actuators, fresh, "imported", world)
            s.world_import_actions(buf + 4, 2, first=8)  # a sub-range from the middle of the buffer
            fresh[8:10] = fresh[1:3]
            pass_and_step(s, params, ref_world, actuators, fresh, "imported sub-range", world)
        finally:
            s.device_free(buf)
        # a replaced list starts from zeros
        s.world_set_actuators(actuators[:3].copy(), n)
        _, states, _ = pass_and_step(s, params, ref_world, actuators[:3].copy(), np.zeros(n, dtype=F), "replaced", world)
        assert not states["action"].any() and (states["status"] == ref.APPLIED).all()


def test_statuses():
    """A disabled actuator, a free body slot, a free joint slot, a servo on a mouse joint, a mouse target on a revolute joint, a NaN in
    the second component: none of them writes anything; every other actuator is APPLIED."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    at = slots_of(world)
    assert len(at["free"]) and len(at["free_joint"]) and len(at["mouse"]) and len(at["revolute"]) >= 2
    d = at["dynamic"]
    quiet = wire.actuator_list([
        wire.actuator(FORCE, d[0], 0, flags=wire.ACTUATOR_DISABLED), wire.actuator(LINEAR, at["free"][0], 2), wire.actuator(MOTOR, at["free_joint"][0], 4),
        wire.actuator(SERVO, at["mouse"][0], 5, kp=1.0, max_speed=1.0), wire.actuator(MOUSE, at["revolute"][0], 6), wire.actuator(FORCE, d[1], 8)])
    acting = wire.actuator_list([wire.actuator(THRUST, d[2], 10, gain=20.0, axis=(0.0, 1.0)), wire.actuator(SERVO, at["revolute"][1], 11, kp=2.0, max_speed=1.0)])
    actions = np.array([5.0, 5.0, 1.0, 1.0, 2.0, 0.5, 3.0, 3.0, 1.0, np.nan, 0.75, 0.3], dtype=F)
    want_status = [ref.DISABLED, ref.SKIPPED, ref.SKIPPED, ref.SKIPPED, ref.SKIPPED, ref.NONFINITE]
    with hip.Solver(0) as s, hip.Solver(0) as plain:
        # the quiet ones alone: the step is the plain step
        s.world_set_actuators(quiet, len(actions))
        s.world_set_actions(actions)
        upload(s, world), upload(plain, world)
        ref_world = world_chain.copy_world(world)
        edits, states, counts = pass_and_step(s, params, ref_world, quiet, actions, "the quiet ones", world)
        assert len(edits) == 0 and states["status"].tolist() == want_status and counts.tolist() == [0, 1, 4, 1]
        assert not states["command"].any() and not states["output"].any() and not states["action"][0].any()
        plain.world_step(params)
        assert_same_world(download(s, world)[0], download(plain, world)[0], "a pass without terms")
        # among acting ones
        both = np.concatenate([quiet[:3], acting[:1], quiet[3:], acting[1:]])
        s.world_set_actuators(both, len(actions))
        s.world_set_actions(actions)
        edits, states, counts = pass_and_step(s, params, ref_world, both, actions, "quiet among acting", world)
        assert counts.tolist() == [2, 1, 4, 1] and states["status"].tolist() == want_status[:3] + [0] + want_status[3:] + [0] and len(edits) == 2


# ---- chains ----
def chain_case(name):
    """-> (params, world, actuators, channels, scale): motor speeds and servos on the revolute joints, thrusters and forces on a third
    of the dynamic bodies.  ragdoll0 carries a motor speed AND a servo on every joint (targets repeat: the walk), the others alternate."""
    params, world = golden(name)
    world = motorised(world)
    at = slots_of(world)
    records, channel = [], 0
    for k, joint in enumerate(at["revolute"]):
        if name.startswith("ragdoll0") or k % 2 == 1:
            records.append(wire.actuator(MOTOR, joint, channel, gain=3.0))
            channel += 1
        if name.startswith("ragdoll0") or k % 2 == 0:
            records.append(wire.actuator(SERVO, joint, channel, gain=0.8, kp=5.0, max_speed=4.0))
            channel += 1
    for k, body in enumerate(at["dynamic"][::3]):
        if k % 2 == 0:
            records.append(wire.actuator(THRUST, body, channel, gain=60.0, axis=(0.0, 1.0)))
            channel += 1
        else:
            records.append(wire.actuator(FORCE, body, channel, gain=60.0, lower=-50.0, upper=50.0))
            channel += 2
    for k, joint in enumerate(at["mouse"]):
        records.append(wire.actuator(MOUSE, joint, channel, gain=0.5, bias=2.0))
        channel += 2
    return params, world, wire.actuator_list(records), channel


CHAINS = ["ragdoll0_PGS_NGS_Block", "mixed24_PGS", "joint_grid6_TGS_NGS"]


def moved_share(world, actuated, plain):
    """the share of the dynamic bodies whose final record differs between the two chains"""
    dyn = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)
    return sum(actuated["bodies"][b].tobytes() != plain["bodies"][b].tobytes() for b in dyn) / float(len(dyn))


@pytest.mark.parametrize("name", CHAINS)
def test_chains_equal_the_oracle_chain(name):
    """12 steps, the actions redrawn every step and written through set_actions: the world and the states after every step are the oracle
    chain's with the statement applied before each step, and the chain ends elsewhere than the plain chain for most dynamic bodies."""
    params, world, actuators, channels = chain_case(name)
    rng = np.random.RandomState(21)
    kinds = set(actuators["kind"].tolist())
    assert {MOTOR, SERVO, THRUST, FORCE} <= kinds
    with hip.Solver(0) as s:
        s.world_set_actuators(actuators, channels)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        for step in range(STEPS):
            actions = rng.uniform(-1.0, 1.0, channels).astype(F)
            s.world_set_actions(actions)
            _, states, counts = pass_and_step(s, params, ref_world, actuators, actions, "%s step %d" % (name, step), world)
            assert counts.tolist() == [len(actuators), 0, 0, 0]
            if SERVO in kinds:
                assert np.abs(states["output"][actuators["kind"] == SERVO][:, 0]).max() > 0
    plain = world_chain.copy_world(world)
    for _ in range(STEPS):
        world_chain.oracle_world_step(params, plain)
    assert np.isfinite(ref_world["bodies"]["position"]).all()
    assert moved_share(world, ref_world, plain) >= 0.5, name


@pytest.mark.skipif(not force_field_ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
def test_beside_the_force_fields():
    """A DRAG field and a BODY_LINEAR_VELOCITY actuator on one body: the field sees the velocity the actuator set -- actuators, then
    fields, then the step, on the oracle."""
    params, world = golden("mixed24_PGS")
    body = int(slots_of(world)["dynamic"][2])
    fields = wire.field_list([wire.field_drag(world["bodies"]["position"][body], 1.5, 0.8)])
    actuators = wire.actuator_list([wire.actuator(LINEAR, body, 0, gain=4.0)])
    rng = np.random.RandomState(2)
    own_shapes = int(((world["shapes"]["body"] == body) & (world["shapes"]["type"] != wire.SHAPE_FREE)).sum())  # one drag term each
    with hip.Solver(0) as s:
        s.world_set_fields(fields)
        s.world_set_actuators(actuators, 2)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        for step in range(4):
            actions = rng.uniform(-1.0, 1.0, 2).astype(F)
            s.world_set_actions(actions)
            _, states, _ = ref.apply(ref_world, actuators, actions)
            velocity = ref_world["bodies"]["linearVelocity"][body].copy()
            field_states = force_field_ref.apply_in_place(ref_world, fields)
            assert field_states["terms"][0] >= 1
            drag = ref_world["bodies"]["force"][body] - world["bodies"]["force"][body] if step == 0 else None
            step_both(s, params, ref_world)
            assert_states(s.world_actuator_states(), states, "step %d" % step)
            assert s.world_field_states().tobytes() == field_states.tobytes()
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "beside a field, step %d" % step)
            if drag is not None:  # the drag term is -0.8 times the velocity the actuator set, not the uploaded one
                assert velocity.tolist() == (F(4.0) * actions).tolist() and np.allclose(drag, -0.8 * own_shapes * velocity, rtol=1e-5) and velocity.any()


def test_errors():
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    nb, nj = len(world["bodies"]), len(world["joints"])
    good, actions = seven_kinds(world)
    n = len(actions)

    def bad_lists():
        for name, value in (("kind", 0), ("kind", 8), ("target", -1), ("target", nb), ("channel", -1), ("channel", n), ("flags", 2), ("flags", -1),
                            ("gain", np.nan), ("gain", np.inf), ("bias", np.nan), ("bias", -np.inf), ("kp", np.nan), ("kp", np.inf), ("lower", np.nan),
                            ("upper", np.nan), ("lower", 11.0), ("maxSpeed", -1.0), ("maxSpeed", np.nan)):
            wrong = good.copy()
            wrong[name][3] = value  # a bad record in the middle of the list: the thruster (width 1, bounds -10 .. 10)
            yield "%s = %r" % (name, value), wrong
        for name, index, value in (("axis", 0, np.nan), ("axis", 1, np.inf), ("reserved", 0, 1), ("reserved", 3, -1)):
            wrong = good.copy()
            wrong[name][3][index] = value
            yield name, wrong
        wrong = good.copy()
        wrong["target"][0] = nj  # a joint target is measured against the joint capacity ...
        yield "joint target", wrong
        wrong = good.copy()
        wrong["channel"][2] = n - 1  # ... and a width-2 kind needs two channels
        yield "width", wrong

    with hip.Solver(0) as s:
        L, h = s._L, s._h
        for call in (s.world_actuator_states, s.world_actuator_counts):
            call()  # an empty list: nothing to report, no error
        assert len(s.world_actuator_states()) == 0 and s.world_actuator_counts().tolist() == [0, 0, 0, 0]
        # the writers without a list
        assert L.s2amd_world_set_actions(h, wire.as_ptr(actions), 0, n) == E_STATE and L.s2amd_world_import_actions(h, wire.as_ptr(actions), 0, n) == E_STATE
        s.world_set_actuators(good, n)  # accepted before any world
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_actuator_states()
        upload(s, world)
        s.world_set_actions(actions)
        refuses(s, E_STATE, ("world_actuator_states", "world_actuator_counts"))  # no step since the upload
        # per call
        many = np.zeros(wire.MAX_ACTUATORS + 1, dtype=wire.actuator_dtype)
        many[:] = good[1]
        assert L.s2amd_world_set_actuators(h, wire.as_ptr(good), -1, n) == E_INVALID and L.s2amd_world_set_actuators(h, None, 2, n) == E_INVALID
        assert L.s2amd_world_set_actuators(h, wire.as_ptr(many), len(many), n) == E_INVALID
        assert L.s2amd_world_set_actuators(h, wire.as_ptr(good), len(good), 0) == E_INVALID
        assert L.s2amd_world_set_actuators(h, wire.as_ptr(good), len(good), wire.MAX_ACTION_CHANNELS + 1) == E_INVALID
        # per record
        for what, wrong in bad_lists():
            assert ref.valid(wrong, n, nb, nj) >= 0, what
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_actuators(wrong, n)
        # the writers
        buf = s.device_alloc(4 * n)
        try:
            for fn, src in ((L.s2amd_world_set_actions, wire.as_ptr(actions)), (L.s2amd_world_import_actions, ctypes.c_void_p(buf))):
                assert fn(h, None, 0, 1) == E_INVALID and fn(h, src, -1, 1) == E_INVALID and fn(h, src, 0, -1) == E_INVALID
                assert fn(h, src, 1, n) == E_INVALID and fn(h, src, n, 1) == E_INVALID and fn(h, src, n, 0) == 0 and fn(h, None, 0, 0) == 0
            assert L.s2amd_device_write(h, None, wire.as_ptr(actions), 4) == E_INVALID and L.s2amd_device_write(h, ctypes.c_void_p(buf), None, 4) == E_INVALID
        finally:
            s.device_free(buf)
        # the world, the old list and its buffer stand: the next step applies `good` to `actions`
        assert_same_world(download(s, world)[0], world, "after the refusals")
        ref_world = world_chain.copy_world(world)
        pass_and_step(s, params, ref_world, good, actions, "after the refusals", world)
        count = ctypes.c_int32(-7)
        out = np.zeros(len(good), dtype=wire.actuator_state_dtype)
        assert L.s2amd_world_actuator_states(h, wire.as_ptr(out), len(good) - 1, ctypes.byref(count)) == E_CAPACITY and count.value == len(good)
        assert out.tobytes() == bytes(out.nbytes)
        assert L.s2amd_world_actuator_states(h, wire.as_ptr(out), -1, ctypes.byref(count)) == E_INVALID
        assert L.s2amd_world_actuator_counts(h, None) == E_INVALID
        s.world_set_actuators(good[::-1].copy(), n)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_actuator_states()  # no step since the list was set
        # a list whose targets lie outside a smaller world is kept, and skipped there
        small = synthetic.pyramid_world(3)
        upload(s, small)
        s.world_set_actions(actions)
        s.world_step(wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True))
        states = s.world_actuator_states()
        outside = [(k >= MOTOR or t >= len(small["bodies"])) for k, t in zip(good[::-1]["kind"], good[::-1]["target"])]
        assert (states["status"][outside] == ref.SKIPPED).all() and sum(outside) >= 3


def test_no_list_no_cost_in_kind():
    """With no list, or a cleared one, a chain is the plain oracle chain and a step enqueues what a solver that never heard of actuators
    enqueues."""
    params, world = golden("mixed24_PGS")
    actuators, actions = seven_kinds(motorised(world))
    with hip.Solver(0) as never, hip.Solver(0) as cleared:
        cleared.world_set_actuators(actuators, len(actions))
        cleared.world_set_actuators(wire.actuator_list([]), 0)
        upload(never, world), upload(cleared, world)
        ref_world = world_chain.copy_world(world)
        for step in range(STEPS):
            step_both(never, params, ref_world)
            cleared.world_step(params)
            a, b = never.stats(), cleared.stats()
            assert (a["kernelLaunches"], a["solveLaunches"], a["structureBuilds"]) == (b["kernelLaunches"], b["solveLaunches"], b["structureBuilds"]), step
            assert len(cleared.world_actuator_states()) == 0 and len(never.world_actuator_states()) == 0
        got = download(never, world)[0]
        world_chain.assert_device_equals_oracle(got, ref_world, "no list")
        assert_same_world(download(cleared, world)[0], got, "a cleared list")


def closed_loop():
    """The body of test_closed_loop_on_the_device, run in a process of its own in which torch has initialised the device first: the
    library then shares torch's HIP runtime, and a tensor's data_ptr() is a pointer it knows."""
    import torch
    fx = rw.load_fixture("pyramid")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    n = len(rays)
    dyn = slots_of(world)["dynamic"]
    assert n >= 8 and len(dyn) >= n // 2
    # ray k drives channel k: every pair of channels pushes one body
    actuators = wire.actuator_list([wire.actuator(FORCE, dyn[k], 2 * k, gain=8.0, lower=-6.0, upper=6.0) for k in range(n // 2)])
    weight = np.linspace(-1.5, 1.5, n).astype(F)
    offset = np.linspace(0.25, -0.25, n).astype(F)
    observed = torch.zeros(n, dtype=torch.float32, device="cuda")
    w, b = torch.from_numpy(weight).cuda(), torch.from_numpy(offset).cuda()
    with hip.Solver(0) as s:
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(wire.RAY_REPORT_RANGES)
        s.world_set_actuators(actuators, n)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        actions = np.zeros(n, dtype=F)
        acted = 0
        for step in range(6):
            if step > 0:
                s.world_export_ray_ranges(observed.data_ptr(), n)
                policy = torch.add(torch.mul(observed, w), b)
                torch.cuda.synchronize()
                s.world_import_actions(policy.data_ptr(), n)
                ranges = s.world_ray_ranges()
                assert observed.cpu().numpy().tobytes() == ranges.tobytes()
                if ray_report_ref.available():
                    assert ranges.tobytes() == ray_report_ref.ranges(ref_world, rays).tobytes()
                actions = (ranges * weight).astype(F) + offset
                assert policy.cpu().numpy().tobytes() == actions.tobytes()
            _, states, counts = pass_and_step(s, params, ref_world, actuators, actions, "closed loop step %d" % step, world)
            assert counts[0] == len(actuators)
            acted += int(np.abs(states["output"]).sum() > 0)
        assert acted >= 5
    print("CLOSED LOOP OK")


def test_closed_loop_on_the_device():
    """Observation to action without the host: the ray ranges are exported into a torch tensor, a fixed per-channel linear map on the GPU
    makes the actions, torch's stream is synchronised, the tensor is imported, the world steps.  The chain equals the same loop on the
    statement (the map is one multiply and one add per channel: the same roundings in numpy).  In a child process: torch's bundled HIP
    runtime cannot initialise after the library's has taken the device, so torch goes first there."""
    pytest.importorskip("torch")
    code = "import torch; torch.zeros(1, device='cuda'); from tests import test_gpu_actuators as t; t.closed_loop()"
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "CLOSED LOOP OK" in out, out[-4000:]
