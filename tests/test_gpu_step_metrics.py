"""The step metrics of the resident world (s2amd_world_set_metrics / _metrics / _metrics_history; solver2d_amd/csrc/step_metrics.hip) against
their numpy statement (tests/step_metrics_ref.py) on the oracle chain of tests/world_chain.py, stepped in the contact and joint orders the
device reports: after every step the record equals the statement byte for byte, after the run the history is the records in order and the
downloaded world is the oracle's."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import body_report_ref, body_report_world, common, contact_report_ref, joint_report_ref, shape_report_ref, step_metrics_ref as ref, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, assert_metrics_equal_reference, assert_record, download, refuses, step_both, upload
from tests.world_chain import _create_contacts, golden, oracle_find_pairs, oracle_world_step

pytestmark = pytest.mark.gpu

ALL = wire.METRICS_ALL
f32 = np.float32


def run_chain(s, params, world, what, steps, flags=ALL):
    """upload -> `steps` steps, the record checked after each -> the world checked; returns the reference records"""
    ref_world = world_chain.copy_world(world)
    upload(s, world)
    records = []
    for step in range(steps):
        step_both(s, params, ref_world)
        records.append(assert_metrics_equal_reference(s, ref_world, params, flags, step, "%s step %d" % (what, step)))
    got, _ = download(s, world)
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    return records, ref_world


def assert_history(s, records, what):
    got = s.world_metrics_history()
    assert len(got) == len(records), "%s: %d records, expected %d" % (what, len(got), len(records))
    for k, want in enumerate(records):
        assert_record(got[k], want, "%s: history entry %d" % (what, k))


@pytest.mark.parametrize("name", ["far_ragdoll_pile0_PGS_Soft", "high_mass_ratio1_PGS_NGS", "tumbler60_TGS_Soft", "mixed24_Jacobi", "circle_pile20_XPBD",
                                  "joint_grid6_TGS_NGS"])
def test_golden_worlds_record_every_step(name):
    """12 steps, all flags, a ring of 16: far_ragdoll_pile0 has 1,066 contact slots (five tiles) and 60 revolute joints, high_mass_ratio1
    most of its 474 slots touching (417 after three steps of the CPU chain, 354 after twelve), tumbler60 711 slots, mixed24 revolute and mouse joints, joint_grid6 no touching contact (the -1 sentinels)."""
    params, world = golden(name)
    with hip.Solver(0) as s:
        s.world_set_metrics(ALL, 16)
        records, ref_world = run_chain(s, params, world, name, 12)
        assert_history(s, records, name)
    last = records[-1]
    print(name, last)
    assert [int(r["step"]) for r in records] == list(range(12))
    if name == "far_ragdoll_pile0_PGS_Soft":
        assert len(world["contacts"]) == 1066 and int(last["revoluteJoints"]) == 60 and int(last["touchingContacts"]) >= 50
    if name == "high_mass_ratio1_PGS_NGS":
        assert len(world["contacts"]) == 474 and int(last["touchingContacts"]) >= 300 and int(last["penetratingPoints"]) >= 100
    if name == "tumbler60_TGS_Soft":
        assert len(world["contacts"]) == 711 and int(last["touchingContacts"]) > 0
    if name == "mixed24_Jacobi":
        types = set(world["joints"]["type"].tolist())
        assert wire.JOINT_REVOLUTE in types and wire.JOINT_MOUSE in types and int(last["maxJointGapSlot"]) >= 0
    if name == "joint_grid6_TGS_NGS":
        assert (int(last["touchingContacts"]), int(last["minGapSlot"]), int(last["maxApproachSlot"])) == (0, -1, -1)
        assert float(last["minGap"]) == 0.0 and float(last["maxApproachSpeed"]) == 0.0 and int(last["revoluteJoints"]) > 0


@pytest.mark.parametrize("steps", [8, 36])
def test_wreck_world_with_contacts_created_during_the_run(steps):
    """wreck_world(1, 24): 303 body slots (two tiles) and 2,244 contact slots (nine tiles), the whole loop with pair query and contact
    creation.  On the CPU chain the ball reaches the pile in step 31 (20 contacts created there, 51 by step 36): the 8-step run steps
    the loop, the 36-step run also creates contacts."""
    world = world_chain.wreck_world(1, 24)
    assert len(world["bodies"]) == 303 and len(world["contacts"]) == 2244
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)
    ref_world = world_chain.copy_world(world)
    created = 0
    records = []
    with hip.Solver(0) as s:
        s.world_set_metrics(ALL, 64)
        upload(s, world)
        for step in range(steps):
            if world_chain.moved_any(ref_world):
                got = s.world_find_pairs()
                want = oracle_find_pairs(ref_world)
                assert np.array_equal(got, want), "step %d: new pairs" % step
                if len(got):
                    created += len(got)
                    slots, contacts, pairs = _create_contacts(ref_world, got)
                    s.world_set_contacts(slots, contacts, pairs)
            s.world_step(params)
            order, _ = s.contact_order()
            oracle_world_step(params, ref_world, contact_order=order)
            records.append(assert_metrics_equal_reference(s, ref_world, params, ALL, step, "wreck step %d" % step))
        got_world, _ = download(s, world)
        world_chain.assert_device_equals_oracle(got_world, ref_world, "wreck")
        assert_history(s, records, "wreck")
    print(steps, created, records[-1])
    assert int(records[-1]["touchingContacts"]) >= 700 and int(records[-1]["energyBodies"]) == 302
    if steps > 8:
        assert created >= 10, created


def test_synthetic_world_crosses_the_wave_and_the_tile():
    """body_report_world.synthetic_world(): 640 body slots (three tiles) with free slots in each, 133 joint slots with revolute joints across
    wave and tile boundaries, no touching contact.  6 steps."""
    world = body_report_world.synthetic_world()
    body_report_world.assert_world_is_what_it_says(world)
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", float(body_report_world.DT), vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_metrics(ALL, 8)
        records, _ = run_chain(s, params, world, "synthetic", 6)
        assert_history(s, records, "synthetic")
    last = records[-1]
    assert len(world["bodies"]) == 640 and int((world["bodies"]["type"] == wire.BODY_FREE).sum()) > 0
    assert 0 < int(last["energyBodies"]) < 640 and int(last["revoluteJoints"]) >= 64 and int(last["touchingContacts"]) == 0
    assert float(last["kineticEnergy"]) > 0 and int(last["maxJointGapSlot"]) >= 0


def test_ring_wraps_restarts_and_refuses_small_buffers():
    """A ring of 5 and 12 steps: the history holds steps 7..11, oldest first; capacity 4 gives S2AMD_E_CAPACITY with count 5 and writes
    nothing, capacity 5 succeeds.  A step with flags 0 records nothing; the setter and an upload restart the recorder; a ring of 1."""
    params, world = golden("mixed24_Jacobi")
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.world_set_metrics(ALL, 5)
        records, ref_world = run_chain(s, params, world, "ring of 5", 12)
        assert_history(s, records[7:], "ring of 5")
        assert [int(r["step"]) for r in s.world_metrics_history()] == [7, 8, 9, 10, 11]
        count = ctypes.c_int32(-7)
        out = np.zeros(5, dtype=wire.step_metrics_dtype)
        rc = L.s2amd_world_metrics_history(h, wire.as_ptr(out), 4, ctypes.byref(count))
        assert (rc, count.value) == (E_CAPACITY, 5) and out.tobytes() == bytes(5 * 128)
        rc = L.s2amd_world_metrics_history(h, wire.as_ptr(out), 5, ctypes.byref(count))
        assert (rc, count.value) == (0, 5) and [int(r["step"]) for r in out] == [7, 8, 9, 10, 11]
        assert_history(s, records[7:], "ring of 5, read again")  # reading never clears the ring
        # a step with flags 0 in the middle: nothing recorded, both getters refuse; turning the recorder on again restarts it at step 0
        s.world_set_metrics(0, 0)
        step_both(s, params, ref_world)
        refuses(s, E_STATE, ("world_metrics", "world_metrics_history"))
        s.world_set_metrics(ALL, 5)
        assert len(s.world_metrics_history()) == 0
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_metrics()  # no step since the restart
        step_both(s, params, ref_world)
        first = assert_metrics_equal_reference(s, ref_world, params, ALL, 0, "after the setter's restart")
        step_both(s, params, ref_world)
        second = assert_metrics_equal_reference(s, ref_world, params, ALL, 1, "after the setter's restart, second step")
        assert_history(s, [first, second], "after the setter's restart")
        # the same call again restarts as well
        s.world_set_metrics(ALL, 5)
        assert len(s.world_metrics_history()) == 0
        step_both(s, params, ref_world)
        assert_metrics_equal_reference(s, ref_world, params, ALL, 0, "after the second restart")
        # an upload restarts it; flags and length hold across it
        ref_world = world_chain.copy_world(world)
        upload(s, world)
        assert len(s.world_metrics_history()) == 0
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_metrics()
        again = []
        for step in range(7):
            step_both(s, params, ref_world)
            again.append(assert_metrics_equal_reference(s, ref_world, params, ALL, step, "after the upload, step %d" % step))
        assert_history(s, again[2:], "after the upload")
        # a ring of one record
        s.world_set_metrics(ALL, 1)
        for step in range(3):
            step_both(s, params, ref_world)
            want = assert_metrics_equal_reference(s, ref_world, params, ALL, step, "ring of 1, step %d" % step)
            assert_history(s, [want], "ring of 1")
        got, _ = download(s, world)
        world_chain.assert_device_equals_oracle(got, ref_world, "ring")


@pytest.mark.parametrize("flags", [wire.METRICS_CONTACTS, wire.METRICS_BODIES, wire.METRICS_JOINTS, wire.METRICS_CONTACTS | wire.METRICS_JOINTS])
def test_flag_subsets_leave_the_other_sections_zero(flags):
    params, world = golden("far_ragdoll_pile0_PGS_Soft")
    sections = {wire.METRICS_CONTACTS: (16, 56), wire.METRICS_BODIES: (56, 80), wire.METRICS_JOINTS: (80, 96)}
    with hip.Solver(0) as s:
        s.world_set_metrics(flags, 4)
        records, ref_world = run_chain(s, params, world, "flags %d" % flags, 3, flags)
        got = s.world_metrics().tobytes()
    whole = ref.record(ref_world, params, ALL, 2).tobytes()
    for flag, (lo, hi) in sections.items():
        if flags & flag:
            assert got[lo:hi] == whole[lo:hi] and got[lo:hi] != bytes(hi - lo), flag
        else:
            assert got[lo:hi] == bytes(hi - lo), flag
    assert got[96:] == bytes(32) and int(records[-1]["flags"]) == flags


def test_nothing_else_moves():
    """The metrics and all four reports on at once: each report equals its own statement in the same steps, and the final world is, byte
    for byte, that of the same run with the metrics off."""
    params, world = golden("mixed24_PGS")
    thresholds = (f32(0.2), f32(f32(0.2) * f32(3.4906585)), f32(3) * f32(params.dt))
    steps = 8
    finals = []
    for metrics_on in (True, False):
        ref_world = world_chain.copy_world(world)
        with hip.Solver(0) as s:
            s.world_set_report(wire.REPORT_ALL)
            s.world_set_joint_report(wire.JOINT_REPORT_ALL)
            s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
            s.world_set_body_report(wire.BODY_REPORT_STATES | wire.BODY_REPORT_REST | wire.BODY_REPORT_ISLANDS)
            s.world_set_rest_thresholds(*thresholds)
            if metrics_on:
                s.world_set_metrics(ALL, 4)
            upload(s, world)
            prev_touch = contact_report_ref.before_of(ref_world["contacts"])
            prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
            prev_view = shape_report_ref.in_view(ref_world, None)
            state = body_report_ref.new_state(ref_world)
            for step in range(steps):
                step_both(s, params, ref_world)
                what = "mixed24 step %d, metrics %s" % (step, metrics_on)
                if metrics_on:
                    assert_metrics_equal_reference(s, ref_world, params, ALL, step, what)
                else:
                    with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                        s.world_metrics()
                # the contact report
                want_began, want_ended = contact_report_ref.events(prev_touch, ref_world)
                began, ended = s.world_touch_events()
                assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
                want_touching = contact_report_ref.touching(ref_world)
                assert s.world_touching(expected=max(len(want_touching), 1)).tobytes() == want_touching.tobytes(), what
                assert s.world_body_sums().tobytes() == contact_report_ref.body_sums(ref_world).tobytes(), what
                # the joint report
                want_states = joint_report_ref.states(ref_world)
                assert s.world_joint_states(expected=max(len(want_states), 1)).tobytes() == want_states.tobytes(), what
                want_began, want_ended = joint_report_ref.events(prev_limits, ref_world)
                began, ended = s.world_joint_limit_events()
                assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
                assert s.world_body_joint_sums().tobytes() == joint_report_ref.body_sums(ref_world).tobytes(), what
                assert s.world_joint_summary().tobytes() == joint_report_ref.summary(ref_world).tobytes(), what
                # the shape report
                assert s.world_shape_draws(expected=64).tobytes() == shape_report_ref.draws(ref_world, None).tobytes(), what
                want_entered, want_left = shape_report_ref.events(prev_view, ref_world, None)
                entered, left = s.world_shape_view_events()
                assert entered.tolist() == want_entered.tolist() and left.tolist() == want_left.tolist(), what
                assert s.world_shape_summary().tobytes() == shape_report_ref.summary(ref_world, None).tobytes(), what
                # the body report
                body_step = body_report_ref.advance(state, ref_world, thresholds, params.dt)
                island, island_states = body_report_ref.islands(ref_world, body_step)
                assert s.world_islands(expected=max(len(island_states), 1)).tobytes() == island_states.tobytes(), what
                want_bodies = body_report_ref.states(ref_world, body_step, False, island, island_states)
                assert s.world_body_states(expected=max(len(want_bodies), 1)).tobytes() == want_bodies.tobytes(), what
                assert s.world_body_summary().tobytes() == body_report_ref.summary(ref_world, body_step, island_states).tobytes(), what
                prev_touch = contact_report_ref.touching_mask(ref_world)
                prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
                prev_view = shape_report_ref.in_view(ref_world, None)
            got, status = download(s, world)
            world_chain.assert_device_equals_oracle(got, ref_world, "mixed24, metrics %s" % metrics_on)
            finals.append((got, status))
    (on, status_on), (off, status_off) = finals
    assert np.array_equal(status_on, status_off)
    for k in world_chain.WORLD_KEYS:
        assert np.ascontiguousarray(on[k]).tobytes() == np.ascontiguousarray(off[k]).tobytes(), k


def test_errors():
    params, world = golden("mixed24_PGS")
    with hip.Solver(0) as s:
        refuses(s, E_STATE, ("world_metrics", "world_metrics_history"))  # no resident world
        for flags, length in ((8, 4), (-1, 4), (16 | ALL, 4), (ALL, 0), (ALL, 4097), (wire.METRICS_BODIES, -1)):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_metrics(flags, length)
        s.world_set_metrics(0, 0)      # the length is ignored with flags 0
        s.world_set_metrics(0, 99999)
        upload(s, world)
        refuses(s, E_STATE, ("world_metrics", "world_metrics_history"))  # the recorder is off
        s.world_step(params)
        refuses(s, E_STATE, ("world_metrics", "world_metrics_history"))  # the flags were 0 before the last step
        s.world_set_metrics(ALL, 4096)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_metrics()  # no step since the restart
        assert len(s.world_metrics_history()) == 0
        s.world_step(params)
        assert int(s.world_metrics()["step"]) == 0 and len(s.world_metrics_history()) == 1
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_metrics(ALL, 4097)  # refused: what holds stays, the recorder goes on
        s.world_step(params)
        assert int(s.world_metrics()["step"]) == 1 and [int(r["step"]) for r in s.world_metrics_history()] == [0, 1]
