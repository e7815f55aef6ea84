"""The joint report of the resident world (s2amd_world_set_joint_report / _joint_states / _joint_limit_events / _body_joint_sums /
_joint_summary; solver2d_amd/csrc/joint_report.hip) against its numpy statement (tests/joint_report_ref.py) on the oracle chain of
tests/world_chain.py, stepped in the contact and joint orders the device reports: every list, every record, every sum and the summary
equal byte for byte, every step."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import common, contact_report_ref, joint_report_ref as ref, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, refuses, step_both, upload
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

STEPS = 12


def new_totals():
    return {"began": 0, "ended": 0, "lower": 0, "upper": 0, "max_degree": 0}


def assert_joint_report_equals_reference(s, prev_mask, world, what, totals=None):
    """The four getters against the reference statement on `world` (the oracle chain after the step) and the limit state before it."""
    want = ref.states(world)
    got = s.world_joint_states(expected=max(len(want), 1))
    assert len(got) == len(want), "%s: %d joint states, reference %d" % (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: joint states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))
    want_began, want_ended = ref.events(prev_mask, world)
    began, ended = s.world_joint_limit_events()
    assert began.tolist() == want_began.tolist(), what + ": limits began"
    assert ended.tolist() == want_ended.tolist(), what + ": limits ended"
    want_sums = ref.body_sums(world)
    sums = s.world_body_joint_sums()
    if sums.tobytes() != want_sums.tobytes():
        rows = np.flatnonzero([sums[i].tobytes() != want_sums[i].tobytes() for i in range(len(sums))])
        raise AssertionError("%s: body joint sums differ in rows %s: %s / %s" % (what, rows[:5].tolist(), sums[rows[:3]], want_sums[rows[:3]]))
    want_summary = ref.summary(world)
    summary = s.world_joint_summary()
    assert summary.tobytes() == want_summary.tobytes(), "%s: summary %s, reference %s" % (what, summary, want_summary)
    if totals is not None:
        totals["began"] += len(began)
        totals["ended"] += len(ended)
        totals["lower"] += int((np.concatenate([began, ended]) % 2 == 0).sum())
        totals["upper"] += int((np.concatenate([began, ended]) % 2 == 1).sum())
        totals["max_degree"] = max(totals["max_degree"], int(sums["joints"].max()) if len(sums) else 0)


def run_chain(s, params, world, what, steps=STEPS):
    ref_world = world_chain.copy_world(world)
    totals = new_totals()
    upload(s, world)
    prev = ref.limit_mask(ref_world["joints"])
    for step in range(steps):
        step_both(s, params, ref_world)
        assert_joint_report_equals_reference(s, prev, ref_world, "%s step %d" % (what, step), totals)
        prev = ref.limit_mask(ref_world["joints"])
    got, _ = download(s, world)
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    assert np.isfinite(ref_world["bodies"]["position"]).all(), what
    return totals, ref_world


@pytest.mark.parametrize("name,live,revolute,free", [("far_ragdoll_pile0_PGS_Soft", 60, 60, 3), ("mixed24_PGS", 10, 9, 3),
                                                     ("ragdoll0_PGS_NGS_Block", None, None, None), ("joint_grid6_TGS_NGS", None, None, None)])
def test_golden_worlds_report_every_step(name, live, revolute, free):
    params, world = golden(name)
    joints = world["joints"]
    if live is not None:
        # the input is what the test says it is
        assert int((joints["type"] != wire.JOINT_FREE).sum()) == live and int((joints["type"] == wire.JOINT_REVOLUTE).sum()) == revolute
        assert int((joints["type"] == wire.JOINT_FREE).sum()) == free
    with hip.Solver(0) as s:
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        totals, _ = run_chain(s, params, world, name)
    print(name, totals)
    if name.startswith("far_ragdoll_pile0"):
        live_joints = joints[joints["type"] != wire.JOINT_FREE]
        assert (live_joints["enableLimit"] != 0).all() and (live_joints["enableMotor"] != 0).all()
        # the test cannot pass on joints that never reach a limit: the CPU oracle chain in pool order has 25 limit-state changes in these
        # 12 steps, with 12-16 joints at their lower and 4-11 at their upper limit; the device sweeps in another order, hence the margin
        assert totals["began"] + totals["ended"] >= 5 and totals["lower"] >= 1 and totals["upper"] >= 1, totals


def star_world():
    """The smallest input that crosses both kernel boundaries: a hub with more than 64 adjacency entries and live joints on both sides
    of slot 256.  A static body 0; a dynamic hub (body 1) pinned to it; 70 arms of two unit-mass bodies each, at radius 2 and 4, joined
    hub -> arm -> tip; 141 revolute joints and one mouse joint spread over 302 joint slots; nothing collides."""
    arms = 70
    nb = 2 + 2 * arms
    bodies = np.zeros(nb, dtype=wire.body_dtype)
    synthetic._static_body(bodies[0], 0.0, 0.0)
    synthetic._dynamic_body(bodies[1], 0.0, 0.0, 4.0, 2.0)
    joints = np.zeros(302, dtype=wire.joint_dtype)
    joints["type"] = wire.JOINT_FREE
    joints["bodyA"] = joints["bodyB"] = -1
    listed = [(0, 1, (0.0, 0.0), (0.0, 0.0), True)]  # (bodyA, bodyB, anchorA, anchorB, limited)
    for k in range(arms):
        angle = 2.0 * np.pi * k / arms
        c, sn = np.float32(np.cos(angle)), np.float32(np.sin(angle))
        arm, tip = 2 + 2 * k, 3 + 2 * k
        synthetic._dynamic_body(bodies[arm], 2.0 * c, 2.0 * sn, 1.0, 0.5)
        synthetic._dynamic_body(bodies[tip], 4.0 * c, 4.0 * sn, 1.0, 0.5)
        listed.append((1, arm, (c, sn), (-c, -sn), True))
        listed.append((arm, tip, (c, sn), (-c, -sn), k % 3 == 0))
    for n, (a, b, la, lb, limited) in enumerate(listed):
        j = joints[2 * n + 1 if n % 5 == 0 else 2 * n]
        j["type"], j["bodyA"], j["bodyB"] = wire.JOINT_REVOLUTE, a, b
        j["localOriginAnchorA"], j["localOriginAnchorB"] = la, lb
        if limited:
            j["enableLimit"], j["lowerAngle"], j["upperAngle"] = 1, -0.02, 0.03
        if n % 7 == 0:
            j["enableMotor"], j["motorSpeed"], j["maxMotorTorque"] = 1, 1.0, 5.0
    m = joints[299]
    assert m["type"] == wire.JOINT_FREE
    m["type"], m["bodyA"], m["bodyB"] = wire.JOINT_MOUSE, 0, 3
    m["targetA"], m["hertz"], m["dampingRatio"] = (5.0, 1.0), 5.0, 0.7
    shapes = np.zeros(nb, dtype=wire.shape_dtype)
    for i, b in enumerate(bodies):
        synthetic._box_shape(shapes[i], i, b["type"], 0.125, 0.125, b["position"][0], b["position"][1], i)
    shapes["maskBits"] = 0
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    origins = np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": shapes, "pairs": pairs, "origins": origins}


def assert_star_crosses_both_boundaries(world):
    joints = world["joints"]
    live = np.flatnonzero(joints["type"] != wire.JOINT_FREE)
    assert len(live) == 142 and int((live >= 256).sum()) >= 1 and int((live < 256).sum()) >= 1
    revolute = joints[joints["type"] == wire.JOINT_REVOLUTE]
    hub_degree = int((revolute["bodyA"] == 1).sum() + (revolute["bodyB"] == 1).sum())
    assert hub_degree >= 65, hub_degree


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "PGS_NGS_Block", "Jacobi"])
def test_star_world_crosses_the_wave_and_the_tile(solver_name):
    """A hub of degree 71 (its sum is gathered in two batches of the wave that owns it) and joints beyond slot 256 (two tiles).  On the
    CPU oracle chain in pool order the limit-state changes of these 12 steps number several hundred under TGS_Soft and well over a
    hundred under PGS_NGS_Block and Jacobi; 50 are required of the device's chain."""
    world = star_world()
    assert_star_crosses_both_boundaries(world)
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        totals, _ = run_chain(s, params, world, "star " + solver_name)
    print(solver_name, totals)
    assert totals["began"] + totals["ended"] >= 50 and totals["max_degree"] >= 65, totals


def test_star_world_under_xpbd_reports_no_limit_events():
    """s2Solve_XPBD stores no limit impulses: the lists are empty while the states and the sums still match."""
    world = star_world()
    vel, pos = common.DEFAULT_ITERS["XPBD"]
    params = wire.StepParams.make("XPBD", 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        totals, ref_world = run_chain(s, params, world, "star XPBD")
    assert totals["began"] == 0 and totals["ended"] == 0 and totals["max_degree"] >= 65, totals
    assert not ref.limit_mask(ref_world["joints"]).any()


def test_report_off_changes_nothing_and_the_getters_refuse():
    """Two solvers in lockstep on the ragdoll pile, one with every joint flag and one with none: the same world bytes, step counters and
    stage-3 status every step; without a flag the getters refuse."""
    params, world = golden("far_ragdoll_pile0_PGS_Soft")
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    with hip.Solver(0) as on, hip.Solver(0) as off:
        off_getters = (off.world_joint_states, off.world_joint_limit_events, off.world_body_joint_sums, off.world_joint_summary)
        for getter in off_getters:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                getter()  # no resident world
        on.world_set_joint_report(wire.JOINT_REPORT_ALL)
        upload(on, world), upload(off, world)
        for step in range(STEPS):
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            assert len(on.world_joint_states()) == 60
            on.world_joint_limit_events(), on.world_body_joint_sums(), on.world_joint_summary()
            for getter in off_getters:
                with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                    getter()
            (wa, sa), (wb, sb) = download(on, world), download(off, world)
            assert np.array_equal(sa, sb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert a["activeContacts"] >= 1, a


def test_both_reports_on_at_once():
    """The contact report and the joint report together on a world with contacts and joints: each equals its own statement."""
    params, world = golden("mixed24_PGS")
    ref_world = world_chain.copy_world(world)
    touching_seen = 0
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        upload(s, world)
        prev_touch = contact_report_ref.before_of(ref_world["contacts"])
        prev_limits = ref.limit_mask(ref_world["joints"])
        for step in range(STEPS):
            step_both(s, params, ref_world)
            what = "mixed24 step %d" % step
            assert_joint_report_equals_reference(s, prev_limits, ref_world, what)
            want_began, want_ended = contact_report_ref.events(prev_touch, ref_world)
            began, ended = s.world_touch_events()
            assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
            want_touching = contact_report_ref.touching(ref_world)
            touching_seen = max(touching_seen, len(want_touching))
            assert s.world_touching(expected=max(len(want_touching), 1)).tobytes() == want_touching.tobytes(), what
            assert s.world_body_sums().tobytes() == contact_report_ref.body_sums(ref_world).tobytes(), what
            prev_touch = contact_report_ref.touching_mask(ref_world)
            prev_limits = ref.limit_mask(ref_world["joints"])
    assert touching_seen >= 1


def test_flag_subsets_unknown_bits_and_timing():
    params, world = golden("far_ragdoll_pile0_PGS_Soft")
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        for bad in (8, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_joint_report(bad)
        s.world_set_joint_report(wire.JOINT_REPORT_LIMITS)
        upload(s, world)
        refuses(s, E_STATE, ("world_joint_limit_events", "world_joint_summary", "world_joint_states"))  # no step has run since the flag was set
        prev = ref.limit_mask(ref_world["joints"])
        step_both(s, params, ref_world)
        want_began, want_ended = ref.events(prev, ref_world)
        began, ended = s.world_joint_limit_events()
        assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist()
        assert s.world_joint_summary().tobytes() == ref.summary(ref_world).tobytes()  # any flag will do
        refuses(s, E_STATE, ("world_joint_states", "world_body_joint_sums"))
        # a flag set between two steps takes effect from the next step
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        refuses(s, E_STATE, ("world_joint_states", "world_body_joint_sums"))
        prev = ref.limit_mask(ref_world["joints"])
        step_both(s, params, ref_world)
        assert_joint_report_equals_reference(s, prev, ref_world, "all flags from the second step")
        # ... and one cleared as well; the limit state keeps advancing while nobody asks for the lists
        s.world_set_joint_report(wire.JOINT_REPORT_BODY_SUMS)
        step_both(s, params, ref_world)
        assert s.world_body_joint_sums().tobytes() == ref.body_sums(ref_world).tobytes()
        refuses(s, E_STATE, ("world_joint_states", "world_joint_limit_events"))
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        prev = ref.limit_mask(ref_world["joints"])
        step_both(s, params, ref_world)
        assert_joint_report_equals_reference(s, prev, ref_world, "after a step without the limits flag")


def test_capacity_errors_and_a_second_upload():
    """Through the raw C calls: a buffer one entry too small gives S2AMD_E_CAPACITY with the true counts; the same call with room
    succeeds.  Then the downloaded state uploaded again: "before" is taken from the uploaded joints, so the next step's `began` is not
    the whole at-limit set."""
    params, world = golden("far_ragdoll_pile0_PGS_Soft")
    ref_world = world_chain.copy_world(world)
    ref_world["joints"]["lowerImpulse"] = 0  # every limit that is active after the first step begins in it
    ref_world["joints"]["upperImpulse"] = 0
    world = world_chain.copy_world(ref_world)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        upload(s, world)
        step_both(s, params, ref_world)
        want_began, want_ended = ref.events(np.zeros(2 * len(world["joints"]), dtype=bool), ref_world)
        n = len(want_began)
        assert n >= 2 and len(want_ended) == 0, (n, len(want_ended))
        nb, ne = ctypes.c_int32(-7), ctypes.c_int32(-7)
        began = np.full(n, -1, dtype=np.int32)
        rc = L.s2amd_world_joint_limit_events(h, wire.as_ptr(began), n - 1, ctypes.byref(nb), None, 0, ctypes.byref(ne))
        assert (rc, nb.value, ne.value) == (E_CAPACITY, n, 0) and (began == -1).all()
        rc = L.s2amd_world_joint_limit_events(h, wire.as_ptr(began), n, ctypes.byref(nb), None, 0, ctypes.byref(ne))
        assert (rc, nb.value, ne.value) == (0, n, 0) and began.tolist() == want_began.tolist()
        out = np.zeros(60, dtype=wire.joint_state_dtype)
        count = ctypes.c_int32(-7)
        rc = L.s2amd_world_joint_states(h, wire.as_ptr(out), 59, ctypes.byref(count))
        assert (rc, count.value) == (E_CAPACITY, 60) and out.tobytes() == bytes(60 * 64)
        rc = L.s2amd_world_joint_states(h, wire.as_ptr(out), 60, ctypes.byref(count))
        assert (rc, count.value) == (0, 60) and out.tobytes() == ref.states(ref_world).tobytes()
        sums = np.zeros(len(world["bodies"]), dtype=wire.body_joint_sum_dtype)
        assert L.s2amd_world_body_joint_sums(h, wire.as_ptr(sums), len(sums) - 1) == E_CAPACITY
        assert L.s2amd_world_body_joint_sums(h, wire.as_ptr(sums), len(sums)) == 0 and sums.tobytes() == ref.body_sums(ref_world).tobytes()
        # the Python getters, asked afterwards, see the same step
        b2, e2 = s.world_joint_limit_events(expected=1)
        assert b2.tolist() == want_began.tolist() and e2.tolist() == []

        # a second upload, of the state as it stands
        state, _ = download(s, world)
        world_chain.assert_device_equals_oracle(state, ref_world, "before the second upload")
        upload(s, state)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_joint_limit_events()  # no step since the upload
        prev = ref.limit_mask(ref_world["joints"])
        assert int(prev.sum()) == n
        step_both(s, params, ref_world)
        assert_joint_report_equals_reference(s, prev, ref_world, "the step after the second upload")
        began, _ = s.world_joint_limit_events()
        at_limit = np.flatnonzero(ref.limit_mask(ref_world["joints"]))
        assert len(at_limit) >= 2 and len(began) < len(at_limit), (began.tolist(), at_limit.tolist())
