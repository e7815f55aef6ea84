"""The body report of the resident world (s2amd_world_set_body_report / _set_rest_thresholds / _body_states / _body_rest_events /
_islands / _body_summary; solver2d_amd/csrc/body_report.hip) against its numpy statement (tests/body_report_ref.py) on the oracle chain of
tests/world_chain.py, stepped in the contact and joint orders the device reports: every record, both lists, every island and the summary
equal byte for byte, every step."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import body_report_ref as ref, body_report_world, common, contact_report_ref, joint_report_ref, shape_report_ref, world_chain
from tests.body_report_world import assert_body_report_equals_reference, thresholds_of
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, refuses, step_both, upload
from tests.world_chain import _create_contacts, golden, oracle_find_pairs, oracle_world_step, rain_world

pytestmark = pytest.mark.gpu

STEPS = 12
f32 = np.float32
ALL, NO_FILTER = wire.BODY_REPORT_ALL, wire.BODY_REPORT_STATES | wire.BODY_REPORT_REST | wire.BODY_REPORT_ISLANDS


def new_totals():
    return {"rested": 0, "woke": 0, "rested_high": 0, "woke_high": 0, "islands": [], "largest": 0, "spanning": 0, "records": 0, "unmoved": 0}


def run_chain(s, params, world, thresholds, what, steps=STEPS, flags=ALL):
    ref_world = world_chain.copy_world(world)
    totals = new_totals()
    s.world_set_rest_thresholds(*thresholds)
    upload(s, world)
    state = ref.new_state(ref_world)
    for step in range(steps):
        step_both(s, params, ref_world)
        assert_body_report_equals_reference(s, state, ref_world, thresholds, params.dt, "%s step %d" % (what, step), flags, totals)
    got, _ = download(s, world)
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    assert np.isfinite(ref_world["bodies"]["position"]).all(), what
    return totals, ref_world


def rises_and_falls(counts):
    return any(b > a for a, b in zip(counts, counts[1:])) and any(b < a for a, b in zip(counts, counts[1:]))


@pytest.mark.parametrize("name", ["far_pyramid0_TGS_Soft", "far_ragdoll_pile0_PGS_Soft", "high_mass_ratio1_PGS_NGS", "mixed24_Jacobi", "circle_pile20_XPBD",
                                  "shapes_zoo40_TGS_Sticky"])
def test_golden_worlds_report_every_step(name):
    """12 steps, all flags (so the records are those of the bodies that moved; the other tests list every reported body), thresholds 0.2,
    0.2 * 3.4906585, 3 dt.  The CPU oracle chain in pool order has, as rested / woke,
    57/5, 45/11, 32/15, 7/4, 5/3 and 18/2 events on these worlds, and island counts that fall 7 -> 1 (far_pyramid0), go 12 -> 11 -> 10 ->
    11 (circle_pile20) and 15 -> 16 -> 15 -> 18 (mixed24_Jacobi); the device may sweep contacts and joints in another
    order, hence the floors."""
    params, world = golden(name)
    with hip.Solver(0) as s:
        s.world_set_body_report(ALL)
        totals, _ = run_chain(s, params, world, thresholds_of(0.2, params.dt), name, flags=ALL)
    totals.pop("last_moved")
    print(name, totals)
    assert totals["rested"] >= 3 and totals["woke"] >= 1, totals
    if name in ("circle_pile20_XPBD", "mixed24_Jacobi"):
        assert rises_and_falls(totals["islands"]), totals


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "Jacobi"])
def test_synthetic_world_crosses_the_wave_and_the_tile(solver_name):
    """640 body slots: three tiles, free slots in each, chains across a wave and a tile boundary, a chain that alternates between the tiles
    and a hub with 70 spokes.  tests/test_body_report_host.py asserts, by the reference alone on the CPU chain, that this input has the
    events; the totals are asserted here as well.  Then the same run under MOVED_ONLY: exactly the unmoved bodies are left out."""
    world = body_report_world.synthetic_world()
    body_report_world.assert_world_is_what_it_says(world)
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, float(body_report_world.DT), vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_body_report(NO_FILTER)
        totals, _ = run_chain(s, params, world, body_report_world.THRESHOLDS, "synthetic " + solver_name, flags=NO_FILTER)
        totals.pop("last_moved")
        print(solver_name, totals)
        assert totals["rested"] >= 8 and totals["woke"] >= 8, totals
        assert 1 <= totals["rested_high"] < totals["rested"] and 1 <= totals["woke_high"] < totals["woke"], totals
        assert totals["largest"] == 71 and totals["spanning"] == 2 and totals["unmoved"] >= 30 * STEPS, totals
        s.world_set_body_report(ALL)
        filtered, _ = run_chain(s, params, world, body_report_world.THRESHOLDS, "synthetic, moved only, " + solver_name, flags=ALL)
        assert filtered["unmoved"] == totals["unmoved"] and filtered["records"] == totals["records"]
        # (the last step once more by hand: the list is the reported bodies less the unmoved ones)
        states = s.world_body_states()
        summary = s.world_body_summary()
        assert len(states) == int(summary["movedBodies"]) < int(summary["bodies"]) and (states["flags"] & 1).all()
        moved = filtered.pop("last_moved")
        assert states["slot"].tolist() == np.flatnonzero(moved).tolist()
        # (most of the still bodies are among those left out: Jacobi's integration rewrites the rotation of a few of them)
        assert int((~moved[body_report_world.STILL]).sum()) >= 30


def whole_loop(s, params, world, thresholds, steps, what):
    """The whole s2World_Step loop like tests/test_gpu_contact_report.py: whole_loop, with the body report checked against the oracle chain."""
    ref_world = world_chain.copy_world(world)
    totals = new_totals()
    s.world_set_rest_thresholds(*thresholds)
    upload(s, world)
    state = ref.new_state(ref_world)
    for step in range(steps):
        if world_chain.moved_any(ref_world):
            got = s.world_find_pairs()
            want = oracle_find_pairs(ref_world)
            assert np.array_equal(got, want), "%s step %d: new pairs" % (what, step)
            if len(got):
                slots, contacts, pairs = _create_contacts(ref_world, got)
                s.world_set_contacts(slots, contacts, pairs)
        info = s.world_step(params)
        order, _ = s.contact_order()
        status = oracle_world_step(params, ref_world, contact_order=order)
        assert info["separatedCount"] == int((status == wire.PAIR_SEPARATED).sum()), "%s step %d" % (what, step)
        assert_body_report_equals_reference(s, state, ref_world, thresholds, params.dt, "%s step %d" % (what, step), NO_FILTER, totals)
        if step % 10 == 9:
            got_world, _ = download(s, world)
            world_chain.assert_device_equals_oracle(got_world, ref_world, "%s step %d" % (what, step))
    return totals


@pytest.mark.parametrize("seed,solver_name", [(1, "TGS_Soft"), (6, "Jacobi")])
def test_rain_loops_report_every_step(seed, solver_name):
    """330 bodies of every shape type rain into a trough for 70 steps: contacts are created, begin and end all the time, so islands merge
    and split and bodies come to rest and wake up.  On the CPU chain in pool order the islands go 331 -> 197 (TGS_Soft) and 331 -> 205
    (Jacobi), the largest ever has 52 / 48 bodies, the count falls on 46 / 44 steps and rises on 5 / 8, 3 / 4 islands hold bodies on both
    sides of slot 256, and rested / woke is 175/159 and 149/148, of which 26/26 and 29/29 in slots >= 256."""
    vel, pos = common.DEFAULT_ITERS[solver_name]
    dt = 1.0 / 60.0
    params = wire.StepParams.make(solver_name, dt, vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_body_report(NO_FILTER)
        totals = whole_loop(s, params, rain_world(seed, 330), thresholds_of(0.7, params.dt), 70, "rain %d %s" % (seed, solver_name))
    totals.pop("last_moved")
    print(seed, solver_name, totals)
    counts = totals["islands"]
    fell = sum(1 for a, b in zip(counts, counts[1:]) if b < a)
    rose = sum(1 for a, b in zip(counts, counts[1:]) if b > a)
    assert fell >= 20 and rose >= 2, (fell, rose, counts)
    assert totals["largest"] >= 15 and totals["spanning"] >= 1, totals
    assert totals["rested"] >= 50 and totals["woke"] >= 50 and totals["rested_high"] >= 5 and totals["woke_high"] >= 5, totals


def test_report_off_changes_nothing_and_the_getters_refuse():
    """Two solvers in lockstep, one with every body flag and one with none: the same world bytes and step counters every step; without a
    flag the getters refuse.  Then the errors: capacities, bad thresholds, unknown bits."""
    params, world = golden("mixed24_PGS")
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    thresholds = thresholds_of(0.2, params.dt)
    with hip.Solver(0) as on, hip.Solver(0) as off:
        off_getters = (off.world_body_states, off.world_body_rest_events, off.world_islands, off.world_body_summary)
        for getter in off_getters:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                getter()  # no resident world
        for bad in (16, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                on.world_set_body_report(bad)
        for bad in ((-0.5, 1.0, 1.0), (0.5, -1.0, 1.0), (0.5, 1.0, -0.25), (np.nan, 1.0, 1.0), (0.5, np.nan, 1.0), (0.5, 1.0, np.nan)):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                on.world_set_rest_thresholds(*bad)
        on.world_set_body_report(ALL)
        on.world_set_rest_thresholds(*thresholds)
        off.world_set_rest_thresholds(*thresholds)  # thresholds without a flag: nothing to enqueue
        upload(on, world), upload(off, world)
        refuses(on, E_STATE, ("world_body_states", "world_body_rest_events", "world_islands", "world_body_summary"))  # no step since the upload
        launches_compared = 0
        for step in range(STEPS):
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            sa, sb = on.stats(), off.stats()
            if (sa["structureBuilds"], sa["asyncBuildsAdopted"]) == (sb["structureBuilds"], sb["asyncBuildsAdopted"]):
                # (the two solvers adopt their worker threads' structures when those are ready: only steps on the same structure compare)
                assert sa["kernelLaunches"] == sb["kernelLaunches"] and sa["solveLaunches"] == sb["solveLaunches"], "step %d: %r / %r" % (step, sa, sb)
                launches_compared += 1
            assert int(on.world_body_summary()["bodies"]) >= 20
            on.world_body_states(), on.world_body_rest_events(), on.world_islands()
            for getter in off_getters:
                with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                    getter()
            (wa, sta), (wb, stb) = download(on, world), download(off, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert a["activeContacts"] >= 1 and launches_compared >= STEPS // 2, (a, launches_compared)


def test_capacity_errors_thresholds_off_and_on_and_a_second_upload():
    """Through the raw C calls: a buffer one entry too small gives S2AMD_E_CAPACITY with the true counts and nothing written; the same call
    with room succeeds.  Changing the thresholds between steps raises no event by itself; turning the report off and on zeroes the timers;
    a second upload resets timers and pose copy."""
    world = body_report_world.synthetic_world()
    ref_world = world_chain.copy_world(world)
    thresholds = body_report_world.THRESHOLDS
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", float(body_report_world.DT), vel, pos, True)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.world_set_body_report(NO_FILTER)
        s.world_set_rest_thresholds(*thresholds)
        upload(s, world)
        state = ref.new_state(ref_world)
        for n in range(4):  # after step 4 the bodies that started at rest wake up, while the still ones came to rest in step 3
            step_both(s, params, ref_world)
            step = assert_body_report_equals_reference(s, state, ref_world, thresholds, params.dt, "step %d" % n, NO_FILTER)
        want_rested, want_woke = ref.events(step)
        nr_want, nw_want = len(want_rested), len(want_woke)
        assert nw_want >= 8
        nr, nw = ctypes.c_int32(-7), ctypes.c_int32(-7)
        rested, woke = np.full(max(nr_want, 1), -1, dtype=np.int32), np.full(nw_want, -1, dtype=np.int32)
        rc = L.s2amd_world_body_rest_events(h, wire.as_ptr(rested), nr_want, ctypes.byref(nr), wire.as_ptr(woke), nw_want - 1, ctypes.byref(nw))
        assert (rc, nr.value, nw.value) == (E_CAPACITY, nr_want, nw_want) and (rested == -1).all() and (woke == -1).all()
        rc = L.s2amd_world_body_rest_events(h, wire.as_ptr(rested), nr_want, ctypes.byref(nr), wire.as_ptr(woke), nw_want, ctypes.byref(nw))
        assert (rc, nr.value, nw.value) == (0, nr_want, nw_want)
        assert rested[:nr_want].tolist() == want_rested.tolist() and woke.tolist() == want_woke.tolist()
        island, island_states = ref.islands(ref_world, step)
        for fn, want, dtype in ((L.s2amd_world_body_states, ref.states(ref_world, step, False, island, island_states), wire.body_state_dtype),
                                (L.s2amd_world_islands, island_states, wire.island_state_dtype)):
            n = len(want)
            assert n >= 65
            out = np.zeros(n, dtype=dtype)
            count = ctypes.c_int32(-7)
            rc = fn(h, wire.as_ptr(out), n - 1, ctypes.byref(count))
            assert (rc, count.value) == (E_CAPACITY, n) and out.tobytes() == bytes(n * dtype.itemsize)
            rc = fn(h, wire.as_ptr(out), n, ctypes.byref(count))
            assert (rc, count.value) == (0, n) and out.tobytes() == want.tobytes()
        # the Python getters, asked afterwards, see the same step
        r2, w2 = s.world_body_rest_events(expected=1)
        assert r2.tolist() == want_rested.tolist() and w2.tolist() == want_woke.tolist()

        # thresholds changed between steps.  `seconds` raised to 5 dt: the still bodies (timers at 4 dt) are not at rest before the next step
        # any more and reach 5 dt in it -- they are its `rested`
        tight = (thresholds[0], thresholds[1], f32(5) * f32(params.dt))
        s.world_set_rest_thresholds(*tight)
        step_both(s, params, ref_world)
        step = assert_body_report_equals_reference(s, state, ref_world, tight, params.dt, "after raising `seconds`", NO_FILTER)
        assert set(body_report_world.STILL) <= set(ref.events(step)[0].tolist())
        # ... lowered to dt: the damped bodies whose timers stand between dt and 5 dt are at rest from here on, by the caller's own act.  A
        # report that kept its old at-rest bits would list them as `rested` in the next step; only what the step changes is an event
        loose = (thresholds[0], thresholds[1], f32(params.dt))
        between = np.flatnonzero(step["reported"] & (state["timer"] >= loose[2]) & ~step["now"])
        assert len(between) >= 5, between
        s.world_set_rest_thresholds(*loose)
        step_both(s, params, ref_world)
        step = assert_body_report_equals_reference(s, state, ref_world, loose, params.dt, "after lowering `seconds`", NO_FILTER)
        assert step["now"][between].all() and not set(between.tolist()) & set(ref.events(step)[0].tolist())
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_rest_thresholds(np.nan, 1.0, 1.0)  # the ones that hold stay
        step_both(s, params, ref_world)
        assert_body_report_equals_reference(s, state, ref_world, loose, params.dt, "after refused thresholds", NO_FILTER)

        # off and on: the timers start at +0 again and the pose copy is of the bodies as they stand
        assert int((state["timer"] > 0).sum()) >= 30
        s.world_set_body_report(0)
        step_both(s, params, ref_world)  # advances nothing
        refuses(s, E_STATE, ("world_body_summary", "world_body_states"))
        s.world_set_body_report(wire.BODY_REPORT_REST)
        state = ref.new_state(ref_world)
        step_both(s, params, ref_world)
        step = assert_body_report_equals_reference(s, state, ref_world, loose, params.dt, "off and on", wire.BODY_REPORT_REST)
        assert len(ref.events(step)[0]) >= 30  # (everything still or slow has a timer of dt again: rested under `seconds` = dt)
        refuses(s, E_STATE, ("world_body_states", "world_islands"))  # not this step's flags

        # a second upload with other capacities: 42 body slots instead of 640; flags and thresholds hold across it
        params2, world2 = golden("mixed24_PGS")
        ref_world2 = world_chain.copy_world(world2)
        s.world_set_body_report(NO_FILTER)
        upload(s, world2)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_body_summary()  # no step since the upload
        state2 = ref.new_state(ref_world2)
        step_both(s, params2, ref_world2)
        assert_body_report_equals_reference(s, state2, ref_world2, loose, params2.dt, "the step after the second upload", NO_FILTER)
        # ... and back to the larger one
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        state = ref.new_state(ref_world)
        step_both(s, params, ref_world)
        step = assert_body_report_equals_reference(s, state, ref_world, loose, params.dt, "the step after the third upload", NO_FILTER)
        assert int(step["moved"].sum()) >= 100 and int((step["reported"] & ~step["moved"]).sum()) >= 30


def test_all_four_reports_on_at_once():
    """The contact, the joint, the shape and the body report together on a world with contacts, joints and a kinematic body: each equals
    its own statement in the same steps."""
    params, world = golden("mixed24_PGS")
    ref_world = world_chain.copy_world(world)
    thresholds = thresholds_of(0.2, params.dt)
    touching_seen = 0
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_body_report(NO_FILTER)
        s.world_set_rest_thresholds(*thresholds)
        upload(s, world)
        prev_touch = contact_report_ref.before_of(ref_world["contacts"])
        prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
        prev_view = shape_report_ref.in_view(ref_world, None)
        state = ref.new_state(ref_world)
        for step in range(STEPS):
            step_both(s, params, ref_world)
            what = "mixed24 step %d" % step
            assert_body_report_equals_reference(s, state, ref_world, thresholds, params.dt, what, NO_FILTER)
            assert s.world_shape_draws(expected=64).tobytes() == shape_report_ref.draws(ref_world, None).tobytes(), what
            want_entered, want_left = shape_report_ref.events(prev_view, ref_world, None)
            entered, left = s.world_shape_view_events()
            assert entered.tolist() == want_entered.tolist() and left.tolist() == want_left.tolist(), what
            assert s.world_shape_summary().tobytes() == shape_report_ref.summary(ref_world, None).tobytes(), what
            want_began, want_ended = contact_report_ref.events(prev_touch, ref_world)
            began, ended = s.world_touch_events()
            assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
            want_touching = contact_report_ref.touching(ref_world)
            touching_seen = max(touching_seen, len(want_touching))
            assert s.world_touching(expected=max(len(want_touching), 1)).tobytes() == want_touching.tobytes(), what
            assert s.world_body_sums().tobytes() == contact_report_ref.body_sums(ref_world).tobytes(), what
            want_states = joint_report_ref.states(ref_world)
            assert s.world_joint_states(expected=max(len(want_states), 1)).tobytes() == want_states.tobytes(), what
            want_began, want_ended = joint_report_ref.events(prev_limits, ref_world)
            began, ended = s.world_joint_limit_events()
            assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
            assert s.world_body_joint_sums().tobytes() == joint_report_ref.body_sums(ref_world).tobytes(), what
            assert s.world_joint_summary().tobytes() == joint_report_ref.summary(ref_world).tobytes(), what
            prev_touch = contact_report_ref.touching_mask(ref_world)
            prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
            prev_view = shape_report_ref.in_view(ref_world, None)
    assert touching_seen >= 1
