"""The shape report of the resident world (s2amd_world_set_shape_report / _set_shape_view / _shape_draws / _shape_view_events /
_shape_summary; solver2d_amd/csrc/shape_report.hip) against its numpy statement (tests/shape_report_ref.py) on the oracle chain of
tests/world_chain.py, stepped in the contact and joint orders the device reports: every record, both lists and the summary equal byte
for byte, every step."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import common, contact_report_ref, joint_report_ref, shape_report_ref as ref, shape_report_world, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, refuses, step_both, upload
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

STEPS = 12
f32 = np.float32


def middle_third(world):
    """The middle third of the movable bounds as the world stands"""
    lx, ly, ux, uy = ref.summary(world, None)["movableBounds"]
    w, h = f32(ux - lx), f32(uy - ly)
    return (f32(lx + w / f32(3)), f32(ly + h / f32(3)), f32(ux - w / f32(3)), f32(uy - h / f32(3)))


def new_totals():
    return {"entered": 0, "left": 0, "low": 0, "high": 0, "both": 0, "records": 0}


def assert_shape_report_equals_reference(s, prev_mask, world, view, what, totals=None):
    """The three getters against the reference statement on `world` (the oracle chain after the step) and the in-view state before it."""
    want = ref.draws(world, view)
    got = s.world_shape_draws(expected=max(len(want), 1))
    assert len(got) == len(want), "%s: %d draw records, reference %d" % (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: draw records differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))
    want_entered, want_left = ref.events(prev_mask, world, view)
    entered, left = s.world_shape_view_events()
    assert entered.tolist() == want_entered.tolist(), what + ": entered"
    assert left.tolist() == want_left.tolist(), what + ": left"
    want_summary = ref.summary(world, view)
    summary = s.world_shape_summary()
    assert summary.tobytes() == want_summary.tobytes(), "%s: summary %s, reference %s" % (what, summary, want_summary)
    if totals is not None:
        events = np.concatenate([entered, left])
        totals["entered"] += len(entered)
        totals["left"] += len(left)
        totals["low"] += int((events < 256).sum())
        totals["high"] += int((events >= 256).sum())
        totals["both"] += 1 if len(entered) and len(left) else 0
        totals["records"] += len(got)


def run_chain(s, params, world, view, what, steps=STEPS):
    ref_world = world_chain.copy_world(world)
    totals = new_totals()
    s.world_set_shape_view(view)
    upload(s, world)
    prev = ref.in_view(ref_world, view)
    for step in range(steps):
        step_both(s, params, ref_world)
        assert_shape_report_equals_reference(s, prev, ref_world, view, "%s step %d" % (what, step), totals)
        prev = ref.in_view(ref_world, view)
    got, _ = download(s, world)
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    assert np.isfinite(ref_world["bodies"]["position"]).all(), what
    return totals, ref_world


ZOO = (54, 63, [9, 16, 24, 5])


@pytest.mark.parametrize("with_view", [False, True])
@pytest.mark.parametrize("name,census", [("shapes_zoo40_TGS_Sticky", ZOO), ("shapes_zoo40_PGS_NGS_Block", ZOO), ("mixed24_PGS", (37, 42, [14, 6, 17, 0])),
                                         ("far_pyramid0_TGS_Soft", (56, 63, [0, 0, 56, 0]))])
def test_golden_worlds_report_every_step(name, census, with_view):
    params, world = golden(name)
    shapes, bodies = world["shapes"], world["bodies"]
    live = shapes["type"] != wire.SHAPE_FREE
    # the input is what the test says it is
    assert (int(live.sum()), len(shapes), [int((live & (shapes["type"] == t)).sum()) for t in range(4)]) == census
    body_type = bodies["type"][np.where(live, shapes["body"], 0)]
    if name.startswith("shapes_zoo40"):
        polygons = live & (shapes["type"] == wire.SHAPE_POLYGON)
        assert sorted(set(shapes["count"][polygons].tolist())) == [3, 4, 5, 6, 7, 8]
        assert int((polygons & (shapes["radius"] > 0)).sum()) == 8 and int((live & (body_type == wire.BODY_STATIC)).sum()) == 6
    if name == "mixed24_PGS":
        assert int((live & (body_type == wire.BODY_KINEMATIC)).sum()) >= 1
    if name.startswith("far_pyramid0"):
        assert float(np.abs(world["origins"]).max()) > 5e4
    view = middle_third(world) if with_view else None
    if with_view:
        inside = int(ref.in_view(world, view).sum())
        assert 0 < inside < int(live.sum()), inside
    with hip.Solver(0) as s:
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        totals, _ = run_chain(s, params, world, view, name)
    print(name, with_view, totals)
    assert totals["records"] >= STEPS


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "Jacobi"])
def test_synthetic_world_crosses_the_wave_and_the_tile(solver_name):
    """331 shape slots: two tiles, free slots in both, shapes crossing the lower, upper and side edges of the view all through the 12
    steps.  tests/test_shape_report_host.py asserts, by the reference alone on the CPU chain, that this input has the events; free-falling
    bodies without contacts move alike under every solver, and the totals are asserted here as well."""
    world = shape_report_world.synthetic_world()
    shape_report_world.assert_world_is_what_it_says(world)
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        totals, ref_world = run_chain(s, params, world, shape_report_world.VIEW, "synthetic " + solver_name)
    print(solver_name, totals)
    assert totals["entered"] >= 8 and totals["left"] >= 8 and totals["low"] >= 1 and totals["high"] >= 1 and totals["both"] >= 1, totals
    now = ref.in_view(ref_world, shape_report_world.VIEW)
    assert any(int(now[t:t + 256].sum()) % 64 != 0 for t in (0, 256))


def test_changing_the_view_between_steps():
    """A change of view raises no events; the next step's events are relative to the new view; without a view every live shape is
    reported and nothing enters or leaves any more."""
    world = shape_report_world.synthetic_world()
    ref_world = world_chain.copy_world(world)
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)
    first, second = shape_report_world.VIEW, (-3.0, 0.25, 3.0, 7.5)
    live = int((world["shapes"]["type"] != wire.SHAPE_FREE).sum())
    with hip.Solver(0) as s:
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_shape_view(first)
        upload(s, world)
        prev = ref.in_view(ref_world, first)
        for step in range(3):
            step_both(s, params, ref_world)
            assert_shape_report_equals_reference(s, prev, ref_world, first, "first view, step %d" % step)
            prev = ref.in_view(ref_world, first)
        # the change itself: the last step's report still stands as it was, and "before" is now taken under the second view
        s.world_set_shape_view(second)
        changed = ref.in_view(ref_world, second) != prev
        assert int(changed.sum()) >= 20  # (what a report that kept the old "before" would list as events)
        prev = ref.in_view(ref_world, second)
        events_seen = 0
        for step in range(3):
            step_both(s, params, ref_world)
            assert_shape_report_equals_reference(s, prev, ref_world, second, "second view, step %d" % step)
            entered, left = s.world_shape_view_events()
            events_seen += len(entered) + len(left)
            assert len(entered) + len(left) < int(changed.sum())
            prev = ref.in_view(ref_world, second)
        assert events_seen >= 3  # (the CPU chain in pool order: about 15 shapes leave the second view in each of these steps)
        # cleared: everything live is in view from here on
        s.world_set_shape_view(None)
        prev = ref.in_view(ref_world, None)
        for step in range(2):
            step_both(s, params, ref_world)
            assert_shape_report_equals_reference(s, prev, ref_world, None, "no view, step %d" % step)
            entered, left = s.world_shape_view_events()
            assert len(entered) == 0 and len(left) == 0 and len(s.world_shape_draws()) == live
            assert int(s.world_shape_summary()["inView"]) == live
        got, _ = download(s, world)
        world_chain.assert_device_equals_oracle(got, ref_world, "after three views")


def test_report_off_changes_nothing_and_the_getters_refuse():
    """Two solvers in lockstep on the shape zoo, one with every shape flag and a view and one with none: the same world bytes, step
    counters, stage-3 status and kernel launches of the solve every step; without a flag the getters refuse."""
    params, world = golden("shapes_zoo40_TGS_Sticky")
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    with hip.Solver(0) as on, hip.Solver(0) as off:
        off_getters = (off.world_shape_draws, off.world_shape_view_events, off.world_shape_summary)
        for getter in off_getters:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                getter()  # no resident world
        on.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        on.world_set_shape_view(middle_third(world))
        off.world_set_shape_view(middle_third(world))  # a view without a flag: nothing to enqueue
        upload(on, world), upload(off, world)
        launches_compared = 0
        for step in range(STEPS):
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            sa, sb = on.stats(), off.stats()
            if (sa["structureBuilds"], sa["asyncBuildsAdopted"]) == (sb["structureBuilds"], sb["asyncBuildsAdopted"]):
                # (the two solvers adopt their worker threads' structures when those are ready: only steps on the same structure compare)
                assert sa["kernelLaunches"] == sb["kernelLaunches"] and sa["solveLaunches"] == sb["solveLaunches"], "step %d: %r / %r" % (step, sa, sb)
                launches_compared += 1
            assert 1 <= len(on.world_shape_draws()) < 54
            on.world_shape_view_events(), on.world_shape_summary()
            for getter in off_getters:
                with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                    getter()
            (wa, sta), (wb, stb) = download(on, world), download(off, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert a["activeContacts"] >= 1 and launches_compared >= STEPS // 2, (a, launches_compared)


def test_all_three_reports_on_at_once():
    """The contact, the joint and the shape report together on a world with contacts, joints and a kinematic body: each equals its own
    statement."""
    params, world = golden("mixed24_PGS")
    ref_world = world_chain.copy_world(world)
    view = middle_third(world)
    touching_seen = 0
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_shape_view(view)
        upload(s, world)
        prev_touch = contact_report_ref.before_of(ref_world["contacts"])
        prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
        prev_view = ref.in_view(ref_world, view)
        for step in range(STEPS):
            step_both(s, params, ref_world)
            what = "mixed24 step %d" % step
            assert_shape_report_equals_reference(s, prev_view, ref_world, view, what)
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
            prev_view = ref.in_view(ref_world, view)
    assert touching_seen >= 1


def test_flag_subsets_unknown_bits_bad_views_and_timing():
    world = shape_report_world.synthetic_world()
    ref_world = world_chain.copy_world(world)
    view = shape_report_world.VIEW
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        for bad in (8, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_shape_report(bad)
        for bad in ((1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0), (np.nan, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, np.nan)):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_shape_view(bad)
        s.world_set_shape_view(view)
        s.world_set_shape_report(wire.SHAPE_REPORT_VIEW)
        upload(s, world)
        refuses(s, E_STATE, ("world_shape_view_events", "world_shape_summary", "world_shape_draws"))  # no step has run since the flag was set
        prev = ref.in_view(ref_world, view)
        step_both(s, params, ref_world)
        want_entered, want_left = ref.events(prev, ref_world, view)
        entered, left = s.world_shape_view_events()
        assert entered.tolist() == want_entered.tolist() and left.tolist() == want_left.tolist()
        assert s.world_shape_summary().tobytes() == ref.summary(ref_world, view).tobytes()  # any flag will do
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_shape_draws()
        # a flag set between two steps takes effect from the next step
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_shape_draws()
        prev = ref.in_view(ref_world, view)
        step_both(s, params, ref_world)
        assert_shape_report_equals_reference(s, prev, ref_world, view, "all flags from the second step")
        # ... and one cleared as well; the in-view state keeps advancing while nobody asks for the lists
        s.world_set_shape_report(wire.SHAPE_REPORT_BOUNDS)
        for _ in range(3):
            step_both(s, params, ref_world)
        assert s.world_shape_summary().tobytes() == ref.summary(ref_world, view).tobytes()
        refuses(s, E_STATE, ("world_shape_draws", "world_shape_view_events"))
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        prev = ref.in_view(ref_world, view)
        step_both(s, params, ref_world)
        assert_shape_report_equals_reference(s, prev, ref_world, view, "after steps without the view flag")
        # a bad view leaves the one that holds
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_shape_view((np.nan, 0.0, 1.0, 1.0))
        prev = ref.in_view(ref_world, view)
        step_both(s, params, ref_world)
        assert_shape_report_equals_reference(s, prev, ref_world, view, "after a refused view")


def test_capacity_errors_and_a_second_upload():
    """Through the raw C calls: a buffer one entry too small gives S2AMD_E_CAPACITY with the true counts and nothing written; the same
    call with room succeeds.  Then another world with other capacities uploaded into the same solver: "before" is taken from the
    uploaded shapes, so the next step's `entered` is not the whole in-view set."""
    world = shape_report_world.synthetic_world()
    ref_world = world_chain.copy_world(world)
    view = shape_report_world.VIEW
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_shape_view(view)
        upload(s, world)
        prev = ref.in_view(ref_world, view)
        want_entered = want_left = np.zeros(0, dtype=np.int32)
        for _ in range(STEPS):  # up to a step with events of both kinds (tests/test_shape_report_host.py: the CPU chain has one)
            step_both(s, params, ref_world)
            want_entered, want_left = ref.events(prev, ref_world, view)
            if len(want_entered) and len(want_left):
                break
            prev = ref.in_view(ref_world, view)
        ne_want, nl_want = len(want_entered), len(want_left)
        assert ne_want >= 1 and nl_want >= 1
        ne, nl = ctypes.c_int32(-7), ctypes.c_int32(-7)
        entered, left = np.full(ne_want, -1, dtype=np.int32), np.full(nl_want, -1, dtype=np.int32)
        rc = L.s2amd_world_shape_view_events(h, wire.as_ptr(entered), ne_want - 1, ctypes.byref(ne), wire.as_ptr(left), nl_want, ctypes.byref(nl))
        assert (rc, ne.value, nl.value) == (E_CAPACITY, ne_want, nl_want) and (entered == -1).all() and (left == -1).all()
        rc = L.s2amd_world_shape_view_events(h, wire.as_ptr(entered), ne_want, ctypes.byref(ne), wire.as_ptr(left), nl_want - 1, ctypes.byref(nl))
        assert (rc, ne.value, nl.value) == (E_CAPACITY, ne_want, nl_want) and (entered == -1).all() and (left == -1).all()
        rc = L.s2amd_world_shape_view_events(h, wire.as_ptr(entered), ne_want, ctypes.byref(ne), wire.as_ptr(left), nl_want, ctypes.byref(nl))
        assert (rc, ne.value, nl.value) == (0, ne_want, nl_want)
        assert entered.tolist() == want_entered.tolist() and left.tolist() == want_left.tolist()
        want = ref.draws(ref_world, view)
        n = len(want)
        assert n >= 65
        out = np.zeros(n, dtype=wire.shape_draw_dtype)
        count = ctypes.c_int32(-7)
        rc = L.s2amd_world_shape_draws(h, wire.as_ptr(out), n - 1, ctypes.byref(count))
        assert (rc, count.value) == (E_CAPACITY, n) and out.tobytes() == bytes(n * 128)
        rc = L.s2amd_world_shape_draws(h, wire.as_ptr(out), n, ctypes.byref(count))
        assert (rc, count.value) == (0, n) and out.tobytes() == want.tobytes()
        # the Python getters, asked afterwards, see the same step
        e2, l2 = s.world_shape_view_events(expected=1)
        assert e2.tolist() == want_entered.tolist() and l2.tolist() == want_left.tolist()
        assert s.world_shape_draws(expected=1).tobytes() == want.tobytes()

        # a second upload with other capacities: the shape zoo, 63 shape slots instead of 331; flags and view hold across it
        params2, world2 = golden("shapes_zoo40_TGS_Sticky")
        ref_world2 = world_chain.copy_world(world2)
        upload(s, world2)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_shape_view_events()  # no step since the upload
        prev = ref.in_view(ref_world2, view)
        assert int(prev.sum()) >= 2
        step_both(s, params2, ref_world2)
        assert_shape_report_equals_reference(s, prev, ref_world2, view, "the step after the second upload")
        entered, _ = s.world_shape_view_events()
        assert len(entered) < int(ref.in_view(ref_world2, view).sum())
        # ... and back to the larger one
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        prev = ref.in_view(ref_world, view)
        step_both(s, params, ref_world)
        assert_shape_report_equals_reference(s, prev, ref_world, view, "the step after the third upload")
