"""The sensor report of the resident world (s2amd_world_set_sensors / _set_sensor_report / _sensor_inside / _sensor_events /
_sensor_states; solver2d_amd/csrc/sensor_report.hip) against its statement (tests/sensor_report_ref.py), byte for byte: the recorded
lists of tests/golden/sensor_report on the oracle chain of tests/world_chain.py stepped in the device's orders, the statement itself
where the reference library is built, and the device's own s2amd_world_shapes_in_range under the composed transform."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import sensor_report_ref as ref, sensor_report_world as sw, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, downloaded_world, refuses, step_both, upload

pytestmark = pytest.mark.gpu

ALL = wire.SENSOR_REPORT_ALL


def device_lists(s, world, sensors):
    """What s2amd_world_shapes_in_range answers for every active sensor's proxy under its composed transform with maxDistance = margin,
    asked of the resident world as it stands, minus the shapes the sensor's rule excludes (its own body's, static ones under
    SKIP_STATIC).  `world` is the oracle chain's copy of the resident world (body types, shape bodies, the poses to compose with)."""
    active = [i for i, q in enumerate(sensors) if ref.is_active(world, q)]
    lists = [[] for _ in sensors]
    if not active:
        return lists
    queries = np.array([ref.as_query(world, sensors[i]) for i in active], dtype=wire.proximity_query_dtype)
    offsets, shapes = s.world_shapes_in_range(queries)
    body_of, static = world["shapes"]["body"], world["bodies"]["type"] == wire.BODY_STATIC
    for j, i in enumerate(active):
        q = sensors[i]
        skip = bool(int(q["flags"]) & wire.SENSOR_SKIP_STATIC)
        lists[i] = [int(x) for x in shapes[offsets[j]:offsets[j + 1]] if body_of[x] != q["body"] and not (skip and static[body_of[x]])]
    return lists


def c_getters(s, count):
    """The three getters through the raw C calls with buffers of exactly the stated sizes: asked with capacity 0 first, which must
    state the counts and touch nothing."""
    L, h = s._L, s._h
    offsets, total = np.full(count + 1, -1, dtype=np.int32), ctypes.c_int32(-7)
    rc = L.s2amd_world_sensor_inside(h, wire.as_ptr(offsets), None, 0, ctypes.byref(total))
    assert rc == (E_CAPACITY if total.value > 0 else 0) and total.value == offsets[count], (rc, total.value, offsets)
    shapes = np.full(total.value, -1, dtype=np.int32)
    rc = L.s2amd_world_sensor_inside(h, wire.as_ptr(offsets), wire.as_ptr(shapes) if total.value else None, total.value, ctypes.byref(total))
    assert rc == 0, rc
    ne, nl = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = L.s2amd_world_sensor_events(h, None, 0, ctypes.byref(ne), None, 0, ctypes.byref(nl))
    assert rc == (E_CAPACITY if ne.value + nl.value > 0 else 0), rc
    entered, left = np.zeros(ne.value, dtype=wire.sensor_event_dtype), np.zeros(nl.value, dtype=wire.sensor_event_dtype)
    if ne.value > 0:
        # one entry too few on one side: both counts stated, neither list touched
        entered.view(np.uint8)[:] = 0xFF
        left.view(np.uint8)[:] = 0xFF
        rc = L.s2amd_world_sensor_events(h, wire.as_ptr(entered), ne.value - 1, ctypes.byref(ne), wire.as_ptr(left) if nl.value else None, nl.value, ctypes.byref(nl))
        assert (rc, ne.value, nl.value) == (E_CAPACITY, len(entered), len(left)), rc
        assert (entered.view(np.uint8) == 0xFF).all() and (left.view(np.uint8) == 0xFF).all()
    rc = L.s2amd_world_sensor_events(h, wire.as_ptr(entered) if ne.value else None, ne.value, ctypes.byref(ne), wire.as_ptr(left) if nl.value else None, nl.value,
                                     ctypes.byref(nl))
    assert rc == 0 and (ne.value, nl.value) == (len(entered), len(left)), rc
    n = ctypes.c_int32(-7)
    states = np.zeros(count, dtype=wire.sensor_state_dtype)
    if count > 0:
        rc = L.s2amd_world_sensor_states(h, wire.as_ptr(states), count - 1, ctypes.byref(n))
        assert (rc, n.value) == (E_CAPACITY, count) and states.tobytes() == bytes(64 * count)
    rc = L.s2amd_world_sensor_states(h, wire.as_ptr(states) if count else None, count, ctypes.byref(n))
    assert (rc, n.value) == (0, count)
    return offsets, shapes, entered, left, states


def assert_report(s, world, sensors, before, now, what, raw=True):
    """Every getter, through hip.py and through the C calls, against the statement's bytes for the lists `before` and `now`"""
    want_offsets, want_shapes = ref.csr(now)
    want_entered, want_left = ref.events(before, now, world, sensors)
    want_states = ref.states(world, sensors, before, now)
    got = [(s.world_sensor_inside() + s.world_sensor_events() + (s.world_sensor_states(),))]
    if raw:
        got.append(c_getters(s, len(sensors)))
    for offsets, shapes, entered, left, states in got:
        assert offsets.tolist() == want_offsets.tolist() and shapes.tolist() == want_shapes.tolist(), "%s: inside %s %s, statement %s %s" % (
            what, offsets.tolist(), shapes.tolist(), want_offsets.tolist(), want_shapes.tolist())
        assert entered.tobytes() == want_entered.tobytes(), "%s: entered %s, statement %s" % (what, entered, want_entered)
        assert left.tobytes() == want_left.tobytes(), "%s: left %s, statement %s" % (what, left, want_left)
        if states.tobytes() != want_states.tobytes():
            bad = [n for n in states.dtype.names if states[n].tobytes() != want_states[n].tobytes()]
            rows = np.flatnonzero([states[i].tobytes() != want_states[i].tobytes() for i in range(len(states))])
            raise AssertionError("%s: states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), states[rows[:2]], want_states[rows[:2]]))


def apply_events(lists, entered, left):
    out = [set(x) for x in lists]
    for e in left:
        out[int(e["sensor"])].remove(int(e["shape"]))
    for e in entered:
        assert int(e["shape"]) not in out[int(e["sensor"])]
        out[int(e["sensor"])].add(int(e["shape"]))
    return [sorted(x) for x in out]


@pytest.mark.parametrize("scene,fast,list_capacity", [(scene, False, cap) for scene in sw.SCENES for cap in (0, 1, 4096)] + [(scene, True, 64) for scene in sw.SCENES])
def test_recorded_scenes_every_step(scene, fast, list_capacity):
    """The three scenes of tests/golden/sensor_report for 12 steps, in libs2amd.so with listCapacity 0 (every list rebuilt by its
    getter), 1 and ample, and in libs2amd_fast.so: the recorded lists, the states on the chain in the device's orders, the statement
    itself where the reference is built, s2amd_world_shapes_in_range asked after the same step, and the events summed over the steps."""
    fx = sw.load_fixture(scene)
    world, sensors, params = sw.fixture_world(fx), fx["sensors"], sw.params()
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0, fast=fast) as s:
        s.world_set_sensors(sensors)
        s.world_set_sensor_report(ALL, list_capacity)
        upload(s, world)
        before = sw.fixture_lists(fx, "before")
        assert device_lists(s, ref_world, sensors) == before
        summed = before
        for k in range(sw.STEPS):
            step_both(s, params, ref_world)
            now = sw.fixture_lists(fx, "inside", k)
            what = "%s step %d" % (scene, k)
            if not fast:
                # (the tolerance mode's poses are not the oracle chain's; its lists are, under the fixtures' clearance)
                assert_report(s, ref_world, sensors, before, now, what)
                assert device_lists(s, ref_world, sensors) == now, what
                if ref.available():
                    assert ref.inside_lists(ref_world, sensors) == now, what
            offsets, shapes = s.world_sensor_inside()
            entered, left = s.world_sensor_events()
            states = s.world_sensor_states()
            assert ref.from_csr(offsets, shapes) == now, what
            want_entered, want_left = ref.events(before, now, ref_world, sensors)
            assert entered.tobytes() == want_entered.tobytes() and left.tobytes() == want_left.tobytes(), what
            for name in ("sensor", "body", "active", "inside", "entered", "left", "lowestShape", "pad"):
                assert states[name].tobytes() == fx["states_%d" % k][name].tobytes(), "%s: %s" % (what, name)
            summed = apply_events(summed, entered, left)
            before = now
        assert summed == before
        if not fast:
            world_chain.assert_device_equals_oracle(downloaded_world(s, world), ref_world, scene)


def run_sweep(slots, count, steps=2, list_capacity=256):
    world = sw.sweep_world(slots)
    sensors = sw.sweep_sensors(world, count)
    ref_world, params = world_chain.copy_world(world), sw.params()
    seen = {"entered": 0, "left": 0, "inside": 0}
    with hip.Solver(0) as s:
        s.world_set_sensor_report(ALL, list_capacity)
        s.world_set_sensors(sensors)
        upload(s, world)
        before = device_lists(s, ref_world, sensors)
        if ref.available():
            assert ref.inside_lists(ref_world, sensors[:7]) == before[:7]
        for k in range(steps):
            step_both(s, params, ref_world)
            now = device_lists(s, ref_world, sensors)
            what = "%d slots, %d sensors, step %d" % (slots, count, k)
            assert_report(s, ref_world, sensors, before, now, what, raw=k == 0)
            if ref.available():
                assert ref.inside_lists(ref_world, sensors[:7]) == now[:7], what
            seen["entered"] += sum(len(set(n) - set(b)) for b, n in zip(before, now))
            seen["left"] += sum(len(set(b) - set(n)) for b, n in zip(before, now))
            seen["inside"] += sum(len(n) for n in now)
            before = now
        world_chain.assert_device_equals_oracle(downloaded_world(s, world), ref_world, "%d slots" % slots)
    return seen, before


@pytest.mark.parametrize("slots", [63, 64, 65, 255, 256, 257, 513])
def test_shape_capacities_at_the_wave_and_tile_edges(slots):
    """Seven sensors over worlds whose last shape slot is the last lane of a wave or tile, the first of the next, or one short; free
    slots among them.  The tall sensor holds shapes in every wave of every tile."""
    seen, last = run_sweep(slots, 7)
    assert seen["entered"] >= 1 and seen["left"] >= 1, seen
    tall = last[0]
    # (at 65, 257 and 513 slots the last wave, and at 257 and 513 the last tile, is the one slot of lattice column 0, outside the sensor)
    lone = slots % 64 == 1
    waves, tiles = {x // 64 for x in tall}, {x // 256 for x in tall}
    assert waves == set(range(slots // 64 if lone else (slots + 63) // 64)), (slots, sorted(waves))
    assert tiles == set(range(max(1, slots // 256) if lone else (slots + 255) // 256)), (slots, sorted(tiles))
    if slots == 513:
        assert {0, 1} <= tiles and {3, 4} <= waves  # one sensor with shapes on both sides of a tile edge and of a wave edge
    assert last[2] and last[4] == [] and last[5] == [] and last[6] == []  # the carried one holds neighbours; disabled, free body, masked out


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 1024])
def test_sensor_counts_at_the_chunk_edges(count):
    """257 shape slots (two tiles, the second with one slot) under 0, 1, one chunk less one, one chunk, one more, and the most sensors
    a list takes; listCapacity 256 is too small from 255 sensors on, so the getters rebuild their lists there."""
    seen, last = run_sweep(257, count, steps=2 if count < 1024 else 1)
    if count >= 255:
        assert seen["inside"] > 256
    if count == 0:
        assert seen == {"entered": 0, "left": 0, "inside": 0}


def test_lifecycle_set_sensors_uploads_flags_and_errors():
    fx = sw.load_fixture("chain")
    world, sensors, params = sw.fixture_world(fx), fx["sensors"], sw.params()
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        total, offsets = ctypes.c_int32(-7), np.full(8, -1, dtype=np.int32)
        # no resident world
        assert L.s2amd_world_sensor_inside(h, wire.as_ptr(offsets), None, 0, ctypes.byref(total)) == E_STATE and total.value == -7 and (offsets == -1).all()
        for bad in (8, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_sensor_report(bad)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_sensor_report(ALL, -1)
        s.world_set_sensors(sensors)
        for field, value in (("count", 0), ("count", 9), ("radius", -1.0), ("margin", -0.5), ("margin", np.inf), ("flags", 4), ("position", (np.nan, 0.0))):
            wrong = sensors.copy()
            wrong[1][field] = value
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_sensors(wrong)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_sensors(np.zeros(wire.MAX_SENSORS + 1, dtype=wire.sensor_dtype))
        s.world_set_sensor_report(wire.SENSOR_REPORT_EVENTS)
        upload(s, world)
        wrong = sensors.copy()
        wrong[0]["body"] = len(world["bodies"])
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_sensors(wrong)  # a body outside the resident world: refused, the old list stands
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_sensor_events()  # no step since the upload
        before = device_lists(s, ref_world, sensors)
        step_both(s, params, ref_world)
        now = device_lists(s, ref_world, sensors)
        want_entered, want_left = ref.events(before, now, ref_world, sensors)
        entered, left = s.world_sensor_events()
        assert entered.tobytes() == want_entered.tobytes() and left.tobytes() == want_left.tobytes()
        refuses(s, E_STATE, ("world_sensor_inside", "world_sensor_states"))  # their flags were not set before the step
        s.world_set_sensor_report(ALL)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_sensor_inside()  # a flag set between two steps takes effect from the next step
        before = now
        for k in range(4):
            step_both(s, params, ref_world)
            now = device_lists(s, ref_world, sensors)
            assert_report(s, ref_world, sensors, before, now, "all flags, step %d" % k, raw=k == 3)
            before = now
        assert sum(len(x) for x in now) >= 2
        # a buffer one entry too small: the counts stated, nothing written
        want_entered, want_left = ref.events(sw.fixture_lists(fx, "before"), now, ref_world, sensors)  # (only for its size)
        n_inside = sum(len(x) for x in now)
        shapes = np.full(n_inside, -1, dtype=np.int32)
        rc = L.s2amd_world_sensor_inside(h, wire.as_ptr(offsets), wire.as_ptr(shapes), n_inside - 1, ctypes.byref(total))
        assert (rc, total.value) == (E_CAPACITY, n_inside) and (shapes == -1).all() and offsets[:len(sensors) + 1].tolist() == ref.csr(now)[0].tolist()
        # listCapacity changed after the step, whatever the flags: the last report was laid out under the old value and is void --
        # no getter reads lists that were never written; the next step's bytes are the same under every value
        for flags, capacity in ((0, 65536), (ALL, 1), (ALL, 65536), (0, 0), (ALL, 0)):
            s.world_set_sensor_report(flags, capacity)
            refuses(s, E_STATE, ("world_sensor_inside", "world_sensor_events", "world_sensor_states"))
            if flags:
                before = now
                step_both(s, params, ref_world)
                now = device_lists(s, ref_world, sensors)
                assert_report(s, ref_world, sensors, before, now, "listCapacity %d" % capacity)
        s.world_set_sensor_report(0, 0)  # the same value again with flags 0: the last report stands, as with the other reports
        assert_report(s, ref_world, sensors, before, now, "flags 0 after the step", raw=False)
        s.world_set_sensor_report(ALL, 0)
        # a new list between steps: the caller's act raises no events, and the last step's report is void
        moved = sensors.copy()
        moved["position"] += np.float32((0.4, -0.3))
        moved = np.concatenate([moved, sensors[:1]])
        s.world_set_sensors(moved)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_sensor_inside()
        changed = device_lists(s, ref_world, moved)
        assert changed[:3] != now  # (what a report that kept the old "before" would list as events)
        before = changed
        for k in range(2):
            step_both(s, params, ref_world)
            now = device_lists(s, ref_world, moved)
            assert_report(s, ref_world, moved, before, now, "the new list, step %d" % k)
            before = now
        # an upload in between re-bases "before": another world with other capacities, the list held across it; the sensor whose
        # body lies outside the new world is inactive there
        fx2 = sw.load_fixture("ball")
        world2, ref_world2 = sw.fixture_world(fx2), sw.fixture_world(fx2)
        assert moved[1]["body"] >= len(world2["bodies"])
        upload(s, world2)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_sensor_states()
        before = device_lists(s, ref_world2, moved)
        assert before[1] == []
        for k in range(3):
            step_both(s, params, ref_world2)
            now = device_lists(s, ref_world2, moved)
            assert_report(s, ref_world2, moved, before, now, "after the second upload, step %d" % k)
            before = now
        assert s.world_sensor_states()["active"].tolist() == [1, 0, 1, 1]
        # cleared: nothing to report, and the getters say so
        s.world_set_sensors(np.zeros(0, dtype=wire.sensor_dtype))
        step_both(s, params, ref_world2)
        assert_report(s, ref_world2, moved[:0], [], [], "no sensors")


def test_flags_zero_is_a_solver_that_never_heard_of_sensors():
    """Two solvers in lockstep on the pyramid scene, one with the sensors set and no flag and one without: the same step info, kernel
    launches and world bytes every step, and the getters refuse."""
    fx = sw.load_fixture("pyramid")
    world, sensors, params = sw.fixture_world(fx), fx["sensors"], sw.params()
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    with hip.Solver(0) as on, hip.Solver(0) as off:
        on.world_set_sensors(sensors)
        on.world_set_sensor_report(0, 64)
        upload(on, world), upload(off, world)
        compared = 0
        for step in range(6):
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            sa, sb = on.stats(), off.stats()
            if (sa["structureBuilds"], sa["asyncBuildsAdopted"]) == (sb["structureBuilds"], sb["asyncBuildsAdopted"]):
                assert sa["kernelLaunches"] == sb["kernelLaunches"] and sa["solveLaunches"] == sb["solveLaunches"], "step %d: %r / %r" % (step, sa, sb)
                compared += 1
            refuses(on, E_STATE, ("world_sensor_inside", "world_sensor_events", "world_sensor_states"))
            wa, wb = downloaded_world(on, world), downloaded_world(off, world)
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert compared >= 3


def test_a_step_the_library_repeats_reports_once():
    """The base-100 pyramid stepped by the one-launch kernel with a hand-off that never arrives (option persist_debug 8, as
    tests/test_gpu_strips.py injects it): the library repeats the step on another path, and the report is of the step that stands,
    once -- the events are the difference between the lists before and after it."""
    world = synthetic.pyramid_world(100)
    ref_world, params = world_chain.copy_world(world), sw.params()
    top = len(world["bodies"]) - 1
    sensors = np.array([sw.make_sensor([(0.0, 0.0)], 1.2, (0.0, 0.0), body=top), sw.make_sensor(sw.box_vertices(3.0, 0.75), 0.0, (0.0, 0.7), margin=0.1),
                        sw.make_sensor(sw.box_vertices(3.0, 0.75), 0.0, (0.0, 0.7), margin=0.1, flags=wire.SENSOR_SKIP_STATIC)], dtype=wire.sensor_dtype)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        s.set_option("persist_spin_limit", 4096)
        s.set_option("persist_debug", 8)
        s.world_set_sensors(sensors)
        s.world_set_sensor_report(ALL, 16)
        upload(s, world)
        before = device_lists(s, ref_world, sensors)
        assert len(before[0]) >= 2 and len(before[1]) == len(before[2]) + 1 >= 4
        step_both(s, params, ref_world)
        assert s.stats()["persistFallbacks"] >= 1
        now = device_lists(s, ref_world, sensors)
        assert_report(s, ref_world, sensors, before, now, "the repeated step")
        before = now
        step_both(s, params, ref_world)
        assert_report(s, ref_world, sensors, before, device_lists(s, ref_world, sensors), "the step after it")
