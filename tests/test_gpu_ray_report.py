"""The ray report of the resident world (s2amd_world_set_ray_sensors / _set_ray_report / _ray_states / _ray_ranges /
_export_ray_ranges / _ray_events; solver2d_amd/csrc/ray_report.hip) against its statement (tests/ray_report_ref.py), byte for byte:
the recorded hit shapes and events of tests/golden/ray_report on the oracle chain of tests/world_chain.py stepped in the device's
orders, the statement itself where the reference library is built, and the device's own s2amd_world_ray_cast of the world rays
wherever the two exclusions change nothing."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import ray_report_ref as ref, ray_report_world as rw, sensor_report_world as sw, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, downloaded_world, refuses, step_both, upload

pytestmark = pytest.mark.gpu

ALL = wire.RAY_REPORT_ALL
DISABLED, SKIP_STATIC = wire.RAY_SENSOR_DISABLED, wire.RAY_SENSOR_SKIP_STATIC
GETTERS = ("world_ray_states", "world_ray_ranges", "world_ray_events")


def c_getters(s, count):
    """The three host getters through the raw C calls with buffers of exactly the stated sizes: asked one entry short first, which must
    state the count and touch nothing."""
    L, h = s._L, s._h
    n = ctypes.c_int32(-7)
    states, ranges = np.zeros(count, dtype=wire.ray_state_dtype), np.full(count, -3.0, dtype=np.float32)
    if count > 0:
        assert (L.s2amd_world_ray_states(h, wire.as_ptr(states), count - 1, ctypes.byref(n)), n.value) == (E_CAPACITY, count) and states.tobytes() == bytes(64 * count)
        assert (L.s2amd_world_ray_ranges(h, wire.as_ptr(ranges), count - 1, ctypes.byref(n)), n.value) == (E_CAPACITY, count) and (ranges == -3.0).all()
    assert (L.s2amd_world_ray_states(h, wire.as_ptr(states) if count else None, count, ctypes.byref(n)), n.value) == (0, count)
    assert (L.s2amd_world_ray_ranges(h, wire.as_ptr(ranges) if count else None, count, ctypes.byref(n)), n.value) == (0, count)
    rc = L.s2amd_world_ray_events(h, None, 0, ctypes.byref(n))
    assert rc == (E_CAPACITY if n.value > 0 else 0), rc
    events = np.zeros(n.value, dtype=wire.ray_event_dtype)
    if n.value > 0:
        events.view(np.uint8)[:] = 0xFF
        assert (L.s2amd_world_ray_events(h, wire.as_ptr(events), len(events) - 1, ctypes.byref(n)), n.value) == (E_CAPACITY, len(events))
        assert (events.view(np.uint8) == 0xFF).all()
    assert (L.s2amd_world_ray_events(h, wire.as_ptr(events) if len(events) else None, len(events), ctypes.byref(n)), n.value) == (0, len(events))
    return states, ranges, events


def tiled_states(world, rays, before, period):
    """The statement's states of a list that repeats its first `period` rays (and whose `before` repeats likewise)"""
    if period is None or period >= len(rays):
        return ref.states(world, rays, before)
    assert all(rays[i].tobytes() == rays[i % period].tobytes() and before[i] == before[i % period] for i in range(len(rays)))
    head = ref.states(world, rays[:period], before[:period])
    out = np.array([head[i % period] for i in range(len(rays))], dtype=wire.ray_state_dtype)
    out["ray"] = np.arange(len(rays))
    return out


def assert_one_shot(s, world, rays, states, what):
    """s2amd_world_ray_cast of the statement's world rays, asked of the same solver: field by field the state of every active ray whose
    one-shot winner neither exclusion removes (then it is the winner among the fewer candidates as well); where it is removed, the
    state names another shape."""
    plain, index = ref.world_rays(world, rays)
    active = np.zeros(len(rays), dtype=bool)
    active[index] = True
    assert states["active"].tolist() == active.astype(int).tolist(), what
    idle = states[~active]
    assert (idle["shape"] == -1).all() and (idle["hitBody"] == -1).all() and idle["fraction"].tobytes() == rays["maxFraction"][~active].tobytes(), what
    for name in ("p1", "p2", "point", "normal"):
        assert idle[name].tobytes() == bytes(8 * len(idle)), (what, name)
    if not index:
        return 0
    hits = s.world_ray_cast(plain)
    st, q = states[index], rays[index]
    static = world["bodies"]["type"] == wire.BODY_STATIC
    removed = (hits["body"] >= 0) & (((q["body"] >= 0) & (hits["body"] == q["body"])) | (((q["flags"] & SKIP_STATIC) != 0) & static[np.maximum(hits["body"], 0)]))
    assert st["p1"].tobytes() == plain["p1"].tobytes() and st["p2"].tobytes() == plain["p2"].tobytes(), what
    for mine, theirs in (("shape", "shape"), ("hitBody", "body"), ("fraction", "fraction"), ("point", "point"), ("normal", "normal")):
        assert st[mine][~removed].tobytes() == hits[theirs][~removed].tobytes(), (what, mine)
    assert (st["shape"][removed] != hits["shape"][removed]).all(), what
    return int((~removed).sum())


def assert_report(s, world, rays, before, what, period=None, raw=True, one_shot=True):
    """Every getter, through hip.py and through the C calls: the structure every report has, the one-shot call, and the statement's
    bytes where the reference is built.  `world` holds the resident world's bytes.  -> the hit shapes now"""
    got = [(s.world_ray_states(), s.world_ray_ranges(), s.world_ray_events(expected=max(len(rays), 1)))]
    if raw:
        got.append(c_getters(s, len(rays)))
    want = tiled_states(world, rays, before, period) if ref.available() else None
    for states, ranges, events in got:
        assert states["ray"].tolist() == list(range(len(rays))) and states["body"].tobytes() == rays["body"].tobytes(), what
        assert states["shapeBefore"].tolist() == list(before), "%s: shapeBefore %s, expected %s" % (what, states["shapeBefore"].tolist(), list(before))
        assert (states["pad"] == 0).all() and ranges.tobytes() == states["fraction"].tobytes(), what
        hit = states["shape"] >= 0
        assert (states["hitBody"][hit] == world["shapes"]["body"][states["shape"][hit]]).all() and (states["hitBody"][~hit] == -1).all(), what
        assert events.tobytes() == ref.events_of(list(before), states).tobytes(), "%s: events %s" % (what, events)
        if want is not None and states.tobytes() != want.tobytes():
            bad = [n for n in states.dtype.names if states[n].tobytes() != want[n].tobytes()]
            rows = np.flatnonzero([states[i].tobytes() != want[i].tobytes() for i in range(len(states))])
            raise AssertionError("%s: states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), states[rows[:2]], want[rows[:2]]))
    assert got[0][0].tobytes() == got[-1][0].tobytes()
    if one_shot:
        assert_one_shot(s, world, rays, got[0][0], what)
    return got[0][0]["shape"].tolist()


@pytest.mark.parametrize("scene,fast", [(scene, fast) for scene in rw.SCENES for fast in (False, True)])
def test_recorded_scenes_every_step(scene, fast):
    """The three scenes of tests/golden/ray_report for 12 steps in both libraries: the recorded hit shapes and events every step; in
    libs2amd.so the states, ranges and events on the chain in the device's orders against the statement, and the world's bytes at the end."""
    fx = rw.load_fixture(scene)
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0, fast=fast) as s:
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(ALL)
        upload(s, world)
        before = fx["before"].tolist()
        for k in range(rw.STEPS):
            step_both(s, params, ref_world)
            what = "%s step %d" % (scene, k)
            if not fast:
                # (the tolerance mode's poses are not the oracle chain's; its hit shapes are, under the fixtures' clearance)
                now = assert_report(s, ref_world, rays, before, what, raw=k in (0, 7))
            else:
                now = s.world_ray_states()["shape"].tolist()
                assert s.world_ray_states()["shapeBefore"].tolist() == before, what
            assert now == fx["hits_%d" % k].tolist(), "%s: hit shapes %s, recorded %s" % (what, now, fx["hits_%d" % k].tolist())
            assert s.world_ray_events().tobytes() == fx["events_%d" % k].tobytes(), what
            before = now
        if not fast:
            world_chain.assert_device_equals_oracle(downloaded_world(s, world), ref_world, scene)


def test_agreement_with_the_one_shot_call():
    """Fixed rays without flags: s2amd_world_ray_states agrees field by field with s2amd_world_ray_cast of the same rays on the same
    solver, every one of them.  Mounted rays: with the call of the statement's world rays wherever the exclusions change nothing."""
    world = sw.sweep_world(513)
    rng = np.random.RandomState(3)
    fixed = []
    for _ in range(300):
        a = (rng.rand() * 9.0 - 0.5, rng.rand() * 21.0)
        angle = rng.rand() * 6.28
        fixed.append(rw.make_ray(a, (a[0] + 4.0 * np.cos(angle), a[1] + 4.0 * np.sin(angle)), max_fraction=(0.25, 1.0, 1.5)[rng.randint(3)]))
    fixed = np.array(fixed, dtype=wire.ray_sensor_dtype)
    carriers = [int(b) for b in world["shapes"]["body"][[7, 70, 300, 501]]]
    mounted = np.array([rw.make_ray((0.0, 0.0), (3.0 * np.cos(a), 3.0 * np.sin(a)), body=b, flags=SKIP_STATIC if j % 3 == 0 else 0)
                        for b in carriers for j, a in enumerate(np.linspace(0.0, 6.0, 16))]
                       + [rw.make_ray((0.9, 0.0), (-3.0, 0.1 * j), body=b) for b in carriers for j in range(4)], dtype=wire.ray_sensor_dtype)
    params = sw.params()
    with hip.Solver(0) as s:
        s.world_set_ray_report(wire.RAY_REPORT_STATES)
        upload(s, world)
        for rays, what in ((fixed, "fixed"), (mounted, "mounted")):
            s.world_set_ray_sensors(rays)
            for k in range(2):
                s.world_step(params)
                now = downloaded_world(s, world)
                states = s.world_ray_states()
                kept = assert_one_shot(s, now, rays, states, "%s rays, step %d" % (what, k))
                if what == "fixed":
                    assert kept == len(rays)
                    hits = s.world_ray_cast(ref.world_rays(now, rays)[0])
                    assert (hits["shape"] >= 0).sum() >= 100 and (hits["shape"] < 0).sum() >= 3
                else:
                    assert 10 <= kept < len(rays) and (states["shape"] >= 0).sum() >= 10


def sweep_rays(world, count):
    """`count` rays that repeat eight distinct ones: a tall fixed ray up a lattice column (candidates in every wave of every tile), a
    fixed one across the rows, one carried by a falling body that points through the body's own shape, one from the ground's body down
    through the ground with SKIP_STATIC, a DISABLED copy of the first, one on the free body slot, one that passes category 2 only
    (nothing), and one with maxFraction 0."""
    bodies, shapes = world["bodies"], world["shapes"]
    slot = min(70, len(shapes) - 1)
    carrier = int(shapes["body"][slot]) if shapes["type"][slot] != wire.SHAPE_FREE else 1
    assert bodies["type"][carrier] == wire.BODY_DYNAMIC and bodies["type"][len(bodies) - 1] == wire.BODY_FREE
    distinct = [
        rw.make_ray((3.1, -0.5), (3.3, 22.0)),
        rw.make_ray((-1.0, 2.2), (9.0, 2.9)),
        rw.make_ray((1.0, 0.1), (-2.5, 0.3), body=carrier),
        rw.make_ray((-1.5, 4.0), (-1.4, -1.0), body=0, flags=SKIP_STATIC),
        rw.make_ray((3.1, -0.5), (3.3, 22.0), flags=DISABLED),
        rw.make_ray((0.0, 0.0), (5.0, 5.0), body=len(bodies) - 1),
        rw.make_ray((3.1, -0.5), (3.3, 22.0), mask=2),
        rw.make_ray((3.1, 1.0), (3.3, 22.0), max_fraction=0.0),
    ]
    return np.array([distinct[i % len(distinct)] for i in range(count)], dtype=wire.ray_sensor_dtype)


def run_sweep(slots, count, steps=2):
    world = sw.sweep_world(slots)
    rays = sweep_rays(world, count)
    params = sw.params()
    seen = {"events": 0, "hits": 0}
    with hip.Solver(0) as s:
        s.world_set_ray_report(ALL)
        s.world_set_ray_sensors(rays)
        upload(s, world)
        before = ref.hits(world, rays[:8]) if ref.available() else None
        for k in range(steps):
            s.world_step(params)
            now = downloaded_world(s, world)
            if before is None:
                before = s.world_ray_states()["shapeBefore"][:8].tolist()  # (no reference here: the structure and the one-shot call only)
            full = [before[i % 8] for i in range(count)]
            shapes = assert_report(s, now, rays, full, "%d slots, %d rays, step %d" % (slots, count, k), period=8, raw=k == 0, one_shot=count <= 1024)
            seen["events"] += len(s.world_ray_events(expected=max(count, 1)))
            seen["hits"] += sum(1 for x in shapes if x >= 0)
            assert shapes == [shapes[i % 8] for i in range(count)]
            before = shapes[:8] if count >= 8 else (shapes + before[count:])
    return seen


@pytest.mark.parametrize("slots", [63, 64, 65, 255, 256, 257, 513])
def test_shape_capacities_at_the_wave_and_tile_edges(slots):
    """Eight rays over worlds whose last shape slot is the last lane of a wave or tile, the first of the next, or one short; free slots
    among them.  The tall ray's candidates lie in every wave of every tile."""
    seen = run_sweep(slots, 8)
    assert seen["hits"] >= 4, seen


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 16384])
def test_ray_counts_at_the_group_and_chunk_edges(count):
    """257 shape slots (two tiles, the second with one slot) under 0 and 1 rays, one group of 64 (a workgroup of the candidates pass)
    less one, one group, one more, the same for a chunk of 256 (a workgroup of the other passes), and the most rays a list takes (256
    groups; 64 chunks: the events pass's whole prefix)."""
    seen = run_sweep(257, count, steps=2 if count < 16384 else 1)
    if count == 0:
        assert seen == {"events": 0, "hits": 0}
    else:
        assert seen["hits"] >= 1


def test_the_chunk_box_decides_nothing():
    """One list of 1,024 rays -- three tight fans of 256 in three corners of the world and 256 inactive ones -- in three orders: every
    chunk one fan, every chunk a mix of all corners, and a chunk of inactive rays in the middle.  After undoing the permutation the
    answers are the same bytes, and they are the one-shot call's."""
    world = sw.sweep_world(513)
    corners = [((0.2, 1.0), 0.0), ((7.4, 16.5), 3.1), ((7.2, 1.2), 1.6)]
    fans = [[rw.make_ray(o, (o[0] + 3.0 * np.cos(a0 + 0.006 * j), o[1] + 3.0 * np.sin(a0 + 0.006 * j))) for j in range(256)] for o, a0 in corners]
    idle = [rw.make_ray((3.0, 3.0), (4.0, 9.0), flags=DISABLED)] * 192 + [rw.make_ray((0.0, 0.0), (1.0, 1.0), body=len(world["bodies"]) - 1)] * 64
    base = np.array(fans[0] + fans[1] + fans[2] + idle, dtype=wire.ray_sensor_dtype)
    tight = np.arange(1024)
    mixed = np.concatenate([np.arange(768).reshape(3, 256).T.reshape(-1), np.arange(768, 1024)])
    middle = np.concatenate([np.arange(0, 256), np.arange(768, 1024), np.arange(256, 768)])
    params = sw.params()
    answers = []
    for order in (tight, mixed, middle):
        assert sorted(order.tolist()) == list(range(1024))
        with hip.Solver(0) as s:
            s.world_set_ray_report(ALL)
            s.world_set_ray_sensors(base[order])
            upload(s, world)
            per_step = []
            for k in range(2):
                s.world_step(params)
                states, ranges, events = s.world_ray_states(), s.world_ray_ranges(), s.world_ray_events(expected=1024)
                if k == 0:
                    assert_one_shot(s, downloaded_world(s, world), base[order], states, "order %d" % len(answers))
                undone = np.zeros(1024, dtype=wire.ray_state_dtype)
                undone[order] = states
                assert states["ray"].tolist() == list(range(1024))
                undone["ray"] = 0
                back = np.zeros(1024, dtype=np.float32)
                back[order] = ranges
                changed = np.zeros(1024, dtype=bool)
                changed[order[events["ray"]]] = True
                per_step.append((undone.tobytes(), back.tobytes(), changed.tobytes()))
            answers.append(per_step)
    assert answers[0] == answers[1] == answers[2]
    first = np.frombuffer(answers[0][0][0], dtype=wire.ray_state_dtype)
    assert (first["shape"][:768] >= 0).sum() >= 100 and (first["shape"][:768] < 0).sum() >= 10 and (first["active"][768:] == 0).all()


def test_export_into_a_device_buffer():
    fx = rw.load_fixture("pyramid")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    with hip.Solver(0) as s:
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(wire.RAY_REPORT_RANGES)
        upload(s, world)
        room = len(rays) + 3
        buf = s.device_alloc(4 * room)
        try:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_export_ray_ranges(buf, room)  # no step since the upload
            for k in range(3):
                s.world_step(params)
                with pytest.raises(hip.S2AmdError, match="error %d" % E_CAPACITY):
                    s.world_export_ray_ranges(buf, len(rays) - 1)
                s.world_export_ray_ranges(buf, room)
                got = s.device_read(buf, (room,), np.float32)
                ranges = s.world_ray_ranges()
                assert got[:len(rays)].tobytes() == ranges.tobytes() and got[len(rays):].tobytes() == bytes(12)
                assert (ranges < rays["maxFraction"]).sum() >= 3
            s.world_set_ray_report(wire.RAY_REPORT_STATES)
            s.world_step(params)
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_export_ray_ranges(buf, room)  # its flag was not set before the step
        finally:
            s.device_free(buf)


def test_lifecycle_set_rays_uploads_flags_and_errors():
    fx = rw.load_fixture("chain")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        n, out = ctypes.c_int32(-7), np.full(64, -1, dtype=np.int32)
        # no resident world
        assert L.s2amd_world_ray_events(h, wire.as_ptr(out), 4, ctypes.byref(n)) == E_STATE and n.value == -7 and (out == -1).all()
        refuses(s, E_STATE, GETTERS)
        for bad in (8, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_ray_report(bad)
        s.world_set_ray_sensors(rays)
        for field, value in (("maxFraction", -0.5), ("maxFraction", 100000.0), ("maxFraction", np.nan), ("p1", (np.inf, 0.0)), ("p2", (0.0, np.nan)), ("flags", 4)):
            wrong = rays.copy()
            wrong[1][field] = value
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_ray_sensors(wrong)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_ray_sensors(np.zeros(wire.MAX_RAY_SENSORS + 1, dtype=wire.ray_sensor_dtype))
        s.world_set_ray_report(wire.RAY_REPORT_EVENTS)
        upload(s, world)
        wrong = rays.copy()
        wrong[0]["body"] = len(world["bodies"])
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_ray_sensors(wrong)  # a body outside the resident world: refused, the old list stands
        refuses(s, E_STATE, GETTERS)  # no step since the upload
        before = fx["before"].tolist()
        step_both(s, params, ref_world)
        assert s.world_ray_events().tobytes() == fx["events_0"].tobytes()
        refuses(s, E_STATE, ("world_ray_states", "world_ray_ranges"))  # their flags were not set before the step
        s.world_set_ray_report(ALL)
        refuses(s, E_STATE, ("world_ray_states", "world_ray_ranges"))  # a flag set between two steps takes effect from the next step
        before = fx["hits_0"].tolist()
        for k in range(1, 4):
            step_both(s, params, ref_world)
            before = assert_report(s, ref_world, rays, before, "all flags, step %d" % k, raw=k == 3)
            assert before == fx["hits_%d" % k].tolist()
        s.world_set_ray_report(0)  # flags 0: the last report stands, as with the other reports
        assert s.world_ray_states()["shape"].tolist() == before
        s.world_set_ray_report(ALL)  # turned on again: "before" re-based, the last report void
        refuses(s, E_STATE, GETTERS)
        # a new list between steps: the caller's act raises no events, and the last step's report is void
        moved = np.concatenate([rays[::-1], rays[:3]])
        moved["p1"][moved["body"] < 0] += np.float32((0.15, -0.1))
        s.world_set_ray_sensors(moved)
        refuses(s, E_STATE, GETTERS)
        now = downloaded_world(s, world)
        shapes = ref.hits(now, moved) if ref.available() else None
        step_both(s, params, ref_world)
        if shapes is None:
            shapes = s.world_ray_states()["shapeBefore"].tolist()
        before = assert_report(s, ref_world, moved, shapes, "the new list, step 0")
        step_both(s, params, ref_world)
        before = assert_report(s, ref_world, moved, before, "the new list, step 1")
        # cleared: nothing to report, and the getters say so
        s.world_set_ray_sensors(moved[:0])
        refuses(s, E_STATE, GETTERS)
        step_both(s, params, ref_world)
        assert_report(s, ref_world, moved[:0], [], "no rays")
        s.world_set_ray_sensors(moved)
        # an upload re-bases "before": another world with other capacities, the list held across it; the rays whose body lies
        # outside the new world are inactive there
        fx2 = rw.load_fixture("ball")
        world2 = rw.fixture_world(fx2)
        on_link = moved["body"] >= len(world2["bodies"])
        assert on_link.sum() >= 8
        upload(s, world2)
        refuses(s, E_STATE, GETTERS)
        before = None
        for k in range(3):
            s.world_step(params)
            states = s.world_ray_states()
            before = states["shapeBefore"].tolist() if before is None else before
            assert (states["active"][on_link] == 0).all() and states["active"][~on_link].sum() >= 3
            before = assert_report(s, downloaded_world(s, world2), moved, before, "after the upload of another world, step %d" % k)


def test_a_body_freed_under_a_ray_turns_the_ray_inactive():
    """A body slot of a resident world becomes free through an upload, which re-bases "before" as every act of the caller does: the
    rays mounted on the ball see past it every step, then the ball's slot and shape are freed and the world uploaded again -- the
    rays are inactive misses with +0 ends, and their turning inactive is no event."""
    fx = rw.load_fixture("ball")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    mounted = np.flatnonzero(rays["body"] >= 0)
    ball = int(rays["body"][mounted[0]])
    with hip.Solver(0) as s:
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(ALL)
        upload(s, world)
        for k in range(9):
            s.world_step(params)
        states = s.world_ray_states()
        assert (states["active"][mounted] == 1).all() and (states["shape"][mounted] >= 0).all()
        freed = downloaded_world(s, world)
        freed["bodies"]["type"][ball] = wire.BODY_FREE
        on_ball = freed["shapes"]["body"] == ball
        freed["shapes"]["type"][on_ball], freed["shapes"]["body"][on_ball] = wire.SHAPE_FREE, -1
        upload(s, freed)
        refuses(s, E_STATE, GETTERS)
        s.world_step(params)
        states, events = s.world_ray_states(), s.world_ray_events()
        idle = states[mounted]
        assert (idle["active"] == 0).all() and (idle["shape"] == -1).all() and (idle["shapeBefore"] == -1).all()
        assert idle["fraction"].tobytes() == rays["maxFraction"][mounted].tobytes() and idle["p1"].tobytes() == bytes(64) and idle["p2"].tobytes() == bytes(64)
        assert not np.isin(events["ray"], mounted).any()
        assert_report(s, downloaded_world(s, freed), rays, states["shapeBefore"].tolist(), "the ball freed")


def test_flags_zero_is_a_solver_that_never_heard_of_rays():
    """Two solvers in lockstep on the pyramid scene, one with the rays set and no flag and one without: the same step info, kernel
    launches and world bytes every step, and the getters refuse."""
    fx = rw.load_fixture("pyramid")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    with hip.Solver(0) as on, hip.Solver(0) as off:
        on.world_set_ray_sensors(rays)
        on.world_set_ray_report(0)
        upload(on, world), upload(off, world)
        compared = 0
        for step in range(6):
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            sa, sb = on.stats(), off.stats()
            if (sa["structureBuilds"], sa["asyncBuildsAdopted"]) == (sb["structureBuilds"], sb["asyncBuildsAdopted"]):
                assert sa["kernelLaunches"] == sb["kernelLaunches"] and sa["solveLaunches"] == sb["solveLaunches"], "step %d: %r / %r" % (step, sa, sb)
                compared += 1
            refuses(on, E_STATE, GETTERS)
            wa, wb = downloaded_world(on, world), downloaded_world(off, world)
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert compared >= 3


def test_together_with_the_older_facilities():
    """The pyramid scene with the sensors of tests/golden/sensor_report, a persistent wind field and all seven reports on, beside a
    solver with everything but the rays: the ray report equals its statement on the resident world's bytes, the sensors' lists are the
    other solver's, and so is every getter of the other five reports and the world itself."""
    fx, sfx = rw.load_fixture("pyramid"), sw.load_fixture("pyramid")
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    fields = wire.field_list([wire.field_uniform((0.0, 2.0), 6.0, 3.0, (1.0, 0.0))])

    def everything(s):
        s.world_set_report(wire.REPORT_ALL)
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_body_report(wire.BODY_REPORT_ALL)
        s.world_set_metrics(wire.METRICS_ALL, 4)
        s.world_set_sensors(sfx["sensors"])
        s.world_set_sensor_report(wire.SENSOR_REPORT_ALL, 64)
        s.world_set_fields(fields)

    def others(s):
        out = [s.world_touch_events(), s.world_touching(), s.world_body_sums(), s.world_joint_states(), s.world_joint_summary(), s.world_shape_draws(),
               s.world_shape_view_events(), s.world_shape_summary(), s.world_body_states(), s.world_body_rest_events(), s.world_islands(), s.world_body_summary(),
               s.world_metrics(), s.world_sensor_inside(), s.world_sensor_events(), s.world_sensor_states(), s.world_field_states()]
        flat = []
        for x in out:
            flat += [np.ascontiguousarray(y).tobytes() for y in (x if isinstance(x, tuple) else (x,))]
        return flat

    with hip.Solver(0) as a, hip.Solver(0) as b:
        everything(a), everything(b)
        a.world_set_ray_sensors(rays)
        a.world_set_ray_report(ALL)
        upload(a, world), upload(b, world)
        before = None
        for k in range(5):
            a.world_step(params), b.world_step(params)
            now = downloaded_world(a, world)
            states = a.world_ray_states()
            before = states["shapeBefore"].tolist() if before is None else before
            before = assert_report(a, now, rays, before, "everything on, step %d" % k, raw=k == 0)
            got, want = others(a), others(b)
            assert len(got) == len(want) and [i for i in range(len(got)) if got[i] != want[i]] == [], "step %d" % k
            theirs = downloaded_world(b, world)
            for key in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(now[key]).tobytes() == np.ascontiguousarray(theirs[key]).tobytes(), "step %d: %s" % (k, key)
        assert sum(1 for x in before if x >= 0) >= 3
