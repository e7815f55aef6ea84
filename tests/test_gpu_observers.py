"""Observers on the resident world (s2amd_world_set_observers / _set_observation_report / _observations / _export_observations(_async)
/ _observer_states / _observer_counts; solver2d_amd/csrc/observers.hip) against their statement (tests/observer_ref.py: numpy float32,
the angles through glibc's atan2f), byte for byte.  The pass runs behind s2amd_world_step, so every case steps: vector, states and
counts equal the statement applied to the oracle chain's world after the same step (tests/world_chain.py).  The contact sums the
statement reads are tests/contact_report_ref.py's on that world; the ray ranges are s2amd_world_ray_ranges' own answer, which the
vector carries verbatim (tests/test_gpu_ray_report.py pins that getter).  The worlds are the committed tests/golden/world_*_step*.npz;
the sizes need more than 1,024 body slots and take a synthetic pyramid."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import actuator_ref, body_report_ref, contact_report_ref, joint_report_ref, observer_ref as ref, shape_report_ref, world_chain
from tests import grid_report_world as gw, sensor_report_world as sw
from tests.grid_report_world import assert_report as assert_grid_report
from tests.resident import (E_CAPACITY, E_INVALID, E_STATE, assert_metrics_equal_reference, assert_same_world, down_ray, download, every_kind, motorised, packed,
                            refuses, slots_of, step_both, upload)
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

F = np.float32
VECTOR, STATES = wire.OBSERVATION_REPORT_VECTOR, wire.OBSERVATION_REPORT_STATES
BOTH = VECTOR | STATES
POINT, ROTATION, ANGLE, LINEAR, ANGULAR, REV_ANGLE, REV_SPEED, REV_IMPULSE, CONTACT, RAY, ACTION = range(1, 12)
RELATIVE, DISABLED = wire.OBSERVER_RELATIVE, wire.OBSERVER_DISABLED


def assert_states(got, want, what):
    assert got.dtype == wire.observer_state_dtype and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))


def expect(s, after, observers, history, what, sums=False, ranges=False, rays=0, actions=None, action_channels=0, states=True):
    """The statement on `after` (the world after the step) against the three getters -> (vector, states, counts, frames)"""
    sources = (contact_report_ref.body_sums(after) if sums else None, s.world_ray_ranges() if ranges else None, actions)
    vector, want_states, counts = ref.observe(after, observers, sources, channels=history.rows.shape[1], lengths=(rays, action_channels))
    frames = history.push(vector)
    got = s.world_observations()
    assert got.shape == frames.shape and got.dtype == np.float32, what
    if got.tobytes() != frames.tobytes():
        where = np.argwhere(got.view(np.uint32) != frames.view(np.uint32))
        raise AssertionError("%s: the vector differs at (frame, channel) %s: %s / %s" % (what, where[:4].tolist(), got[tuple(where[0])], frames[tuple(where[0])]))
    if states:
        assert_states(s.world_observer_states(), want_states, what)
    assert s.world_observer_counts().tolist() == counts.tolist(), what
    return vector, want_states, counts, frames


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
def test_every_kind_once(fast):
    """mixed24_PGS with its motors on and driven, the contact sums and the ray ranges on, an actuator list set.  In the tolerance-mode
    library, whose step is not the oracle's, the statement is applied to that library's own downloaded world: the pass is the same bits."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    at = slots_of(world)
    observers, channels = every_kind(world)
    assert sorted(observers["kind"].tolist()) == list(range(1, 12))
    actuators = wire.actuator_list([wire.actuator(5, at["revolute"][0], 0, gain=3.0), wire.actuator(5, at["revolute"][1], 1, gain=-2.0)])
    actions = np.array([0.75, -0.5], dtype=F)
    rays = np.array([down_ray(world, at["dynamic"][0])], dtype=wire.ray_sensor_dtype)
    with hip.Solver(0, fast=fast) as s:
        s.world_set_report(wire.REPORT_BODY_SUMS)
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(wire.RAY_REPORT_RANGES)
        s.world_set_actuators(actuators, 2)
        s.world_set_actions(actions)
        s.world_set_observers(observers, channels)
        s.world_set_observation_report(BOTH)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(1, channels)
        for step in range(3):
            actuator_ref.apply(ref_world, actuators, actions)
            step_both(s, params, ref_world)
            after = download(s, world)[0] if fast else ref_world
            vector, states, counts, _ = expect(s, after, observers, history, "mixed24 step %d" % step, sums=True, ranges=True, rays=1, actions=actions, action_channels=2)
            assert counts.tolist() == [11, 0, 0, 0] and (states["status"] == ref.OBSERVED).all()
        # nothing is trivially zero: every raw component and every value, the contact flag included
        assert (states["raw"][observers["kind"] != CONTACT][:, 0] != 0).all() and (vector != 0).all() and len(vector) == 15
        assert states["raw"][8].tolist()[0] == 1.0 and states["raw"][8][1] > 0
        if not fast:
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "mixed24")


def test_frames_on_the_ragdoll():
    """ragdoll0: kinds 1-5 in the world frame and in a body's frame, with and without RELATIVE, non-zero `local`; the list with target
    and frame swapped gives other bytes in every framed observer."""
    params, world = golden("ragdoll0_PGS_NGS_Block")
    d = slots_of(world)["dynamic"]
    torso, limb = int(d[0]), int(d[5])

    def listed(target, frame):
        records = []
        for kind in (POINT, ROTATION, ANGLE, LINEAR, ANGULAR):
            for fr, flags in ((-1, 0), (frame, 0), (frame, RELATIVE), (-1, RELATIVE)):
                records.append((kind, target, dict(frame=fr, flags=flags, local=(0.375, -0.25), gain=1.5, bias=-0.0625)))
        return packed(records)

    observers, channels = listed(limb, torso)
    swapped, _ = listed(torso, limb)
    with hip.Solver(0) as s:
        s.world_set_observers(observers, channels)
        s.world_set_observation_report(BOTH)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(1, channels)
        for step in range(4):
            step_both(s, params, ref_world)
            vector, states, counts, _ = expect(s, ref_world, observers, history, "ragdoll0 step %d" % step)
            assert counts.tolist() == [len(observers), 0, 0, 0]
        other = ref.observe(ref_world, swapped, (None, None, None), channels=channels)[1]
        framed = observers["frame"] >= 0
        assert all(a.tobytes() != b.tobytes() for a, b in zip(states["value"][framed], other["value"][framed]))
        # RELATIVE changes the velocities in a frame and nothing without one
        for kind in (LINEAR, ANGULAR):
            rows = np.flatnonzero(observers["kind"] == kind)
            assert states["raw"][rows[1]].tobytes() != states["raw"][rows[2]].tobytes() and states["raw"][rows[0]].tobytes() == states["raw"][rows[3]].tobytes()
        # the same list on the swapped solver
        s.world_set_observers(swapped, channels)
        step_both(s, params, ref_world)
        expect(s, ref_world, swapped, ref.History(1, channels), "ragdoll0 swapped")
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "ragdoll0")


def test_statuses():
    """DISABLED; SKIPPED for a free slot, a mouse joint under kind 6, a frame on a free slot and targets beyond the capacities of a smaller
    upload; SOURCE_OFF with each source's flag off and OBSERVED in the next step once it is on."""
    params, world = golden("mixed24_PGS")
    at = slots_of(world)
    d = at["dynamic"]
    assert len(at["free"]) and len(at["mouse"]) and len(at["free_joint"])
    quiet, channels = packed([(POINT, d[0], dict(flags=DISABLED, bias=1.0)), (LINEAR, at["free"][0], dict(bias=1.0)), (REV_ANGLE, at["mouse"][0], dict(bias=1.0)),
                              (ROTATION, d[-2], dict(frame=at["free"][0], bias=1.0)), (REV_SPEED, at["free_joint"][0], dict(bias=1.0)),
                              (CONTACT, at["free"][0], dict(bias=1.0)), (RAY, 5, dict(bias=1.0)), (ACTION, 9, dict(bias=1.0)),
                              (CONTACT, d[-3], dict(bias=1.0)), (RAY, 0, dict(bias=1.0)), (ACTION, 1, dict(bias=1.0)), (ANGULAR, d[-1], dict(bias=1.0))])
    want = [ref.DISABLED] + [ref.SKIPPED] * 5 + [ref.SOURCE_OFF] * 5 + [ref.OBSERVED]
    rays = np.array([down_ray(world, d[0]), down_ray(world, d[1])], dtype=wire.ray_sensor_dtype)
    idle = wire.actuator_list([wire.actuator(1, d[0], 0, flags=wire.ACTUATOR_DISABLED), wire.actuator(1, d[1], 2, flags=wire.ACTUATOR_DISABLED)])
    with hip.Solver(0) as s:
        s.world_set_observers(quiet, channels)
        s.world_set_observation_report(BOTH)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(1, channels)
        step_both(s, params, ref_world)
        vector, states, counts, _ = expect(s, ref_world, quiet, history, "every source off")
        assert states["status"].tolist() == want and counts.tolist() == [1, 1, 5, 5]
        assert not vector[:-1].any() and vector[-1] != 0 and not states["raw"][:-1].any()
        # lists set, their flags still off: beyond the ray count and the action channels is SKIPPED, inside is SOURCE_OFF
        s.world_set_ray_sensors(rays)
        s.world_set_actuators(idle, 4)
        actions = np.array([0.5, -0.25, 0.125, 2.0], dtype=F)
        s.world_set_actions(actions)
        step_both(s, params, ref_world)
        _, states, counts, _ = expect(s, ref_world, quiet, history, "lists set", rays=2, actions=actions, action_channels=4)
        want[6], want[7], want[10] = ref.SKIPPED, ref.SKIPPED, ref.OBSERVED
        assert states["status"].tolist() == want and counts.tolist() == [2, 1, 7, 2]
        # each flag on: OBSERVED in the next step
        s.world_set_report(wire.REPORT_BODY_SUMS)
        step_both(s, params, ref_world)
        _, states, _, _ = expect(s, ref_world, quiet, history, "sums on", sums=True, rays=2, actions=actions, action_channels=4)
        want[8] = ref.OBSERVED
        assert states["status"].tolist() == want
        s.world_set_ray_report(wire.RAY_REPORT_RANGES)
        step_both(s, params, ref_world)
        vector, states, counts, _ = expect(s, ref_world, quiet, history, "ranges on", sums=True, ranges=True, rays=2, actions=actions, action_channels=4)
        want[9] = ref.OBSERVED
        assert states["status"].tolist() == want and counts.tolist() == [4, 1, 7, 0] and states["raw"][9][0] > 0 and states["value"][10][0] == F(0.75)
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "the idle actuators and the reports change nothing")
        # a smaller upload: the list is kept, targets beyond the new capacities are SKIPPED
        small = synthetic.pyramid_world(3)
        upload(s, small)
        small_ref = world_chain.copy_world(small)
        small_params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
        step_both(s, small_params, small_ref)
        _, states, counts, _ = expect(s, small_ref, quiet, ref.History(1, channels), "a smaller world", sums=True, ranges=True, rays=2, actions=actions, action_channels=4)
        outside = [i for i, o in enumerate(quiet) if int(o["kind"]) in (LINEAR, ROTATION, CONTACT, ANGULAR) and int(o["target"]) >= len(small["bodies"])]
        assert len(outside) >= 3 and (states["status"][outside] == ref.SKIPPED).all() and (states["status"][[2, 4]] == ref.SKIPPED).all()


def test_sizes():
    """A base-45 pyramid (1,036 body slots): 1, 63, 64, 65, 257, 1,024 and S2AMD_MAX_OBSERVERS observers of kinds 1-5 with random frames
    -- across the wave, the workgroup and 64 workgroups; the last observer writes the last channel; then channels = 1."""
    world = synthetic.pyramid_world(45)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    live = np.flatnonzero(world["bodies"]["type"] != wire.BODY_FREE)
    assert len(world["bodies"]) > 1024
    rng = np.random.RandomState(13)
    with hip.Solver(0) as s:
        s.world_set_observation_report(BOTH)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        for count in (1, 63, 64, 65, 257, 1024, wire.MAX_OBSERVERS):
            kinds = rng.randint(1, 6, size=count)
            kinds[-1] = LINEAR
            starts = np.concatenate([[0], np.cumsum([wire.OBSERVER_WIDTH[int(k)] for k in kinds])])
            channels = int(starts[-1])
            observers = np.zeros(count, dtype=wire.observer_dtype)
            observers["kind"], observers["target"], observers["channel"] = kinds, live[rng.randint(len(live), size=count)], starts[:-1]
            observers["frame"] = np.where(rng.rand(count) < 0.5, -1, live[rng.randint(len(live), size=count)])
            observers["flags"] = np.where(rng.rand(count) < 0.5, 0, RELATIVE)
            observers["gain"], observers["bias"] = rng.uniform(-2.0, 2.0, count), rng.uniform(-0.1, 0.1, count)
            observers["lower"], observers["upper"], observers["local"] = -4.0, 4.0, rng.uniform(-1.0, 1.0, (count, 2))
            assert observers["channel"][-1] + 2 == channels and ref.valid(observers, channels, 2) == -1
            s.world_set_observers(observers, channels, 2)
            history = ref.History(2, channels)
            for step in range(2 if count < wire.MAX_OBSERVERS else 1):
                step_both(s, params, ref_world)
                vector, states, counts, _ = expect(s, ref_world, observers, history, "%d observers" % count)
            assert counts.tolist() == [count, 0, 0, 0] and vector[-2:].tobytes() == states["value"][-1].tobytes()
        one = wire.observer_list([wire.observer(ANGLE, live[7], 0, frame=live[3], bias=0.5)])
        s.world_set_observers(one, 1, 3)
        step_both(s, params, ref_world)
        expect(s, ref_world, one, ref.History(3, 1), "channels = 1")
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "the pyramid")


def three_ways(s, shape):
    """The host getter, the waiting export and the enqueued export + wait, the exports into an s2amd_device_alloc buffer"""
    n = int(np.prod(shape))
    host = s.world_observations()
    buf = s.device_alloc(4 * n)
    try:
        s.device_write(buf, np.full(n, -7.0, dtype=F))
        s.world_export_observations(buf, n)
        waited = s.device_read(buf, shape, np.float32)
        s.device_write(buf, np.full(n, -7.0, dtype=F))
        s.world_export_observations_async(buf, n, slot=3)
        s.export_wait(3)
        enqueued = s.device_read(buf, shape, np.float32)
    finally:
        s.device_free(buf)
    assert host.tobytes() == waited.tobytes() == enqueued.tobytes()
    return host


@pytest.mark.parametrize("frames", [1, 2, 3, 4])
def test_history(frames):
    """ragdoll0 over 6 steps, newest first: every frame equal after the first step; a re-base by upload, by list replacement and by the
    flags off and on; a step with the flags at 0 in between does not advance the history; the three ways out give the same bytes."""
    params, world = golden("ragdoll0_PGS_NGS_Block")
    d = slots_of(world)["dynamic"]
    observers, channels = packed([(POINT, d[3], dict(frame=d[0])), (ANGULAR, d[4], {}), (LINEAR, d[6], dict(gain=0.5))])
    channels += 1  # one channel no observer covers
    with hip.Solver(0) as s:
        s.world_set_observers(observers, channels, frames)
        s.world_set_observation_report(VECTOR)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(frames, channels)
        seen = []
        for step in range(6):
            step_both(s, params, ref_world)
            vector, _, _, want = expect(s, ref_world, observers, history, "frames %d step %d" % (frames, step), states=False)
            assert three_ways(s, (frames, channels)).tobytes() == want.tobytes()
            seen.insert(0, vector)
            assert all(want[k].tobytes() == seen[min(k, len(seen) - 1)].tobytes() for k in range(frames)) and not want[:, -1].any()
            assert len({v.tobytes() for v in seen}) == len(seen)  # the ragdoll moves: every step's vector is another
        # a step with the flags at 0 is none ...
        s.world_set_observation_report(0)
        step_both(s, params, ref_world)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_observations()
        # ... and turning them on again re-bases
        s.world_set_observation_report(VECTOR)
        history.rebase()
        for step in range(2):
            step_both(s, params, ref_world)
            vector, _, _, want = expect(s, ref_world, observers, history, "frames %d, flags on again, step %d" % (frames, step), states=False)
            assert step > 0 or all(row.tobytes() == vector.tobytes() for row in want)
        # by list replacement
        s.world_set_observers(observers[::-1].copy(), channels, frames)
        history = ref.History(frames, channels)
        for step in range(frames + 1):
            step_both(s, params, ref_world)
            expect(s, ref_world, observers[::-1], history, "frames %d, list replaced, step %d" % (frames, step), states=False)
            three_ways(s, (frames, channels))
        # by upload: the list and the sizes hold
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history.rebase()
        for step in range(2):
            step_both(s, params, ref_world)
            vector, _, _, want = expect(s, ref_world, observers[::-1], history, "frames %d, uploaded, step %d" % (frames, step), states=False)
            assert step > 0 or all(row.tobytes() == vector.tobytes() for row in want)


def test_closed_loop_on_the_device():
    """Observation to action without the host: the vector is exported into a device buffer, its first four channels are imported as the
    actions, the world steps, 8 times.  The chain equals the one in which the statement's vector is fed to the actuators' statement, and
    the ACTION observers see the action this step's actuator pass read: the vector's own channel of the step before."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    at = slots_of(world)
    d, rev = at["dynamic"], at["revolute"]
    observers, channels = packed([(REV_ANGLE, rev[1], dict(gain=-0.5)), (REV_SPEED, rev[0], dict(gain=-0.5, bias=0.5, lower=-2.0, upper=2.0)),
                                  (LINEAR, d[1], dict(frame=d[0], gain=5.0, bias=1.0, lower=-8.0, upper=8.0)), (ACTION, 0, {}), (ACTION, 2, {})])
    actuators = wire.actuator_list([wire.actuator(6, rev[0], 0, kp=4.0, max_speed=3.0), wire.actuator(5, rev[1], 1, gain=2.0), wire.actuator(1, d[0], 2, gain=6.0)])
    with hip.Solver(0) as s:
        s.world_set_actuators(actuators, 4)
        s.world_set_observers(observers, channels)
        s.world_set_observation_report(BOTH)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(1, channels)
        buf = s.device_alloc(4 * channels)
        try:
            actions = np.zeros(4, dtype=F)
            for step in range(8):
                if step > 0:
                    s.world_export_observations_async(buf, channels, slot=1)
                    s.world_import_actions(buf, 4)  # (the same stream: behind the export)
                    actions = vector[:4].copy()
                actuator_ref.apply(ref_world, actuators, actions)
                step_both(s, params, ref_world)
                vector, states, counts, _ = expect(s, ref_world, observers, history, "closed loop step %d" % step, actions=actions, action_channels=4)
                assert counts.tolist() == [5, 0, 0, 0] and vector[4] == actions[0] and vector[5] == actions[2]
                world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "closed loop step %d" % step)
            assert actions.all() and s.world_actuator_counts().tolist() == [3, 0, 0, 0]
        finally:
            s.device_free(buf)


def test_untouched():
    """A list set and the flags at 0: the step enqueues what a solver with no list enqueues, and the chain is the oracle's.  The flags on:
    the downloaded world equals, byte for byte, that of a solver without observers."""
    params, world = golden("mixed24_PGS")
    observers, channels = every_kind(world)
    with hip.Solver(0) as never, hip.Solver(0) as idle, hip.Solver(0) as on:
        idle.world_set_observers(observers, channels, 4)
        on.world_set_observers(observers, channels, 4)
        on.world_set_observation_report(BOTH)
        for s in (never, idle, on):
            upload(s, world)
        ref_world = world_chain.copy_world(world)
        for step in range(6):
            step_both(never, params, ref_world)
            idle.world_step(params)
            on.world_step(params)
            a, b, c = never.stats(), idle.stats(), on.stats()
            assert (a["kernelLaunches"], a["solveLaunches"], a["structureBuilds"]) == (b["kernelLaunches"], b["solveLaunches"], b["structureBuilds"]), step
            assert (a["solveLaunches"], a["structureBuilds"]) == (c["solveLaunches"], c["structureBuilds"]), step
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                idle.world_observations()
        got = download(never, world)[0]
        world_chain.assert_device_equals_oracle(got, ref_world, "no list")
        assert_same_world(download(idle, world)[0], got, "a list and no flags")
        assert_same_world(download(on, world)[0], got, "the report on")
        assert on.world_observer_counts().sum() == len(observers)


def test_errors():
    params, world = golden("mixed24_PGS")
    good, channels = every_kind(world)

    def bad_lists():
        for name, value in (("kind", 0), ("kind", 12), ("target", -1), ("frame", -2), ("channel", -1), ("channel", channels - 1), ("flags", 4), ("flags", -1),
                            ("gain", np.nan), ("gain", np.inf), ("bias", np.nan), ("bias", -np.inf), ("lower", np.nan), ("upper", np.nan), ("lower", 11.0)):
            wrong = good.copy()
            wrong[name][3] = value  # the linear velocity: width 2, bounds -1 .. 1
            yield "%s = %r" % (name, value), wrong
        for name, index, value in (("local", 0, np.nan), ("local", 1, np.inf), ("reserved", 0, 1), ("reserved", 4, -1)):
            wrong = good.copy()
            wrong[name][0][index] = value
            yield name, wrong
        for record in (5, 8, 9, 10):
            wrong = good.copy()
            wrong["frame"][record] = 0  # kinds 6-11 take no frame
            yield "frame on kind %d" % wrong["kind"][record], wrong
        for record, channel in ((1, 1), (4, 6), (10, 0)):
            wrong = good.copy()
            wrong["channel"][record] = channel  # onto another observer's range
            yield "overlap", wrong

    with hip.Solver(0) as s:
        L, h = s._L, s._h
        assert s.world_observations().shape == (0, 0) and len(s.world_observer_states()) == 0 and s.world_observer_counts().tolist() == [0, 0, 0, 0]
        s.world_set_observers(good, channels, 2)  # accepted before any world
        s.world_set_observation_report(BOTH)
        refuses(s, E_STATE, ("world_observations", "world_observer_states", "world_observer_counts"))  # no resident world
        upload(s, world)
        buf = s.device_alloc(4 * 2 * channels)
        try:
            for call in (s.world_observations, s.world_observer_states, s.world_observer_counts, lambda: s.world_export_observations(buf, 2 * channels),
                         lambda: s.world_export_observations_async(buf, 2 * channels)):
                with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                    call()  # no step since the upload
            ref_world = world_chain.copy_world(world)
            history = ref.History(2, channels)
            step_both(s, params, ref_world)
            expect(s, ref_world, good, history, "before the refusals")
            # per call
            many = np.zeros(wire.MAX_OBSERVERS + 1, dtype=wire.observer_dtype)
            many[:] = good[4]
            assert L.s2amd_world_set_observers(h, wire.as_ptr(good), -1, channels, 2) == E_INVALID and L.s2amd_world_set_observers(h, None, 2, channels, 2) == E_INVALID
            assert L.s2amd_world_set_observers(h, wire.as_ptr(many), len(many), channels, 2) == E_INVALID
            for ch, fr in ((0, 2), (wire.MAX_OBSERVATION_CHANNELS + 1, 2), (channels, 0), (channels, wire.MAX_OBSERVATION_FRAMES + 1), (channels - 1, 2)):
                assert L.s2amd_world_set_observers(h, wire.as_ptr(good), len(good), ch, fr) == E_INVALID
            assert L.s2amd_world_set_observation_report(h, 4) == E_INVALID
            # per record
            for what, wrong in bad_lists():
                assert ref.valid(wrong, channels, 2) >= 0, what
                with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                    s.world_set_observers(wrong, channels, 2)
            # a refused list leaves the previous answers in place
            assert s.world_observations().tobytes() == history.rows.tobytes()
            # the getters
            count = ctypes.c_int32(-7)
            n = 2 * channels
            out = np.zeros(n, dtype=F)
            assert L.s2amd_world_observations(h, wire.as_ptr(out), n - 1, ctypes.byref(count)) == E_CAPACITY and count.value == n and not out.any()
            assert L.s2amd_world_observations(h, wire.as_ptr(out), -1, ctypes.byref(count)) == E_INVALID and L.s2amd_world_observations(h, wire.as_ptr(out), n, None) == E_INVALID
            states = np.zeros(len(good), dtype=wire.observer_state_dtype)
            count.value = -7
            assert L.s2amd_world_observer_states(h, wire.as_ptr(states), len(good) - 1, ctypes.byref(count)) == E_CAPACITY and count.value == len(good)
            assert states.tobytes() == bytes(states.nbytes) and L.s2amd_world_observer_counts(h, None) == E_INVALID
            assert L.s2amd_world_export_observations(h, ctypes.c_void_p(buf), n - 1) == E_CAPACITY and L.s2amd_world_export_observations(h, None, n) == E_INVALID
            assert L.s2amd_world_export_observations_async(h, ctypes.c_void_p(buf), n - 1, 0) == E_CAPACITY
            assert L.s2amd_world_export_observations_async(h, ctypes.c_void_p(buf), n, 4) == E_INVALID and L.s2amd_world_export_observations_async(h, ctypes.c_void_p(buf), n, -1) == E_INVALID
            # the next step goes on from the history that stood
            step_both(s, params, ref_world)
            expect(s, ref_world, good, history, "after the refusals")
            # a getter whose flag was not set before the last step
            s.world_set_observation_report(STATES)
            step_both(s, params, ref_world)
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_observations()
            assert len(s.world_observer_states()) == len(good)
            s.world_set_observers(good, channels, 2)
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_observer_states()  # no step since the list was set
        finally:
            s.device_free(buf)


def test_all_nine_facilities_on_together():
    """mixed24 with the contact, joint, shape and body reports, the step metrics, sensors, rays, grids and the observers on at once.  The
    five older reports with a numpy statement equal it; the sensor, ray and grid getters equal those of a second solver that never heard
    of observers, the grid report also its own structure and point-probe check; and the observers equal their statement, kinds 9 and 10
    reading the two reports in front of them."""
    params, world = golden("mixed24_PGS")
    observers, channels = every_kind(world)
    at = slots_of(world)
    d = at["dynamic"]
    rays = np.array([down_ray(world, d[0]), down_ray(world, d[3])], dtype=wire.ray_sensor_dtype)
    centre = world["bodies"]["position"][d[0]]
    grids = np.array([gw.make_grid((float(centre[0]) - 2.0, float(centre[1]) - 2.0), 0.0, 0.5, 8, 8)], dtype=wire.grid_sensor_dtype)
    sensors = np.array([sw.make_sensor(sw.box_vertices(3.0, 3.0), 0.0, position=(float(centre[0]), float(centre[1])))], dtype=wire.sensor_dtype)
    thresholds = (F(0.2), F(F(0.2) * F(3.4906585)), F(3) * F(params.dt))
    with hip.Solver(0) as s, hip.Solver(0) as twin:
        for k in (s, twin):
            k.world_set_report(wire.REPORT_ALL)
            k.world_set_joint_report(wire.JOINT_REPORT_ALL)
            k.world_set_shape_report(wire.SHAPE_REPORT_ALL)
            k.world_set_body_report(wire.BODY_REPORT_STATES | wire.BODY_REPORT_REST | wire.BODY_REPORT_ISLANDS)
            k.world_set_rest_thresholds(*thresholds)
            k.world_set_metrics(wire.METRICS_ALL, 4)
            k.world_set_sensors(sensors)
            k.world_set_sensor_report(wire.SENSOR_REPORT_ALL)
            k.world_set_ray_sensors(rays)
            k.world_set_ray_report(wire.RAY_REPORT_ALL)
            k.world_set_grid_sensors(grids)
            k.world_set_grid_report(wire.GRID_REPORT_ALL)
        s.world_set_observers(observers, channels, 2)
        s.world_set_observation_report(BOTH)
        upload(s, world), upload(twin, world)
        ref_world = world_chain.copy_world(world)
        history = ref.History(2, channels)
        prev_touch = contact_report_ref.before_of(ref_world["contacts"])
        prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
        state = body_report_ref.new_state(ref_world)
        for step in range(4):
            step_both(s, params, ref_world)
            twin.world_step(params)
            what = "all nine, step %d" % step
            _, states, _, _ = expect(s, ref_world, observers, history, what, sums=True, ranges=True, rays=2)
            assert states["status"].tolist() == [ref.OBSERVED] * 10 + [ref.SOURCE_OFF]  # (no actuator list here)
            assert_metrics_equal_reference(s, ref_world, params, wire.METRICS_ALL, step, what)
            want_began, want_ended = contact_report_ref.events(prev_touch, ref_world)
            began, ended = s.world_touch_events()
            assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
            want_touching = contact_report_ref.touching(ref_world)
            assert s.world_touching(expected=max(len(want_touching), 1)).tobytes() == want_touching.tobytes(), what
            assert s.world_body_sums().tobytes() == contact_report_ref.body_sums(ref_world).tobytes(), what
            want_states = joint_report_ref.states(ref_world)
            assert s.world_joint_states(expected=max(len(want_states), 1)).tobytes() == want_states.tobytes(), what
            want_began, want_ended = joint_report_ref.events(prev_limits, ref_world)
            began, ended = s.world_joint_limit_events()
            assert began.tolist() == want_began.tolist() and ended.tolist() == want_ended.tolist(), what
            assert s.world_body_joint_sums().tobytes() == joint_report_ref.body_sums(ref_world).tobytes(), what
            assert s.world_joint_summary().tobytes() == joint_report_ref.summary(ref_world).tobytes(), what
            assert s.world_shape_draws(expected=64).tobytes() == shape_report_ref.draws(ref_world, None).tobytes(), what
            assert s.world_shape_summary().tobytes() == shape_report_ref.summary(ref_world, None).tobytes(), what
            body_step = body_report_ref.advance(state, ref_world, thresholds, params.dt)
            island, island_states = body_report_ref.islands(ref_world, body_step)
            assert s.world_islands(expected=max(len(island_states), 1)).tobytes() == island_states.tobytes(), what
            want_bodies = body_report_ref.states(ref_world, body_step, False, island, island_states)
            assert s.world_body_states(expected=max(len(want_bodies), 1)).tobytes() == want_bodies.tobytes(), what
            assert s.world_body_summary().tobytes() == body_report_ref.summary(ref_world, body_step, island_states).tobytes(), what
            prev_touch = contact_report_ref.touching_mask(ref_world)
            prev_limits = joint_report_ref.limit_mask(ref_world["joints"])
            for a, b in zip(s.world_sensor_inside(), twin.world_sensor_inside()):
                assert a.tobytes() == b.tobytes(), what
            assert s.world_sensor_states().tobytes() == twin.world_sensor_states().tobytes(), what
            assert s.world_ray_states().tobytes() == twin.world_ray_states().tobytes() and s.world_ray_ranges().tobytes() == twin.world_ray_ranges().tobytes(), what
            assert s.world_ray_events().tobytes() == twin.world_ray_events().tobytes(), what
            got = assert_grid_report(s, world, grids, what)
            for a, b in zip(got, (twin.world_grid_categories(), twin.world_grid_shapes(), twin.world_grid_occupancy(), twin.world_grid_states())):
                assert a.tobytes() == b.tobytes(), what
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "all nine")
