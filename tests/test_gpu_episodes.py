"""Episodes on the resident world (s2amd_world_set_episodes / _set_episode_report / _episode_rewards / _episode_flags /
_export_episode_step(_async) / _episode_states / _episode_rule_states / _episode_events / _episode_counts;
solver2d_amd/csrc/episodes.hip) against their statement (tests/episode_ref.py: numpy float32), byte for byte.  The pass runs behind the
observers', so the statement is applied to s.world_observations() of the same step (tests/test_gpu_observers.py pins that getter).  The
worlds are the committed tests/golden/world_mixed24_PGS and world_ragdoll0_PGS_NGS_Block; many agents read the same few channels with
different bounds, so the sizes need no large world.  Where a test must decide a step's numbers it drives an ACTION observer through
s2amd_world_set_actions under a disabled actuator list, which the world never sees."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import episode_ref as ref, grid_report_world as gw, sensor_report_world as sw, world_chain
from tests.resident import (E_CAPACITY, E_INVALID, E_STATE, assert_same_bytes, down_ray, download, every_kind, motorised, packed, refuses, slots_of,
                            step_both, upload)
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

F = np.float32
ALL = wire.EPISODE_REPORT_ALL
STEP, STATES, RULE_STATES, EVENTS = wire.EPISODE_REPORT_STEP, wire.EPISODE_REPORT_STATES, wire.EPISODE_REPORT_RULE_STATES, wire.EPISODE_REPORT_EVENTS
VALUE, TEST, TERMINATE, TRUNCATE = ref.REWARD_VALUE, ref.REWARD_TEST, ref.TERMINATE, ref.TRUNCATE
OUTSIDE, OFF = wire.EPISODE_RULE_OUTSIDE, wire.EPISODE_RULE_DISABLED
POINT, ROTATION, ANGLE, LINEAR, ANGULAR, REV_ANGLE, REV_SPEED, REV_IMPULSE, CONTACT, RAY, ACTION = range(1, 12)
GETTERS = ("world_episode_rewards", "world_episode_flags", "world_episode_states", "world_episode_rule_states", "world_episode_events", "world_episode_counts")
rule = wire.episode_rule


def expect(s, acc, rules, agents, limits, what, obs_on=True, dims=None):
    """The statement on this step's s.world_observations() (None with the observation report off) against every getter -> its dict"""
    obs = s.world_observations() if obs_on else None
    want = ref.step(acc, obs, rules, agents, limits, dims)
    assert_same_bytes(s.world_episode_rewards(), want["rewards"], what + ": rewards")
    assert_same_bytes(s.world_episode_flags(), want["flags"], what + ": flags")
    assert_same_bytes(s.world_episode_states(), want["states"], what + ": agent states")
    assert_same_bytes(s.world_episode_rule_states(), want["rule_states"], what + ": rule states")
    assert_same_bytes(s.world_episode_events(), want["events"], what + ": events")
    assert s.world_episode_counts().tolist() == want["counts"].tolist(), what
    return want


def ragdoll_observers(frames_of=None):
    """Seven channels of the falling ragdoll: two angular velocities, a linear velocity, a point in the torso's frame, an angle"""
    params, world = golden("ragdoll0_PGS_NGS_Block")
    d = slots_of(world)["dynamic"]
    observers, channels = packed([(ANGULAR, d[4], {}), (ANGULAR, d[6], dict(gain=0.5)), (LINEAR, d[5], {}), (POINT, d[3], dict(frame=d[0])), (ANGLE, d[2], {})])
    return params, world, observers, channels


def driven(s, world, channels=4):
    """A disabled actuator list of `channels` action channels and an ACTION observer on each: channel k of the vector is action k"""
    d = slots_of(world)["dynamic"]
    s.world_set_actuators(wire.actuator_list([wire.actuator(1, d[0], 0, flags=wire.ACTUATOR_DISABLED)]), channels)
    observers, n = packed([(ACTION, k, {}) for k in range(channels)])
    s.world_set_observers(observers, n)
    s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
    return n


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
def test_every_kind_shape_and_flag_once(fast):
    """mixed24_PGS with its motors on, kinds 1-8 of the observers over two frames: every rule kind x shape x {plain, OUTSIDE, DIFFERENCE,
    DIFFERENCE | OUTSIDE} and a DISABLED rule over five agents, 3 steps.  The tolerance-mode library steps other bits; the pass on its
    own observations is the same bits."""
    params, world = golden("mixed24_PGS")
    world = motorised(world)
    at = slots_of(world)
    d, rev = at["dynamic"], at["revolute"]
    observers, channels = packed([(POINT, d[0], dict(frame=d[1])), (ROTATION, d[2], {}), (ANGLE, d[4], {}), (LINEAR, d[6], {}), (ANGULAR, d[8], {}),
                                  (REV_ANGLE, rev[0], {}), (REV_SPEED, rev[1], {}), (REV_IMPULSE, rev[0], dict(gain=10.0))])
    listed = []
    for kind in (VALUE, TEST, TERMINATE, TRUNCATE):
        for shape in (ref.LINEAR, ref.ABS, ref.SQUARE):
            for k, (flags, minus) in enumerate(((0, None), (OUTSIDE, None), (0, (len(listed) % channels, 1)), (OUTSIDE, ((len(listed) + 3) % channels, 1)))):
                n = len(listed)
                listed.append(rule(kind, n % 5, n % channels, minus=minus, shape=shape, gain=0.75, bias=0.0 if kind >= TERMINATE else -0.125,
                                   lower=-0.25 if k % 2 else 0.01, upper=0.5, flags=flags))
    listed.append(rule(VALUE, 4, 0, bias=3.0, flags=OFF))
    rules = wire.episode_rule_list(listed)
    assert ref.valid(rules, 5) == -1 and len(rules) == 49
    limits = np.array([0, 2, 0, 3, 0], dtype=np.int32)
    with hip.Solver(0, fast=fast) as s:
        s.world_set_observers(observers, channels, 2)
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        s.world_set_episodes(rules, 5, limits)
        s.world_set_episode_report(ALL)
        upload(s, world)
        acc = ref.Accounting(5)
        fired = []
        for step in range(3):
            s.world_step(params)
            want = expect(s, acc, rules, 5, limits, "mixed24 step %d" % step)
            assert want["counts"][:4].tolist() == [48, 1, 0, 0]
            fired.append(want["rule_states"]["fired"].copy())
        # nothing is trivial: rules fired and rules did not, the differences are non-zero behind the first step, rewards differ per agent
        ending = rules["kind"] >= TERMINATE
        assert fired[-1][ending].any() and not fired[-1][ending].all() and not fired[-1][~ending].any()
        differences = (rules["flags"] & wire.EPISODE_RULE_DIFFERENCE) != 0
        assert (want["rule_states"]["x"][differences] != 0).any() and len(set(want["rewards"].tolist())) == 5


def test_sizes():
    """1, 63, 64, 65, 256, 257, 1,000 and S2AMD_MAX_EPISODE_AGENTS agents on the ragdoll's seven channels -- across the wave, the
    workgroup and the events kernel's 64 chunks --, 0 to 5 rules per agent with agents without any, the list shuffled so that one agent's
    rules are not adjacent, and one agent carrying 300 rules, a run that spans workgroups of the rules kernel."""
    params, world, observers, channels = ragdoll_observers()
    rng = np.random.RandomState(29)
    with hip.Solver(0) as s:
        s.world_set_observers(observers, channels, 2)
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        s.world_set_episode_report(ALL)
        upload(s, world)
        s.world_step(params)
        for agents in (1, 63, 64, 65, 256, 257, 1000, wire.MAX_EPISODE_AGENTS):
            per_agent = rng.randint(0, 6, size=agents)
            heavy = agents // 2
            per_agent[heavy] = 300
            owner = rng.permutation(np.repeat(np.arange(agents), per_agent))
            n = len(owner)
            rules = np.zeros(n, dtype=wire.episode_rule_dtype)
            rules["kind"], rules["agent"], rules["shape"] = rng.randint(1, 5, size=n), owner, rng.randint(0, 3, size=n)
            rules["channelA"], rules["frameA"] = rng.randint(-1, channels, size=n), rng.randint(0, 2, size=n)
            difference = (rng.rand(n) < 0.4) & (rules["channelA"] >= 0)
            rules["channelB"], rules["frameB"] = np.where(difference, rng.randint(0, channels, size=n), 0), np.where(difference, 1, 0)
            rules["flags"] = np.where(difference, wire.EPISODE_RULE_DIFFERENCE, 0) | np.where(rng.rand(n) < 0.3, OUTSIDE, 0) | np.where(rng.rand(n) < 0.05, OFF, 0)
            rules["gain"], rules["bias"] = rng.uniform(-2.0, 2.0, n), np.where(rules["kind"] >= TERMINATE, 0.0, rng.uniform(-0.5, 0.5, n))
            rules["lower"] = rng.uniform(-3.0, 0.5, n)
            rules["upper"] = rules["lower"] + rng.uniform(0.0, 3.0, n).astype(F)
            limits = rng.randint(0, 4, size=agents).astype(np.int32)
            assert ref.valid(rules, agents, limits) == -1 and (agents < 63 or (per_agent == 0).any())
            s.world_set_episodes(rules, agents, limits)
            acc = ref.Accounting(agents)
            for step in range(2 if agents <= 1000 else 1):
                s.world_step(params)
                want = expect(s, acc, rules, agents, limits, "%d agents, step %d" % (agents, step), dims=(2, channels))
            assert want["counts"][:4].sum() == n and want["counts"][0] > n // 2
            assert agents < 64 or (0 < want["counts"][4] < agents and len(want["events"]) == want["counts"][4] and (np.diff(want["events"]["agent"]) > 0).all())


def test_the_sum_takes_the_list_order():
    """1e8 + 1 - 1e8 is +0 in that order and 1 with the big terms first; the device sums in list order whatever lies between."""
    params, world = golden("ragdoll0_PGS_NGS_Block")
    triple = [rule(VALUE, 1, bias=1e8), rule(VALUE, 1, bias=1.0), rule(VALUE, 1, bias=-1e8)]
    between = [rule(VALUE, 0, bias=2.0), rule(VALUE, 2, bias=-4.0)]
    with hip.Solver(0) as s:
        s.world_set_episode_report(ALL)
        upload(s, world)
        for order, bits in (((0, 1, 2), 0), ((0, 2, 1), F(1.0).view(np.uint32)), ((2, 1, 0), 0), ((2, 0, 1), F(1.0).view(np.uint32))):
            rules = wire.episode_rule_list([triple[order[0]], between[0], triple[order[1]], between[1], triple[order[2]]])
            s.world_set_episodes(rules, 3)
            s.world_step(params)
            want = expect(s, ref.Accounting(3), rules, 3, None, "order %s" % (order,), obs_on=False)
            got = s.world_episode_rewards()
            assert got.view(np.uint32).tolist() == [F(2.0).view(np.uint32), bits, F(-4.0).view(np.uint32)] and want["counts"][:4].tolist() == [5, 0, 0, 0]


def test_termination_time_limits_and_the_restart():
    """Eight steps on mixed24 with the vector's channels driven from the host: time limits of 1, 3 and 0; a termination and the time limit
    in the same step; `rule`, `episodes`, lastReturn and lastLength; the restart in the step after; the events ascending; the counts."""
    params, world = golden("mixed24_PGS")
    rules = wire.episode_rule_list([rule(VALUE, 1, 2, gain=0.5), rule(TERMINATE, 1, 0, gain=10.0, lower=1.0), rule(TRUNCATE, 2, 1, gain=-1.0, lower=1.0),
                                    rule(VALUE, 2, 2, shape=ref.SQUARE), rule(TERMINATE, 2, 0, gain=0.25, lower=1.0), rule(TRUNCATE, 1, 0, gain=0.0, lower=1.0)])
    limits = np.array([1, 3, 0, 3], dtype=np.int32)
    script = np.zeros((8, 4), dtype=F)
    script[:, 2] = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    script[2, 0] = script[4, 0] = 1.0  # agent 1 terminates in its third step, beside its time limit, and again two steps on
    script[1, 1] = script[4, 1] = script[5, 1] = 2.0  # agent 2 is truncated by its rule, terminated by channel 0 in step 2, both in step 4
    with hip.Solver(0) as s:
        channels = driven(s, world)
        s.world_set_episodes(rules, 4, limits)
        s.world_set_episode_report(ALL)
        upload(s, world)
        acc = ref.Accounting(4)
        seen = []
        for step in range(8):
            s.world_set_actions(script[step])
            s.world_step(params)
            assert s.world_observations()[0].tobytes() == script[step].tobytes()
            seen.append(expect(s, acc, rules, 4, limits, "step %d" % step))
        flags = np.array([o["flags"] for o in seen])
        assert flags[:, 0].tolist() == [6] * 8 and flags[:, 3].tolist() == [0, 0, 6, 0, 0, 6, 0, 0]
        assert flags[:, 1].tolist() == [0, 0, 7, 0, 3, 0, 0, 6] and flags[:, 2].tolist() == [0, 2, 1, 0, 3, 2, 0, 0]
        states = [o["states"] for o in seen]
        assert [int(st["rule"][1]) for st in states] == [-1, -1, 1, -1, 1, -1, -1, -1] and [int(st["rule"][2]) for st in states] == [-1, 2, 4, -1, 2, 2, -1, -1]
        assert [int(st["episodeLength"][1]) for st in states] == [1, 2, 3, 1, 2, 1, 2, 3] and [int(st["episodes"][1]) for st in states] == [0, 0, 1, 1, 2, 2, 2, 3]
        assert [float(st["reward"][1]) for st in states] == [0.25, 0.5, 10.75, 1.0, 11.25, 1.5, 1.75, 2.0]
        assert [float(st["lastReturn"][1]) for st in states] == [0, 0, 11.5, 11.5, 12.25, 12.25, 12.25, 5.25] and states[-1]["lastLength"].tolist() == [1, 3, 1, 3]
        assert [o["events"]["agent"].tolist() for o in seen] == [[0], [0, 2], [0, 1, 2, 3], [0], [0, 1, 2], [0, 2, 3], [0], [0, 1]]
        assert seen[2]["events"][1].tolist() == (1, 7, 3, 11.5) and seen[4]["counts"].tolist() == [6, 0, 0, 0, 3, 2, 3, 1]


def test_differences_over_frames_and_the_rebases():
    """The ragdoll with frames = 3 and DIFFERENCE rules against frames 1 and 2: +0 at the first step after each re-base of the observers
    (an upload, the observer list replaced, the observation flags from 0 to non-zero) and non-zero behind it; the episodes' own re-bases
    (an upload, the rule list replaced, the episode flags from 0 to non-zero) zero the accounting; a step with the episode flags at 0
    reports nothing and counts nothing."""
    params, world, observers, channels = ragdoll_observers()
    rules = wire.episode_rule_list([rule(VALUE, 0, 0, minus=(0, 1)), rule(VALUE, 0, 2, minus=(2, 2), shape=ref.ABS, gain=4.0), rule(VALUE, 1, 3, frame=1, minus=(3, 2)),
                                    rule(TERMINATE, 1, 6, minus=(6, 1), gain=1.0, shape=ref.ABS, lower=1e-6), rule(VALUE, 1, 1)])
    limits = np.array([0, 4], dtype=np.int32)

    def run(s, acc, steps, what, first_is_flat):
        for step in range(steps):
            s.world_step(params)
            want = expect(s, acc, rules, 2, limits, "%s, step %d" % (what, step))
            x = want["rule_states"]["x"][:4]
            if step == 0 and first_is_flat:
                assert x.view(np.uint32).tolist() == [0, 0, 0, 0] and want["rule_states"]["fired"][3] == 0, what
            if step == 2:
                assert (x != 0).all() and want["rule_states"]["fired"][3] == 1, what
        return want

    with hip.Solver(0) as s:
        s.world_set_observers(observers, channels, 3)
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        s.world_set_episodes(rules, 2, limits)
        s.world_set_episode_report(ALL)
        upload(s, world)
        acc = ref.Accounting(2)
        want = run(s, acc, 4, "uploaded", True)
        assert want["states"]["episodes"].tolist() == [0, 3] and want["states"]["episodeLength"].tolist() == [4, 1]  # (agent 1 ends at every step that is not flat)
        # the episode flags at 0: the observers go on, the episodes do not; on again: re-based
        s.world_set_episode_report(0)
        s.world_step(params)
        refuses(s, E_STATE, GETTERS)
        s.world_set_episode_report(ALL)
        acc.rebase()
        want = run(s, acc, 1, "episode flags on again", False)
        assert want["states"]["episodeLength"].tolist() == [1, 1] and want["states"]["episodes"].tolist() == [0, 1] and (want["rule_states"]["x"][:4] != 0).all()
        # the observation flags off and on: SOURCE_OFF for the step between, then every frame equal
        s.world_set_observation_report(0)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "observation flags at 0", obs_on=False, dims=(3, channels))
        assert want["counts"][:4].tolist() == [0, 0, 0, 5] and want["states"]["episodeLength"].tolist() == [2, 1]
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        run(s, acc, 3, "observation flags on again", True)
        # the observer list replaced (the same list again): the history is re-based, the episodes go on
        s.world_set_observers(observers, channels, 3)
        want = run(s, acc, 3, "observer list replaced", True)
        assert want["states"]["episodeLength"][0] == 8
        # the rule list replaced: the accounting is re-based, the history goes on
        s.world_set_episodes(rules, 2, limits)
        acc.rebase()
        want = run(s, acc, 1, "rule list replaced", False)
        assert want["states"]["episodeLength"].tolist() == [1, 1] and want["states"]["lastLength"].tolist() == [0, 1]
        # an upload re-bases both; the lists hold
        upload(s, world)
        acc.rebase()
        run(s, acc, 3, "uploaded again", True)


def test_statuses():
    """The observation flags at 0: SOURCE_OFF, while rules without a source and the time limit still run; the observer list replaced by a
    narrower one with fewer frames: SKIPPED; no observer list: SOURCE_OFF whatever the channel; DISABLED before all of them."""
    params, world, observers, channels = ragdoll_observers()
    rules = wire.episode_rule_list([rule(VALUE, 0, 1, bias=1.0), rule(VALUE, 0, 6, bias=1.0), rule(VALUE, 0, 0, frame=1, bias=1.0), rule(VALUE, 1, 0, minus=(5, 0), bias=1.0),
                                    rule(TERMINATE, 1, 2, minus=(2, 1), flags=OUTSIDE), rule(VALUE, 1, bias=0.5), rule(TEST, 0, 99, gain=1.0, bias=1.0, flags=OFF),
                                    rule(TRUNCATE, 1, lower=0.0, upper=0.0, flags=OFF)])
    limits = np.array([2, 0], dtype=np.int32)
    with hip.Solver(0) as s:
        s.world_set_observers(observers, channels, 2)
        s.world_set_episodes(rules, 2, limits)
        s.world_set_episode_report(ALL)
        upload(s, world)
        acc = ref.Accounting(2)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "the observation report off", obs_on=False, dims=(2, channels))
        assert want["rule_states"]["status"].tolist() == [3, 3, 3, 3, 3, 0, 1, 1] and want["rewards"].tolist() == [0.0, 0.5] and want["flags"].tolist() == [0, 0]
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "the observation report off, step 2", obs_on=False, dims=(2, channels))
        assert want["flags"].tolist() == [6, 0] and want["states"]["episodeReturn"].tolist() == [0.0, 1.0]
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "the observation report on")
        assert want["rule_states"]["status"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and want["counts"][:4].tolist() == [6, 2, 0, 0]
        # narrower, and one frame: channels 5 and 6 and frame 1 are beyond it
        s.world_set_observers(observers[:3], 5, 1)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "a narrower observer list")
        assert want["rule_states"]["status"].tolist() == [0, 2, 2, 2, 2, 0, 1, 1] and want["counts"][:4].tolist() == [2, 2, 4, 0]
        s.world_set_observation_report(0)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "narrower and off", obs_on=False, dims=(1, 5))
        assert want["rule_states"]["status"].tolist() == [3, 2, 2, 2, 2, 0, 1, 1]
        # no list: nothing to be beyond
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        s.world_set_observers(observers[:0], 0, 0)
        s.world_step(params)
        want = expect(s, acc, rules, 2, limits, "no observer list", obs_on=False, dims=(0, 0))
        assert want["rule_states"]["status"].tolist() == [3, 3, 3, 3, 3, 0, 1, 1]


def test_a_nan_in_the_vector():
    """An ACTION observer on a channel set to NaN through s2amd_world_set_actions: it fires a TERMINATE | OUTSIDE rule and no plain one, and
    passes through REWARD_VALUE into the reward and the return."""
    params, world = golden("mixed24_PGS")
    rules = wire.episode_rule_list([rule(TERMINATE, 0, 1, gain=-1.0, lower=-1.0, upper=1.0, flags=OUTSIDE), rule(TERMINATE, 1, 1, lower=-1.0, upper=1.0),
                                    rule(VALUE, 2, 1, lower=-1.0, upper=1.0), rule(TEST, 1, 1, gain=1.0, bias=-1.0), rule(VALUE, 3, 0, gain=2.0)])
    with hip.Solver(0) as s:
        driven(s, world)
        s.world_set_episodes(rules, 4)
        s.world_set_episode_report(ALL)
        upload(s, world)
        acc = ref.Accounting(4)
        for step, value in enumerate((0.5, np.nan, 0.25)):
            s.world_set_actions(np.array([3.0, value, 0.0, 0.0], dtype=F))
            s.world_step(params)
            want = expect(s, acc, rules, 4, None, "step %d" % step)
            got = s.world_episode_states()
            if step == 1:
                assert want["flags"].tolist() == [1, 0, 0, 0] and np.isnan(got["reward"][2]) and np.isnan(got["episodeReturn"][2]) and got["reward"].tolist()[:2] == [-1.0, -1.0]
            else:
                assert want["flags"].tolist() == [0, 1, 0, 0] and got["reward"][2] == F(value) and got["reward"][3] == 6.0
        assert np.isnan(got["episodeReturn"][2]) and got["episodes"].tolist() == [1, 2, 0, 0]


def test_exports():
    """The waiting export and the enqueued export + wait into s2amd_device_alloc buffers equal the host getters; S2AMD_E_CAPACITY and the
    slot errors; with no list the enqueued export records its event and returns."""
    params, world, observers, channels = ragdoll_observers()
    agents = 300
    rules = wire.episode_rule_list([rule(VALUE, a, a % channels, gain=0.5 + a) for a in range(agents)] + [rule(TERMINATE, a, 0, shape=ref.ABS, lower=0.0) for a in range(0, agents, 3)])
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        rewards, flags = s.device_alloc(4 * agents), s.device_alloc(4 * agents)
        try:
            s.world_set_observers(observers, channels)
            s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
            s.world_set_episode_report(STEP)
            upload(s, world)
            # no list: the event is recorded, nothing is written
            s.device_write(rewards, np.full(agents, -7.0, dtype=F))
            s.world_step(params)
            s.world_export_episode_step_async(rewards, flags, 0, slot=1)
            s.export_wait(1)
            s.world_export_episode_step(rewards, flags, 0)
            assert (s.device_read(rewards, agents) == -7.0).all() and len(s.world_episode_rewards()) == 0
            s.world_set_episodes(rules, agents)
            for step in range(2):
                s.world_step(params)
                host_r, host_f = s.world_episode_rewards(), s.world_episode_flags()
                assert host_r.any() and host_f.any() and not host_f.all()
                for way in range(2):
                    s.device_write(rewards, np.full(agents, -7.0, dtype=F))
                    s.device_write(flags, np.full(agents, -7, dtype=np.int32))
                    if way == 0:
                        s.world_export_episode_step(rewards, flags, agents)
                    else:
                        s.world_export_episode_step_async(rewards, flags, agents, slot=3)
                        s.export_wait(3)
                    assert s.device_read(rewards, agents).tobytes() == host_r.tobytes() and s.device_read(flags, agents, np.int32).tobytes() == host_f.tobytes()
            r, f = ctypes.c_void_p(rewards), ctypes.c_void_p(flags)
            assert L.s2amd_world_export_episode_step(h, r, f, agents - 1) == E_CAPACITY and L.s2amd_world_export_episode_step_async(h, r, f, agents - 1, 0) == E_CAPACITY
            assert L.s2amd_world_export_episode_step(h, None, f, agents) == E_INVALID and L.s2amd_world_export_episode_step(h, r, None, agents) == E_INVALID
            assert L.s2amd_world_export_episode_step(h, r, f, -1) == E_INVALID
            assert L.s2amd_world_export_episode_step_async(h, r, f, agents, 4) == E_INVALID and L.s2amd_world_export_episode_step_async(h, r, f, agents, -1) == E_INVALID
            assert s.device_read(rewards, agents).tobytes() == host_r.tobytes()  # the refusals wrote nothing
        finally:
            s.device_free(rewards)
            s.device_free(flags)


def test_getters_and_refusals():
    """The getters' state machine -- no list, no world, no step, a flag that was not set, a list set since the step -- and every refusal of
    the setter leaving the previous answers in place."""
    params, world = golden("mixed24_PGS")
    good = wire.episode_rule_list([rule(VALUE, 0, 2, frame=0, minus=(1, 0), shape=2, gain=0.5, bias=1.0, lower=-1.0, upper=1.0), rule(TEST, 1, gain=1.0, bias=-1.0),
                                   rule(TERMINATE, 2, 0, gain=5.0, lower=2.0), rule(TRUNCATE, 0, 3, lower=0.0, upper=0.0)])
    limits = np.array([0, 2, 0], dtype=np.int32)

    def bad_lists():
        for name, value, record in (("kind", 0, 0), ("kind", 5, 0), ("shape", -1, 0), ("shape", 3, 0), ("agent", -1, 0), ("agent", 3, 0), ("channelA", -2, 0),
                                    ("channelA", -1, 0), ("frameA", -1, 0), ("channelB", -1, 0), ("frameB", -1, 0), ("channelB", 1, 1), ("frameB", 1, 3), ("flags", 8, 1),
                                    ("flags", -1, 1), ("gain", np.nan, 0), ("gain", np.inf, 1), ("bias", np.nan, 0), ("bias", -np.inf, 1), ("lower", np.nan, 0),
                                    ("upper", np.nan, 0), ("lower", 2.0, 0), ("upper", -2.0, 0), ("bias", 0.5, 2), ("bias", -1.0, 3)):
            wrong = good.copy()
            wrong[name][record] = value
            yield "%s = %r" % (name, value), wrong
        for index, value in ((0, 1), (3, -1)):
            wrong = good.copy()
            wrong["reserved"][2][index] = value
            yield "reserved", wrong

    with hip.Solver(0) as s:
        L, h = s._L, s._h
        assert all(len(getattr(s, name)()) == 0 for name in GETTERS[:5]) and s.world_episode_counts().tolist() == [0] * 8  # no list
        s.world_set_episodes(good, 3, limits)  # accepted before any world
        s.world_set_episode_report(ALL)
        refuses(s, E_STATE, GETTERS)  # no resident world
        driven(s, world)
        upload(s, world)
        refuses(s, E_STATE, GETTERS)  # no step since the upload
        acc = ref.Accounting(3)
        s.world_set_actions(np.array([2.5, 0.5, -1.5, 0.0], dtype=F))
        s.world_step(params)
        before = expect(s, acc, good, 3, limits, "before the refusals")
        assert before["flags"].tolist() == [2, 0, 1] and before["rewards"][0] != 0
        # per call
        many = np.zeros(wire.MAX_EPISODE_RULES + 1, dtype=wire.episode_rule_dtype)
        many[:] = good[1]
        P, n = wire.as_ptr, len(good)
        assert L.s2amd_world_set_episodes(h, P(good), -1, 3, None) == E_INVALID and L.s2amd_world_set_episodes(h, None, n, 3, None) == E_INVALID
        assert L.s2amd_world_set_episodes(h, P(many), len(many), 3, None) == E_INVALID and L.s2amd_world_set_episodes(h, P(good), n, 0, None) == E_INVALID
        assert L.s2amd_world_set_episodes(h, P(good), n, 2, None) == E_INVALID and L.s2amd_world_set_episodes(h, None, 0, -1, None) == E_INVALID
        assert L.s2amd_world_set_episodes(h, None, 0, wire.MAX_EPISODE_AGENTS + 1, None) == E_INVALID
        assert L.s2amd_world_set_episodes(h, P(good), n, 3, P(np.array([0, -1, 0], dtype=np.int32))) == E_INVALID
        assert L.s2amd_world_set_episode_report(h, 16) == E_INVALID
        # per record
        for what, wrong in bad_lists():
            assert ref.valid(wrong, 3) >= 0, what
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_episodes(wrong, 3, limits)
        # a refused list leaves the previous answers in place
        assert_same_bytes(s.world_episode_states(), before["states"], "after the refusals")
        assert_same_bytes(s.world_episode_rule_states(), before["rule_states"], "after the refusals")
        # the getters' arguments
        count = ctypes.c_int32(-7)
        out = np.zeros(3, dtype=F)
        assert L.s2amd_world_episode_rewards(h, P(out), 2, ctypes.byref(count)) == E_CAPACITY and count.value == 3 and not out.any()
        assert L.s2amd_world_episode_rewards(h, P(out), -1, ctypes.byref(count)) == E_INVALID and L.s2amd_world_episode_rewards(h, P(out), 3, None) == E_INVALID
        states = np.zeros(3, dtype=wire.episode_state_dtype)
        assert L.s2amd_world_episode_states(h, P(states), 2, ctypes.byref(count)) == E_CAPACITY and count.value == 3
        rule_states = np.zeros(n, dtype=wire.episode_rule_state_dtype)
        assert L.s2amd_world_episode_rule_states(h, P(rule_states), n - 1, ctypes.byref(count)) == E_CAPACITY and count.value == n
        events = np.zeros(2, dtype=wire.episode_event_dtype)
        count.value = -7
        assert L.s2amd_world_episode_events(h, P(events), 1, ctypes.byref(count)) == E_CAPACITY and count.value == 2 and events.tobytes() == bytes(events.nbytes)
        assert L.s2amd_world_episode_events(h, P(events), 2, ctypes.byref(count)) == 0 and events["agent"].tolist() == [0, 2]
        assert L.s2amd_world_episode_counts(h, None) == E_INVALID
        # the next step goes on from the accounting that stood
        s.world_step(params)
        after = expect(s, acc, good, 3, limits, "after the refusals, the next step")
        assert after["states"]["episodeLength"].tolist() == [1, 2, 1] and after["states"]["episodes"].tolist() == [2, 1, 2]
        # a getter whose flag was not set before the last step
        for flag, opened in ((STEP, GETTERS[:2]), (STATES, GETTERS[2:3]), (RULE_STATES, GETTERS[3:4]), (EVENTS, GETTERS[4:5])):
            s.world_set_episode_report(flag)
            s.world_step(params)
            for name in GETTERS[:5]:
                if name in opened:
                    assert len(getattr(s, name)()) > 0, name
                else:
                    with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                        getattr(s, name)()
            assert s.world_episode_counts()[:4].sum() == n
        s.world_set_episodes(good, 3, limits)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_episode_states()  # no step since the list was set
        # cleared: zero counts at once
        s.world_set_episodes(good[:0], 0)
        assert all(len(getattr(s, name)()) == 0 for name in GETTERS[:5]) and s.world_episode_counts().tolist() == [0] * 8


def test_all_ten_facilities_on_together():
    """mixed24 with the contact, joint, shape and body reports, the step metrics, sensors, rays, grids, the observers and the episodes on
    at once over 4 steps: the downloaded world equals the oracle chain's, the episodes equal their statement, and every answer of the nine
    other reports is byte-equal to that of a second solver whose episode report is off."""
    params, world = golden("mixed24_PGS")
    observers, channels = every_kind(world)
    d = slots_of(world)["dynamic"]
    rays = np.array([down_ray(world, d[0]), down_ray(world, d[3])], dtype=wire.ray_sensor_dtype)
    centre = world["bodies"]["position"][d[0]]
    grids = np.array([gw.make_grid((float(centre[0]) - 2.0, float(centre[1]) - 2.0), 0.0, 0.5, 8, 8)], dtype=wire.grid_sensor_dtype)
    sensors = np.array([sw.make_sensor(sw.box_vertices(3.0, 3.0), 0.0, position=(float(centre[0]), float(centre[1])))], dtype=wire.sensor_dtype)
    rules = wire.episode_rule_list([rule(VALUE, k % 3, k % channels, minus=((k + 1) % channels, 1) if k % 2 else None, shape=k % 3, gain=0.5) for k in range(2 * channels)] +
                                   [rule(TERMINATE, 1, 13, shape=ref.ABS, lower=0.5), rule(TRUNCATE, 2, 0, minus=(0, 1), lower=1e-4)])
    limits = np.array([2, 0, 3], dtype=np.int32)
    answers = (lambda k: k.world_touch_events(), lambda k: k.world_touching(), lambda k: k.world_body_sums(), lambda k: k.world_joint_states(),
               lambda k: k.world_joint_limit_events(), lambda k: k.world_body_joint_sums(), lambda k: k.world_joint_summary(), lambda k: k.world_shape_draws(),
               lambda k: k.world_shape_summary(), lambda k: k.world_islands(), lambda k: k.world_body_states(), lambda k: k.world_body_summary(),
               lambda k: k.world_metrics(), lambda k: k.world_sensor_inside(), lambda k: k.world_sensor_states(), lambda k: k.world_ray_states(),
               lambda k: k.world_ray_ranges(), lambda k: k.world_ray_events(), lambda k: k.world_grid_categories(), lambda k: k.world_grid_shapes(),
               lambda k: k.world_grid_occupancy(), lambda k: k.world_grid_states(), lambda k: k.world_observations(), lambda k: k.world_observer_states(),
               lambda k: k.world_observer_counts())

    def flat(answer):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in answer) if isinstance(answer, tuple) else np.ascontiguousarray(answer).tobytes()

    with hip.Solver(0) as s, hip.Solver(0) as twin:
        for k in (s, twin):
            k.world_set_report(wire.REPORT_ALL)
            k.world_set_joint_report(wire.JOINT_REPORT_ALL)
            k.world_set_shape_report(wire.SHAPE_REPORT_ALL)
            k.world_set_body_report(wire.BODY_REPORT_STATES | wire.BODY_REPORT_REST | wire.BODY_REPORT_ISLANDS)
            k.world_set_metrics(wire.METRICS_ALL, 4)
            k.world_set_sensors(sensors)
            k.world_set_sensor_report(wire.SENSOR_REPORT_ALL)
            k.world_set_ray_sensors(rays)
            k.world_set_ray_report(wire.RAY_REPORT_ALL)
            k.world_set_grid_sensors(grids)
            k.world_set_grid_report(wire.GRID_REPORT_ALL)
            k.world_set_observers(observers, channels, 2)
            k.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR | wire.OBSERVATION_REPORT_STATES)
            k.world_set_episodes(rules, 3, limits)
        s.world_set_episode_report(ALL)
        upload(s, world), upload(twin, world)
        ref_world = world_chain.copy_world(world)
        acc = ref.Accounting(3)
        for step in range(4):
            step_both(s, params, ref_world)
            twin.world_step(params)
            what = "all ten, step %d" % step
            want = expect(s, acc, rules, 3, limits, what)
            assert want["counts"][:4].tolist() == [len(rules), 0, 0, 0]
            for i, answer in enumerate(answers):
                assert flat(answer(s)) == flat(answer(twin)), (what, i)
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                twin.world_episode_rewards()
            a, b = s.stats(), twin.stats()
            assert (a["solveLaunches"], a["structureBuilds"]) == (b["solveLaunches"], b["structureBuilds"]), what
        assert want["states"]["episodes"].sum() > 0 and want["rule_states"]["x"].any()
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "all ten")
