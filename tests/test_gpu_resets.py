"""Resets on the resident world (s2amd_world_set_resets / _set_reset_report / _reset_agents / _reset_states / _reset_counts;
solver2d_amd/csrc/resets.hip) against their statement (tests/reset_ref.py), byte for byte: a pass is compared with the statement applied
to the download taken before it, and the chains with the CPU oracle chain to which the statement is applied at the same places, with the
full pair loop on both sides.  The worlds are the committed tests/golden worlds and one synthetic pyramid; tests/reset_world.py holds
the agents, the reset poses and the chain's conditions."""
import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import contact_report_ref, episode_ref, grid_report_world as gw, reset_ref as ref, reset_world, sensor_report_world as sw, world_chain
from tests.resident import E_INVALID, E_STATE, assert_same_world, down_ray, download, every_kind, refuses, slots_of, upload
from tests.world_chain import _create_contacts, golden

pytestmark = pytest.mark.gpu

ON_END, STATES = wire.RESET_ON_EPISODE_END, wire.RESET_REPORT_STATES


def expect_pass(s, world, before, bodies, joints, agents, seed, trigger, counters, what):
    """The statement applied to `before` (a download) against the download taken now, all six arrays, and the counts -> (the world as
    downloaded, the counts)"""
    want = world_chain.copy_world(before)
    counts = ref.apply(want, bodies, joints, agents, seed, trigger, counters)
    got = download(s, world)[0]
    assert_same_world(got, want, what)
    assert s.world_reset_counts().tolist() == counts.tolist(), what
    return got, counts


def one_of(agents, *which):
    trigger = np.zeros(agents, dtype=bool)
    trigger[list(which)] = True
    return trigger


def pair_loop(s, ref_world, what):
    """s2amd_world_find_pairs against the oracle's query, and the caller's s2CreateContact on both sides -> new pairs"""
    got, want = s.world_find_pairs(), world_chain.oracle_find_pairs(ref_world)
    assert np.array_equal(got, want), what + ": new pairs"
    if len(got):
        slots, contacts, pairs = _create_contacts(ref_world, got)
        s.world_set_contacts(slots, contacts, pairs)
    return len(got)


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
@pytest.mark.parametrize("name", ["far_ragdoll_pile0_PGS_Soft", "joint_grid6_TGS_NGS", "shapes_zoo40_TGS_Sticky"])
def test_one_shot_reset_of_one_agent(name, fast):
    """Two steps, then s2amd_world_reset_agents on the agent with the most bodies, carried to another agent's place: bodies, contacts,
    joints, shapes, pairs and origins equal the statement applied to the download taken before; every other agent stands.  The ragdolls'
    joints are listed with JOINT_SETTINGS; the sticky world's friction cache is cleared with the manifolds."""
    params, world = golden(name)
    agent_of_body, agent_of_joint, agents = reset_world.agents_of(world)
    sizes = np.bincount(agent_of_body[agent_of_body >= 0], minlength=agents)
    touching = reset_world.touching_agents(world, agent_of_body, agents)
    agent = int(np.argmax(sizes * 1000 + touching))
    other = int((agent + 1) % agents)
    poses = reset_world.swapped_poses(world, agent_of_body, agents, [(agent, other)])
    poses["joints"]["motorSpeed"] = poses["joints"]["motorSpeed"] + np.float32(0.25)
    poses["joints"]["enableLimit"] = 1 - poses["joints"]["enableLimit"]
    bodies, joints = wire.resets_from_world(poses["bodies"], poses["joints"], agent_of_body, agent_of_joint)
    assert ref.valid(bodies, joints, agents) is None and (joints["flags"] == wire.RESET_JOINT_SETTINGS).all()
    with hip.Solver(0, fast=fast) as s:
        s.world_set_resets(bodies, joints, agents, seed=3)
        upload(s, world)
        for _ in range(2):
            s.world_step(params)
        before = download(s, world)[0]
        s.world_reset_agents([agent])
        got, counts = expect_pass(s, world, before, bodies, joints, agents, 3, one_of(agents, agent), np.zeros(agents, dtype=np.int32), name)
        assert counts[ref.BODIES] == sizes[agent] and counts[ref.SHAPES] >= 1 and counts[ref.AGENTS] == 1
        listed = joints["joint"][joints["agent"] == agent]
        assert counts[ref.JOINTS] == len(listed)
        if len(listed):
            assert got["joints"]["motorSpeed"][listed].tobytes() != before["joints"]["motorSpeed"][listed].tobytes()
        if "Sticky" in name:
            hit = (before["pairs"]["shapeA"] >= 0) & ((agent_of_body[before["contacts"]["bodyA"]] == agent) | (agent_of_body[before["contacts"]["bodyB"]] == agent))
            assert before["contacts"]["frictionPersisted"][hit].any() and before["contacts"]["points"]["frictionAnchorA"][hit].any()
            assert not got["contacts"]["frictionPersisted"][hit].any() and not got["contacts"]["points"]["frictionAnchorA"][hit].any() and counts[ref.CONTACTS] == hit.sum()
        # and the world steps on from there
        s.world_step(params)


@pytest.mark.parametrize("name", reset_world.CHAIN_WORLDS)
def test_chain_of_steps_with_resets_and_the_pair_loop(name):
    """12 steps with s2amd_world_reset_agents before steps 3 and 7 on different agents and the full pair loop on both sides (the device's
    query and s2amd_world_set_contacts; the oracle's query and _create_contacts): every step byte-equal to the oracle chain with the
    statement applied.  Each chain empties a contact by a reset, separates a pair of a reset body in the step after, and finds a new
    pair in the query behind a reset; no structure is built by the reset call itself."""
    params, world, plan = reset_world.chain_plan(name)
    ref_world = world_chain.copy_world(world)
    counters = np.zeros(plan["agents"], dtype=np.int32)
    seen = reset_world.Conditions()
    marked = None
    with hip.Solver(0) as s:
        s.world_set_resets(plan["bodies"], plan["joints"], plan["agents"], seed=plan["seed"])
        upload(s, world)
        for step in range(1, reset_world.CHAIN_STEPS + 1):
            what = "%s step %d" % (name, step)
            if step in reset_world.RESET_BEFORE:
                agent = plan["resets"][reset_world.RESET_BEFORE.index(step)]
                builds = s.stats()["structureBuilds"]
                s.world_reset_agents([agent])
                assert s.stats()["structureBuilds"] == builds, what
                counts, marked = reset_world.oracle_reset(plan, ref_world, counters, agent)
                assert s.world_reset_counts().tolist() == counts.tolist(), what
                world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, what + ": behind the reset")
                seen.emptied.append(int(counts[ref.CONTACTS]))
                seen.found.append(pair_loop(s, ref_world, what + ": behind the reset"))
            info = s.world_step(params)
            order, _ = s.contact_order()
            jorder, _ = s.joint_order()
            contacts_before = ref_world["contacts"].copy()
            status = world_chain.oracle_world_step(params, ref_world, contact_order=order, joint_order=jorder)
            assert info["separatedCount"] == int((status == wire.PAIR_SEPARATED).sum()), what
            if marked is not None:
                seen.separated.append(reset_world.separated_of(status, contacts_before, marked))
                assert np.array_equal(s.world_separated(), np.flatnonzero(status == wire.PAIR_SEPARATED)), what
                marked = None
            if info["movedCount"] > 0:
                pair_loop(s, ref_world, what)
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, what)
    seen.assert_met(name)


def test_episode_driven_resets():
    """mixed24: an episode list of two agents with step limits {3, 5} and no rules (so no observers), RESET_ON_EPISODE_END for 12 steps.
    Agent 0 resets at the end of steps 3, 6, 9 and 12, agent 1 at the end of steps 5 and 10, by the statement driven by episode_ref's
    flags; the pair loop runs when the refit moved something or somebody was done.  With the episode report flags at 0 the counts say
    source off and the world equals the plain chain."""
    params, world = golden("mixed24_PGS")
    agent_of_body, agent_of_joint, agents = reset_world.agents_of(world)
    poses = reset_world.swapped_poses(world, agent_of_body, agents, [(0, 1)])
    bodies, joints = wire.resets_from_world(poses["bodies"], poses["joints"], agent_of_body, agent_of_joint)
    bodies["positionJitter"], bodies["angularJitter"] = (0.0625, 0.0), 0.5
    limits = np.array([3, 5], dtype=np.int32)
    no_rules = wire.episode_rule_list([])
    with hip.Solver(0) as s:
        s.world_set_episodes(no_rules, 2, limits)
        s.world_set_episode_report(wire.EPISODE_REPORT_STEP)
        s.world_set_resets(bodies, joints, agents, seed=17)
        s.world_set_reset_report(ON_END | STATES)
        upload(s, world)
        ref_world = world_chain.copy_world(world)
        acc, counters = episode_ref.Accounting(2), np.zeros(agents, dtype=np.int32)
        done_at = {0: [], 1: []}
        for step in range(1, 13):
            what = "episode-driven, step %d" % step
            info = s.world_step(params)
            order, _ = s.contact_order()
            jorder, _ = s.joint_order()
            world_chain.oracle_world_step(params, ref_world, contact_order=order, joint_order=jorder)
            want = episode_ref.step(acc, None, no_rules, 2, limits, (0, 0))
            assert s.world_episode_flags().tolist() == want["flags"].tolist(), what
            trigger = ref.episode_trigger(want["flags"], agents)
            counts = ref.apply(ref_world, bodies, joints, agents, 17, trigger, counters)
            assert s.world_reset_counts().tolist() == counts.tolist(), what
            states = s.world_reset_states()
            assert states["resets"].tolist() == counters.tolist() and states["triggered"].tolist() == trigger.astype(int).tolist(), what
            for a in np.flatnonzero(trigger):
                done_at[int(a)].append(step)
            if info["movedCount"] > 0 or trigger.any():
                pair_loop(s, ref_world, what)
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, what)
        assert done_at == {0: [3, 6, 9, 12], 1: [5, 10]} and counters.tolist() == [4, 2] + [0] * (agents - 2)
        # the episode report off: the source is off, nothing is enqueued, the world steps as the plain chain does
        s.world_set_episode_report(0)
        for step in range(3):
            info = s.world_step(params)
            order, _ = s.contact_order()
            jorder, _ = s.joint_order()
            world_chain.oracle_world_step(params, ref_world, contact_order=order, joint_order=jorder)
            assert s.world_reset_counts().tolist() == [0] * 7 + [1]
            assert s.world_reset_states()["resets"].tolist() == counters.tolist()
            if info["movedCount"] > 0:
                pair_loop(s, ref_world, "source off")
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "source off, step %d" % step)


def test_jitter_differs_per_reset_and_per_seed():
    """Three consecutive resets of one agent give three different states, each equal to the statement at the agent's counter; another
    seed gives others; the counters come back through the states getter."""
    params, world = golden("mixed24_PGS")
    agent_of_body, agent_of_joint, agents = reset_world.agents_of(world)
    bodies, joints = wire.resets_from_world(world["bodies"], world["joints"], agent_of_body, agent_of_joint)
    bodies["positionJitter"], bodies["velocityJitter"], bodies["angularJitter"] = (0.125, 0.25), (0.5, 0.0), 1.0
    agent = int(np.argmax(np.bincount(agent_of_body[agent_of_body >= 0])))
    mine = agent_of_body == agent
    with hip.Solver(0) as s:
        upload(s, world)
        s.world_set_reset_report(STATES)
        seen = []
        for seed in (1, 2):
            s.world_set_resets(bodies, joints, agents, seed=seed)
            counters = np.zeros(agents, dtype=np.int32)
            for k in range(3):
                before = download(s, world)[0]
                s.world_reset_agents([agent])
                got, counts = expect_pass(s, world, before, bodies, joints, agents, seed, one_of(agents, agent), counters, "seed %d, reset %d" % (seed, k))
                assert s.world_reset_states()["resets"].tolist() == counters.tolist() and counters[agent] == k + 1
                seen.append(b"".join(got["bodies"][n][mine].tobytes() for n in ("position", "linearVelocity", "angularVelocity")))
                # no jitter on the y velocity: the base's bits
                assert got["bodies"]["linearVelocity"][mine][:, 1].tobytes() == world["bodies"]["linearVelocity"][mine][:, 1].tobytes()
        assert len(set(seen)) == 6


def test_skips_disabled_records_joint_settings_and_counts():
    """A record on a free body slot, on a static body, beyond the capacity and DISABLED; a free joint slot and one beyond the capacity;
    JOINT_SETTINGS on a revolute and on a mouse joint: the world and the counts equal the statement's."""
    params, world = golden("mixed24_PGS")
    at = slots_of(world)
    nb, nj = len(world["bodies"]), len(world["joints"])
    rb = np.zeros(5, dtype=wire.reset_body_dtype)
    rb["body"] = [at["free"][0], at["static"][0], nb + 3, at["dynamic"][0], at["dynamic"][1]]
    rb["rot"], rb["position"] = (0.0, 1.0), (1.0, 20.0)
    rb["flags"][4] = wire.RESET_DISABLED
    rj = np.zeros(5, dtype=wire.reset_joint_dtype)
    rj["joint"] = [at["revolute"][0], at["mouse"][0], at["free_joint"][0], nj + 1, at["revolute"][1]]
    rj["flags"] = [wire.RESET_JOINT_SETTINGS, wire.RESET_JOINT_SETTINGS, wire.RESET_JOINT_SETTINGS, 0, wire.RESET_DISABLED]
    rj["enableMotor"], rj["enableLimit"], rj["motorSpeed"], rj["targetA"] = 1, 1, -2.5, (3.0, 4.0)
    assert ref.valid(rb, rj, 1) is None
    with hip.Solver(0) as s:
        upload(s, world)
        s.world_set_resets(rb, rj, 1)
        s.world_step(params)
        before = download(s, world)[0]
        s.world_reset_agents()
        got, counts = expect_pass(s, world, before, rb, rj, 1, 0, [True], np.zeros(1, dtype=np.int32), "skips")
        assert counts.tolist()[:5] == [1, 1, 3, 2, 2] and counts[ref.SHAPES] >= 1
        assert got["joints"]["targetA"][at["mouse"][0]].tolist() == [3.0, 4.0] and got["joints"]["motorSpeed"][at["revolute"][0]] == -2.5
        # nobody listed: nothing is enqueued and the last pass's counts stand
        s.world_reset_agents([])
        assert s.world_reset_counts().tolist() == counts.tolist()
        s.world_step(params)


def test_boundaries_of_waves_and_workgroups():
    """A base-45 pyramid, 1,035 boxes: 1,024 and then 1,025 records in one agent (the last lane of the fourth workgroup, the first of a
    fifth), then one agent per body with every 64th agent triggered -- ballots and counts across wave and workgroup edges."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    world = synthetic.pyramid_world(45)
    boxes = np.flatnonzero(reset_world.movable(world))
    assert len(boxes) == 1035
    lifted = world_chain.copy_world(world)
    lifted["bodies"]["position"][:, 1] += np.float32(0.5)
    with hip.Solver(0) as s:
        upload(s, world)
        s.world_step(params)
        for count in (1024, 1025):
            agent_of_body = np.full(len(world["bodies"]), -1, dtype=np.int32)
            agent_of_body[boxes[:count]] = 0
            bodies, joints = wire.resets_from_world(lifted["bodies"], lifted["joints"], agent_of_body, np.zeros(0, dtype=np.int32))
            bodies["velocityJitter"] = (0.25, 0.0)
            assert len(bodies) == count
            s.world_set_resets(bodies, joints, 1, seed=count)
            before = download(s, world)[0]
            s.world_reset_agents()
            _, counts = expect_pass(s, world, before, bodies, joints, 1, count, [True], np.zeros(1, dtype=np.int32), "%d records" % count)
            assert counts[ref.BODIES] == count == counts[ref.SHAPES] and counts[ref.CONTACTS] > 0
        agent_of_body = np.full(len(world["bodies"]), -1, dtype=np.int32)
        agent_of_body[boxes] = np.arange(1035)
        bodies, joints = wire.resets_from_world(lifted["bodies"], lifted["joints"], agent_of_body, np.zeros(0, dtype=np.int32))
        s.world_set_resets(bodies, joints, 1035, seed=9)
        s.world_set_reset_report(STATES)
        every64 = np.arange(0, 1035, 64, dtype=np.int32)
        counters = np.zeros(1035, dtype=np.int32)
        before = download(s, world)[0]
        s.world_reset_agents(every64)
        trigger = np.zeros(1035, dtype=bool)
        trigger[every64] = True
        _, counts = expect_pass(s, world, before, bodies, joints, 1035, 9, trigger, counters, "every 64th agent")
        assert counts[ref.AGENTS] == len(every64) == counts[ref.BODIES] == 17
        assert s.world_reset_states()["resets"].tolist() == counters.tolist() and counters.sum() == 17
        # ... and the complement, so that every wave but the triggered lanes' votes
        before = download(s, world)[0]
        s.world_reset_agents(np.flatnonzero(~trigger).astype(np.int32))
        _, counts = expect_pass(s, world, before, bodies, joints, 1035, 9, ~trigger, counters, "all but every 64th")
        assert counts[ref.AGENTS] == 1035 - 17 and (counters == 1).all()


def test_off_state_enqueues_nothing():
    """The list set, the flags at 0, no one-shot call: a 6-step chain is byte-equal to the chain of a solver without a list, with the
    same launches; the getters refuse."""
    params, world, plan = reset_world.chain_plan("mixed24_PGS")
    with hip.Solver(0) as s, hip.Solver(0) as plain:
        s.world_set_resets(plan["bodies"], plan["joints"], plan["agents"], seed=1)
        upload(s, world), upload(plain, world)
        for step in range(6):
            a, b = s.world_step(params), plain.world_step(params)
            assert a["movedCount"] == b["movedCount"]
            if a["movedCount"] > 0:
                new = s.world_find_pairs()
                assert np.array_equal(new, plain.world_find_pairs())
                if len(new):
                    both = world_chain.copy_world(download(s, world)[0])
                    slots, contacts, pairs = _create_contacts(both, new)
                    s.world_set_contacts(slots, contacts, pairs), plain.world_set_contacts(slots, contacts, pairs)
            assert_same_world(download(s, world)[0], download(plain, world)[0], "off state, step %d" % step)
            st, pt = s.stats(), plain.stats()
            assert (st["kernelLaunches"], st["structureBuilds"]) == (pt["kernelLaunches"], pt["structureBuilds"])
            refuses(s, E_STATE, ("world_reset_states", "world_reset_counts"))


def test_all_facilities_on_together_and_refusals():
    """mixed24 with all ten reports and the resets on: the world equals the oracle chain with the statement applied, a contact that
    touched and is parted by a reset is in `ended` of the next step's touch events, and the refusals of the interface."""
    params, world = golden("mixed24_PGS")
    observers, channels = every_kind(world)
    d = slots_of(world)["dynamic"]
    rays = np.array([down_ray(world, d[0]), down_ray(world, d[3])], dtype=wire.ray_sensor_dtype)
    centre = world["bodies"]["position"][d[0]]
    grids = np.array([gw.make_grid((float(centre[0]) - 2.0, float(centre[1]) - 2.0), 0.0, 0.5, 8, 8)], dtype=wire.grid_sensor_dtype)
    sensors = np.array([sw.make_sensor(sw.box_vertices(3.0, 3.0), 0.0, position=(float(centre[0]), float(centre[1])))], dtype=wire.sensor_dtype)
    _, _, plan = reset_world.chain_plan("mixed24_PGS")
    agents, first = plan["agents"], plan["resets"][0]
    limits = np.zeros(agents, dtype=np.int32)
    limits[first] = 2
    no_rules = wire.episode_rule_list([])
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
        s.world_set_body_report(wire.BODY_REPORT_STATES | wire.BODY_REPORT_REST | wire.BODY_REPORT_ISLANDS)
        s.world_set_metrics(wire.METRICS_ALL, 4)
        s.world_set_sensors(sensors)
        s.world_set_sensor_report(wire.SENSOR_REPORT_ALL)
        s.world_set_ray_sensors(rays)
        s.world_set_ray_report(wire.RAY_REPORT_ALL)
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(wire.GRID_REPORT_ALL)
        s.world_set_observers(observers, channels, 2)
        s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR | wire.OBSERVATION_REPORT_STATES)
        s.world_set_episodes(no_rules, agents, limits)
        s.world_set_episode_report(wire.EPISODE_REPORT_ALL)
        # before a world and before a list
        refuses(s, E_STATE, ("world_reset_agents",))
        s.world_set_resets(plan["bodies"], plan["joints"], agents, seed=plan["seed"])
        refuses(s, E_STATE, ("world_reset_agents", "world_reset_states", "world_reset_counts"))
        s.world_set_reset_report(ON_END)
        upload(s, world)
        refuses(s, E_STATE, ("world_reset_states", "world_reset_counts"))
        ref_world = world_chain.copy_world(world)
        counters = np.zeros(agents, dtype=np.int32)
        parted_seen = 0
        touching = contact_report_ref.touching_mask(ref_world)
        parted = None
        for step in range(1, 6):
            what = "together, step %d" % step
            info = s.world_step(params)
            order, _ = s.contact_order()
            jorder, _ = s.joint_order()
            world_chain.oracle_world_step(params, ref_world, contact_order=order, joint_order=jorder)
            began, ended = s.world_touch_events()
            want_began, want_ended = contact_report_ref.events(touching, ref_world)
            assert np.array_equal(began, want_began) and np.array_equal(ended, want_ended), what
            if parted is not None:
                # what touched after the step before, was emptied by that step's reset and does not touch again has ended in this one
                # (a manifold that touches again -- two bodies of the agent, carried together -- is no flip)
                parted = parted[~contact_report_ref.touching_mask(ref_world)[parted]]
                assert np.isin(parted, ended).all(), what
                parted_seen += len(parted)
                parted = None
            touching = contact_report_ref.touching_mask(ref_world)
            trigger = np.zeros(agents, dtype=bool)
            trigger[first] = step % 2 == 0
            counts = ref.apply(ref_world, plan["bodies"], plan["joints"], agents, plan["seed"], trigger, counters)
            assert s.world_reset_counts().tolist() == counts.tolist(), what
            refuses(s, E_STATE, ("world_reset_states",))
            if trigger.any():
                emptied = np.flatnonzero(touching & ~contact_report_ref.touching_mask(ref_world))
                assert len(emptied)
                parted = emptied
            if info["movedCount"] > 0 or trigger.any():
                pair_loop(s, ref_world, what)
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, what)
        assert parted_seen > 0 and counters[first] == 2
        # refusals: a bad record and a slot named twice leave the list standing; unknown flag bits; an agent beyond the agents
        wrong = plan["bodies"].copy()
        wrong["angularJitter"][0] = -1.0
        twice = plan["bodies"].copy()
        twice["body"][1] = twice["body"][0]
        for bad in (wrong, twice):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_resets(bad, plan["joints"], agents)
        for call, args in ((s.world_set_reset_report, (4,)), (s.world_reset_agents, ([agents],)), (s.world_reset_agents, ([-1],))):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                call(*args)
        movable_shapes = np.flatnonzero((world["shapes"]["type"] != wire.SHAPE_FREE) & reset_world.movable(world)[np.clip(world["shapes"]["body"], 0, None)]).astype(np.int32)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_set_refit_order(movable_shapes)
        s.world_reset_agents([first])
        assert s.world_reset_counts()[ref.AGENTS] == 1
        # cleared: every getter answers nothing, a refit order is welcome again and refuses the list in turn
        s.world_set_resets(plan["bodies"][:0], plan["joints"][:0], 0)
        assert len(s.world_reset_states()) == 0 and not s.world_reset_counts().any()
        s.world_set_refit_order(movable_shapes)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_set_resets(plan["bodies"], plan["joints"], agents)
