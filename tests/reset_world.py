"""What the tests of the resets (tests/test_resets_host.py, tests/test_gpu_resets.py) share: the agents of a golden world, the reset
poses chosen on the CPU, and the chain of steps with resets and the full pair loop on the CPU oracle, with the conditions that keep the
chain test from passing vacuously.  Test infrastructure only."""
import numpy as np

from solver2d_amd import wire
from tests import reset_ref, world_chain

CHAIN_WORLDS = ("far_ragdoll_pile0_PGS_Soft", "mixed24_PGS", "tumbler60_TGS_Soft", "shapes_zoo40_TGS_Sticky")
CHAIN_STEPS = 12
RESET_BEFORE = (3, 7)  # the one-shot resets come before these steps (counted from 1), on different agents


def movable(world):
    t = world["bodies"]["type"]
    return (t != wire.BODY_FREE) & (t != wire.BODY_STATIC)


def agents_of(world, single=3):
    """Agents of a world: the bodies a chain of joints holds together are one agent (a ragdoll), and the movable bodies without a
    joint form agents of `single` bodies in slot order.  A body jointed to a static body only (a drum on its axle) is an agent of
    its own.  -> (agent_of_body int32[nb] with -1 for static and free slots, agent_of_joint int32[nj], agents)"""
    b, j = world["bodies"], world["joints"]
    move = movable(world)
    parent = np.arange(len(b))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    jointed = np.zeros(len(b), dtype=bool)
    for k in np.flatnonzero(j["type"] != wire.JOINT_FREE):
        a, c = int(j["bodyA"][k]), int(j["bodyB"][k])
        for body in (a, c):
            if 0 <= body < len(b) and move[body]:
                jointed[body] = True
        if 0 <= a < len(b) and 0 <= c < len(b) and move[a] and move[c]:
            parent[find(a)] = find(c)
    agent_of_body = np.full(len(b), -1, dtype=np.int32)
    roots, agents = {}, 0
    for i in np.flatnonzero(move & jointed):
        r = find(int(i))
        if r not in roots:
            roots[r] = agents
            agents += 1
        agent_of_body[i] = roots[r]
    loose = np.flatnonzero(move & ~jointed)
    for n, i in enumerate(loose):
        agent_of_body[i] = agents + n // single
    agents += (len(loose) + single - 1) // single
    agent_of_joint = np.full(len(j), -1, dtype=np.int32)
    for k in np.flatnonzero(j["type"] != wire.JOINT_FREE):
        for body in (int(j["bodyA"][k]), int(j["bodyB"][k])):
            if 0 <= body < len(b) and agent_of_body[body] >= 0:
                agent_of_joint[k] = agent_of_body[body]
                break
    return agent_of_body, agent_of_joint, agents


def touching_agents(world, agent_of_body, agents):
    """Per agent: manifolds with points on its bodies"""
    c, live = world["contacts"], world["pairs"]["shapeA"] >= 0
    out = np.zeros(agents, dtype=np.int32)
    for i in np.flatnonzero(live & (c["pointCount"] > 0)):
        for body in {int(c["bodyA"][i]), int(c["bodyB"][i])}:
            if agent_of_body[body] >= 0:
                out[agent_of_body[body]] += 1
    return out


def swapped_poses(world, agent_of_body, agents, pairs_of_agents, shift=(0.25, 0.125)):
    """A copy of `world` in which, for every (a, b) of pairs_of_agents, agent a's bodies are carried rigidly to where agent b's centroid
    is (plus `shift`) and b's to where a's was, all at rest: the reset poses of the chain tests.  An agent carried onto another agent's
    place leaves what it touched and meets what lies there."""
    out = world_chain.copy_world(world)
    b = out["bodies"]
    centre = {a: world["bodies"]["position"][agent_of_body == a].mean(axis=0).astype(np.float32) for a in range(agents) if (agent_of_body == a).any()}
    for a, other in pairs_of_agents:
        for src, dst in ((a, other), (other, a)):
            rows = agent_of_body == src
            b["position"][rows] = (world["bodies"]["position"][rows] + (centre[dst] - centre[src]) + np.array(shift, dtype=np.float32)).astype(np.float32)
    at_rest = agent_of_body >= 0
    b["linearVelocity"][at_rest] = 0.0
    b["angularVelocity"][at_rest] = 0.0
    return out


def chain_plan(name):
    """(params, world, plan) of a chain world: plan = dict(agent_of_body, agent_of_joint, agents, bodies, joints, seed, resets), where
    `bodies` and `joints` are the reset records and `resets` the two agents of RESET_BEFORE.  The two agents are those with the most
    touching manifolds among the agents whose bodies are all dynamic and not jointed to a static body; each is carried to the other's
    place."""
    params, world = world_chain.golden(name)
    agent_of_body, agent_of_joint, agents = agents_of(world)
    b, j = world["bodies"], world["joints"]
    ok = np.ones(agents, dtype=bool)
    for i in np.flatnonzero(agent_of_body >= 0):
        if b["type"][i] != wire.BODY_DYNAMIC:
            ok[agent_of_body[i]] = False
    for k in np.flatnonzero(j["type"] != wire.JOINT_FREE):
        ends = [int(j["bodyA"][k]), int(j["bodyB"][k])]
        if any(b["type"][e] == wire.BODY_STATIC for e in ends if 0 <= e < len(b)) or j["type"][k] == wire.JOINT_MOUSE:
            for e in ends:
                if 0 <= e < len(b) and agent_of_body[e] >= 0:
                    ok[agent_of_body[e]] = False
    touching = np.where(ok, touching_agents(world, agent_of_body, agents), -1)
    first, second = [int(a) for a in np.argsort(-touching, kind="stable")[:2]]
    assert touching[first] > 0 and touching[second] > 0, (name, touching)
    poses = swapped_poses(world, agent_of_body, agents, [(first, second)])
    bodies, joints = wire.resets_from_world(poses["bodies"], poses["joints"], agent_of_body, agent_of_joint)
    return params, world, dict(agent_of_body=agent_of_body, agent_of_joint=agent_of_joint, agents=agents, bodies=bodies, joints=joints, seed=0x5EED,
                               resets=(first, second))


def marked_by(plan, world, trigger):
    """The body slots a pass with `trigger` marks"""
    out = np.zeros(len(world["bodies"]), dtype=bool)
    for r in plan["bodies"]:
        slot = int(r["body"])
        if trigger[int(r["agent"])] and not int(r["flags"]) & wire.RESET_DISABLED and slot < len(out) and world["bodies"]["type"][slot] not in (wire.BODY_FREE, wire.BODY_STATIC):
            out[slot] = True
    return out


class Conditions:
    """What a chain must have shown, per reset: contacts emptied, pairs of a reset body separated in the step after, pairs found by
    the query behind the reset"""

    def __init__(self):
        self.emptied, self.separated, self.found = [], [], []

    def assert_met(self, what):
        assert len(self.emptied) == len(RESET_BEFORE), what
        assert sum(self.emptied) >= 1 and sum(self.separated) >= 1 and sum(self.found) >= 1, (what, self.emptied, self.separated, self.found)


def oracle_reset(plan, ref, counters, agent):
    """The one-shot reset of one agent on the oracle side -> (counts, marked body slots)"""
    trigger = np.zeros(plan["agents"], dtype=bool)
    trigger[agent] = True
    marked = marked_by(plan, ref, trigger)
    counts = reset_ref.apply(ref, plan["bodies"], plan["joints"], plan["agents"], plan["seed"], trigger, counters)
    return counts, marked


def separated_of(status, contacts_before, marked):
    sep = status == wire.PAIR_SEPARATED
    return int((sep & (marked[contacts_before["bodyA"]] | marked[contacts_before["bodyB"]])).sum())


def oracle_chain(name):
    """The chain on the CPU oracle alone, in the reference's own sweep order -> Conditions"""
    params, world, plan = chain_plan(name)
    ref = world_chain.copy_world(world)
    counters = np.zeros(plan["agents"], dtype=np.int32)
    seen = Conditions()
    marked = None
    for step in range(1, CHAIN_STEPS + 1):
        if step in RESET_BEFORE:
            counts, marked = oracle_reset(plan, ref, counters, plan["resets"][RESET_BEFORE.index(step)])
            seen.emptied.append(int(counts[reset_ref.CONTACTS]))
            new = world_chain.oracle_find_pairs(ref)
            seen.found.append(len(new))
            if len(new):
                world_chain._create_contacts(ref, new)
        before = ref["contacts"].copy()
        status = world_chain.oracle_world_step(params, ref)
        if marked is not None:
            seen.separated.append(separated_of(status, before, marked))
            marked = None
        if world_chain.moved_any(ref):
            new = world_chain.oracle_find_pairs(ref)
            if len(new):
                world_chain._create_contacts(ref, new)
    return seen
