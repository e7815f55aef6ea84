"""The statement of the resets (include/solver2d_amd.h: s2amd_world_set_resets, s2amd_world_set_reset_report,
s2amd_world_reset_agents, s2amd_world_reset_states, s2amd_world_reset_counts), restated in numpy for the tests.  Test infrastructure only.

A pass takes a world (the six wire arrays of tests/world_chain.py), the two record lists, one trigger per agent and the agents' `resets`
counters, and writes the world in place: steps 1 to 7 of the header, one after another.  Every product and sum of the jitter is a float32
scalar rounded on its own.  The box arithmetic of step 4 and the origin of step 3 are the CPU oracle's refit (oraclebind.refit_shapes) on
a copy of the world that holds the new poses: the tight box and the origin are what stage 4 computes, and the fat box is the tight box
-+ AABB_MARGIN whatever the old one held."""
import numpy as np

from solver2d_amd import synthetic, wire
from tests import oraclebind

F = np.float32
U = np.uint32
AGENTS, BODIES, BODIES_SKIPPED, JOINTS, JOINTS_SKIPPED, SHAPES, CONTACTS, SOURCE_OFF = range(8)


def fmix32(k):
    """MurmurHash3's finaliser on a Python integer, modulo 2^32"""
    k = int(k) & 0xFFFFFFFF
    k ^= k >> 16
    k = (k * 0x85EBCA6B) & 0xFFFFFFFF
    k ^= k >> 13
    k = (k * 0xC2B2AE35) & 0xFFFFFFFF
    k ^= k >> 16
    return k


def jitter_terms(seed, k, c, n):
    """-> (h, u, t) of component c of record k at the agent's n-th reset: u = (h >> 8) * 2^-24 in [0, 1), t = 2 u - 1 in [-1, 1), exact"""
    seed, k, c, n = int(seed), int(k), int(c), int(n)
    h = fmix32(seed + 0x9E3779B9 * ((8 * k + c) & 0xFFFFFFFF))
    h = fmix32(h ^ (n & 0xFFFFFFFF))
    u = F(F(h >> 8) * F(2.0 ** -24))
    t = F(F(2.0) * u - F(1.0))
    return h, u, t


def jittered(base, jitter, seed, k, c, n):
    """base + t * jitter, one multiply and one add; the base's own bits when the jitter is 0"""
    base, jitter = F(base), F(jitter)
    if jitter == 0:
        return base
    t = jitter_terms(seed, k, c, n)[2]
    with np.errstate(all="ignore"):
        return F(base + F(t * jitter))


def valid(bodies, joints, agents):
    """What the host checks before anything is replaced: None, or ("call" | "body" | "joint", index of the first invalid record)"""
    if not 0 <= agents <= wire.MAX_RESET_AGENTS or len(bodies) > wire.MAX_RESET_BODIES or len(joints) > wire.MAX_RESET_JOINTS:
        return "call", 0
    if (len(bodies) or len(joints)) and agents == 0:
        return "call", 0
    floats = ("position", "rot", "linearVelocity", "angularVelocity", "positionJitter", "velocityJitter", "angularJitter")
    for i, r in enumerate(bodies):
        if not 0 <= r["agent"] < agents or r["body"] < 0 or int(r["flags"]) & ~wire.RESET_DISABLED or r["reserved"] != 0:
            return "body", i
        if not all(np.isfinite(r[name]).all() for name in floats):
            return "body", i
        if not (np.all(r["positionJitter"] >= 0) and np.all(r["velocityJitter"] >= 0) and r["angularJitter"] >= 0):
            return "body", i
    for i, r in enumerate(joints):
        if not 0 <= r["agent"] < agents or r["joint"] < 0 or int(r["flags"]) & ~(wire.RESET_DISABLED | wire.RESET_JOINT_SETTINGS):
            return "joint", i
        if not (np.isfinite(r["motorSpeed"]) and np.isfinite(r["targetA"]).all()):
            return "joint", i
    for what, slots in (("body", bodies["body"]), ("joint", joints["joint"])):
        seen = set()
        for i, slot in enumerate(slots.tolist()):
            if slot in seen:
                return what, i
            seen.add(slot)
    return None


def episode_trigger(flags, agents):
    """The trigger of a step: episode flags & 3, 0 for the agents beyond the episode list's; None (the episode pass did not run): nobody"""
    out = np.zeros(agents, dtype=bool)
    if flags is not None:
        n = min(agents, len(flags))
        out[:n] = (np.asarray(flags[:n]) & 3) != 0
    return out


def apply(world, bodies, joints, agents, seed, trigger, resets):
    """One pass, in place on `world` and on `resets` (int32[agents]); -> counts int32[8] (counts[SOURCE_OFF] is the caller's: a step
    whose episode pass did not run calls nothing and reports [0] * 7 + [1])."""
    trigger = np.asarray(trigger, dtype=bool)
    assert len(trigger) == agents and len(resets) == agents
    wb, wj, ws, wc, wp = world["bodies"], world["joints"], world["shapes"], world["contacts"], world["pairs"]
    counts = np.zeros(8, dtype=np.int32)
    marked = np.zeros(len(wb), dtype=bool)
    # 1, 2: the body records
    for k, r in enumerate(bodies):
        a = int(r["agent"])
        if not trigger[a] or int(r["flags"]) & wire.RESET_DISABLED:
            continue
        slot = int(r["body"])
        if slot >= len(wb) or wb["type"][slot] in (wire.BODY_FREE, wire.BODY_STATIC):
            counts[BODIES_SKIPPED] += 1
            continue
        n = int(resets[a])
        b = wb[slot]
        b["position"] = [jittered(r["position"][c], r["positionJitter"][c], seed, k, c, n) for c in range(2)]
        b["rot"] = r["rot"]
        b["linearVelocity"] = [jittered(r["linearVelocity"][c], r["velocityJitter"][c], seed, k, 2 + c, n) for c in range(2)]
        b["angularVelocity"] = jittered(r["angularVelocity"], r["angularJitter"], seed, k, 4, n)
        b["deltaPosition"], b["force"], b["torque"] = 0.0, 0.0, 0.0
        marked[slot] = True
        counts[BODIES] += 1
    # 3, 4: origins and boxes of the marked bodies, from the oracle's stage 4 on a copy that holds the new poses
    if marked.any():
        shapes, origins = ws.copy(), np.ascontiguousarray(world["origins"], dtype=F).copy()
        oraclebind.refit_shapes(wb.copy(), shapes, origins)
        world["origins"] = np.ascontiguousarray(world["origins"], dtype=F)
        world["origins"].reshape(-1, 2)[marked] = origins.reshape(-1, 2)[marked]
        live = (ws["type"] != wire.SHAPE_FREE) & (ws["body"] >= 0) & (ws["body"] < len(wb))
        moved = live & marked[np.clip(ws["body"], 0, len(wb) - 1)]
        margin = F(synthetic.AABB_MARGIN)
        ws["aabb"][moved] = shapes["aabb"][moved]
        tight = shapes["aabb"][moved]
        ws["fatAABB"][moved] = np.stack([tight[:, 0] - margin, tight[:, 1] - margin, tight[:, 2] + margin, tight[:, 3] + margin], axis=1).astype(F)
        ws["enlarged"][moved] = 1
        counts[SHAPES] = int(moved.sum())
        # 5: the contacts of the marked bodies, as s2CreateContact leaves one
        def is_marked(index):
            inside = (index >= 0) & (index < len(wb))
            return inside & marked[np.clip(index, 0, len(wb) - 1)]

        empty = (wp["shapeA"] >= 0) & (is_marked(wc["bodyA"]) | is_marked(wc["bodyB"]))
        for i in np.flatnonzero(empty):
            kept = wc[i].copy()
            wc[i] = np.zeros(1, dtype=wire.contact_dtype)[0]
            for name in ("bodyA", "bodyB", "friction", "constraintIndex"):
                wc[name][i] = kept[name]
            pair = (int(wp["shapeA"][i]), int(wp["shapeB"][i]))
            wp[i] = np.zeros(1, dtype=wire.pair_state_dtype)[0]
            wp["shapeA"][i], wp["shapeB"][i] = pair
        counts[CONTACTS] = int(empty.sum())
    # 6: the joint records
    for r in joints:
        a = int(r["agent"])
        if not trigger[a] or int(r["flags"]) & wire.RESET_DISABLED:
            continue
        slot = int(r["joint"])
        if slot >= len(wj) or wj["type"][slot] == wire.JOINT_FREE:
            counts[JOINTS_SKIPPED] += 1
            continue
        j = wj[slot]
        j["impulse"], j["motorImpulse"], j["lowerImpulse"], j["upperImpulse"] = 0.0, 0.0, 0.0, 0.0
        if int(r["flags"]) & wire.RESET_JOINT_SETTINGS:
            if j["type"] == wire.JOINT_REVOLUTE:
                j["enableMotor"], j["enableLimit"], j["motorSpeed"] = r["enableMotor"], r["enableLimit"], r["motorSpeed"]
            elif j["type"] == wire.JOINT_MOUSE:
                j["targetA"] = r["targetA"]
        counts[JOINTS] += 1
    # 7
    resets[trigger] += 1
    counts[AGENTS] = int(trigger.sum())
    return counts
