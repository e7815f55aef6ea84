"""The synthetic world of the body-report tests (tests/test_body_report_host.py checks it on the CPU, tests/test_gpu_body_report.py runs it
on the device): the smallest input that crosses the wave and tile boundaries of solver2d_amd/csrc/body_report.hip.  Test infrastructure
only.

640 body slots (three tiles of 256, the last one half full), every sixteenth one free, on a lattice 4 m apart; nothing collides
(maskBits = 0), so there are no contacts and every solver moves a free body alike.  Slot 0 is static, slot 1 kinematic.  Revolute chains:
two from the static body and two from the kinematic one (four islands, not one), one across slots 63/64 (a wave boundary), one across
255/256 (a tile boundary), one that alternates between low and high slots of all three tiles, and a hub (slot 400) with 70 spokes below
and above it.  A dynamic body without mass (slot 12) sits between two chains and joins nothing; a mouse joint holds slot 17 and joins
nothing.  In every tile: bodies with gravityScale 0 and no velocity, which never move; bodies that start at rest under 0.9 g, which under
THRESHOLDS are at rest after step 3 and awake after step 4; bodies without gravity whose damping takes them down through the threshold."""
import numpy as np

from solver2d_amd import synthetic, wire
from tests import body_report_ref, oraclebind

SLOTS = 640
DT = np.float32(1.0 / 60.0)
THRESHOLDS = (np.float32(0.5), np.float32(1.745), np.float32(3) * DT)
STATIC, KINEMATIC, MASSLESS, MOUSE_HELD, HUB = 0, 1, 12, 17, 400
CHAINS = ([STATIC, 2, 3, 4], [STATIC, 5, 6], [KINEMATIC, 8, 10], [KINEMATIC, 11, 18], [13, 14, MASSLESS, 15, 16], [61, 62, 63, 64, 65, 66],
          [253, 254, 255, 256, 257, 258], [70, 300, 72, 560, 74, 302, 76, 562])
SPOKES = [i for i in range(326, 366) if i % 16 != 9][:35] + [i for i in range(418, 458) if i % 16 != 9][:35]
STILL = [i for r in (range(100, 116), range(268, 284), range(520, 536)) for i in r if i % 16 != 9]
DROPPED = [i for r in (range(120, 136), range(284, 298), range(540, 556)) for i in r if i % 16 != 9]
DAMPED = [i for r in (range(140, 152), range(306, 318), range(570, 580)) for i in r if i % 16 != 9]


def is_free(slot):
    return slot % 16 == 9


def synthetic_world():
    bodies = np.zeros(SLOTS, dtype=wire.body_dtype)
    bodies["type"] = wire.BODY_FREE
    for i in range(SLOTS):
        if is_free(i):
            continue
        b = bodies[i]
        x, y = 4.0 * (i % 32), 20.0 + 4.0 * (i // 32)
        if i == STATIC:
            synthetic._static_body(b, x, y)
            continue
        synthetic._dynamic_body(b, x, y, 1.0, 0.5)
        angle = 0.1 * i
        b["rot"] = (np.sin(angle), np.cos(angle))
        b["linearVelocity"], b["angularVelocity"] = (1.0 + 0.01 * (i % 50), 0.0), 0.5 - 0.01 * (i % 100)
    k = bodies[KINEMATIC]
    k["type"], k["mass"], k["invMass"], k["I"], k["invI"] = wire.BODY_KINEMATIC, 0.0, 0.0, 0.0, 0.0
    k["linearVelocity"], k["angularVelocity"] = (0.5, 0.0), 0.0
    m = bodies[MASSLESS]
    m["mass"], m["invMass"], m["I"], m["invI"], m["gravityScale"] = 0.0, 0.0, 0.0, 0.0, 0.0
    m["linearVelocity"], m["angularVelocity"] = (0.0, 0.0), 0.0
    for i in STILL:
        bodies[i]["gravityScale"], bodies[i]["linearVelocity"], bodies[i]["angularVelocity"] = 0.0, (0.0, 0.0), 0.0
    for i in DROPPED:
        bodies[i]["gravityScale"], bodies[i]["linearVelocity"], bodies[i]["angularVelocity"] = 0.9, (0.0, 0.0), 0.0
    for n, i in enumerate(DAMPED):
        b = bodies[i]
        b["gravityScale"], b["linearDamping"], b["angularVelocity"] = 0.0, 5.0, 0.0
        b["linearVelocity"] = (0.52 + 0.02 * (n % 9), 0.0)

    links = [(a, b) for chain in CHAINS for a, b in zip(chain, chain[1:])] + [(HUB, spoke) for spoke in SPOKES]
    joints = np.zeros(len(links) + len(links) // 4 + 8, dtype=wire.joint_dtype)
    joints["type"] = wire.JOINT_FREE
    joints["bodyA"] = joints["bodyB"] = -1
    slot = 0
    for a, b in links:
        if slot % 5 == 3:
            slot += 1  # a free joint slot
        j = joints[slot]
        slot += 1
        # the joint sits half way between the two bodies as they start: anchors in the bodies' own frames (s2InvRotateVector)
        half = (bodies[b]["position"] - bodies[a]["position"]) * np.float32(0.5)
        (sa, ca), (sb, cb) = bodies[a]["rot"], bodies[b]["rot"]
        j["type"], j["bodyA"], j["bodyB"] = wire.JOINT_REVOLUTE, a, b
        j["localOriginAnchorA"] = (ca * half[0] + sa * half[1], -sa * half[0] + ca * half[1])
        j["localOriginAnchorB"] = (-(cb * half[0] + sb * half[1]), -(-sb * half[0] + cb * half[1]))
    mouse = joints[len(joints) - 2]
    mouse["type"], mouse["bodyA"], mouse["bodyB"] = wire.JOINT_MOUSE, STATIC, MOUSE_HELD
    mouse["targetA"], mouse["hertz"], mouse["dampingRatio"] = bodies[MOUSE_HELD]["position"] + np.float32(1.0), 5.0, 0.7

    shapes = np.zeros(SLOTS, dtype=wire.shape_dtype)
    shapes["type"], shapes["body"] = wire.SHAPE_FREE, -1
    for i in range(SLOTS):
        if not is_free(i):
            b = bodies[i]
            synthetic._box_shape(shapes[i], i, b["type"], 0.125, 0.125, b["position"][0], b["position"][1], i)
    shapes["maskBits"] = 0
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    origins = np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()
    oraclebind.refit_shapes(bodies, shapes, origins)
    shapes["enlarged"] = 0
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": shapes, "pairs": pairs, "origins": origins}


def assert_world_is_what_it_says(world):
    bodies, joints = world["bodies"], world["joints"]
    special = [s for chain in CHAINS for s in chain] + SPOKES + STILL + DROPPED + DAMPED + [HUB, MOUSE_HELD]
    assert len(bodies) >= 600 and not any(is_free(s) for s in special)
    named = [s for chain in CHAINS for s in chain if s not in (STATIC, KINEMATIC)] + SPOKES + STILL + DROPPED + DAMPED + [HUB, MOUSE_HELD]
    assert len(named) == len(set(named))  # no slot plays two parts
    free = bodies["type"] == wire.BODY_FREE
    for t in (0, 256, 512):
        assert free[t:t + 256].any() and (~free[t:t + 256]).any()
        reported = int(((bodies["type"][t:t + 256] != wire.BODY_FREE) & (bodies["type"][t:t + 256] != wire.BODY_STATIC)).sum())
        assert reported % 64 != 0, (t, reported)
        for group in (STILL, DROPPED):
            assert sum(1 for s in group if t <= s < t + 256) >= 10
        assert sum(1 for s in DAMPED if t <= s < t + 256) >= 5
    assert bodies["type"][STATIC] == wire.BODY_STATIC and bodies["type"][KINEMATIC] == wire.BODY_KINEMATIC
    assert bodies["type"][MASSLESS] == wire.BODY_DYNAMIC and bodies["invMass"][MASSLESS] == 0 and bodies["invI"][MASSLESS] == 0
    assert len(SPOKES) == 70 and min(SPOKES) < HUB < max(SPOKES) and sum(1 for s in SPOKES if s < HUB) == 35
    revolute = joints[joints["type"] == wire.JOINT_REVOLUTE]
    assert int((revolute["bodyA"] == HUB).sum()) == 70 and int((joints["type"] == wire.JOINT_MOUSE).sum()) == 1
    assert (joints["type"] == wire.JOINT_FREE).sum() >= 8 and (world["pairs"]["shapeA"] < 0).all()
    live = world["shapes"]["type"] != wire.SHAPE_FREE
    assert (world["shapes"]["maskBits"][live] == 0).all()


def expected_islands():
    """The islands the chains, the hub and the separators make, as sets of slots (every other reported body is alone)"""
    groups = [{2, 3, 4}, {5, 6}, {8, 10}, {11, 18}, {13, 14}, {15, 16}, {61, 62, 63, 64, 65, 66}, {253, 254, 255, 256, 257, 258},
              {70, 300, 72, 560, 74, 302, 76, 562}, {HUB} | set(SPOKES)]
    return groups


def thresholds_of(linear, dt):
    return (np.float32(linear), np.float32(np.float32(linear) * np.float32(3.4906585)), np.float32(3) * np.float32(dt))


def assert_records_equal(got, want, what):
    assert len(got) == len(want), "%s: %d records, reference %d" % (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: records differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))


def assert_body_report_equals_reference(s, state, world, thresholds, dt, what, flags=wire.BODY_REPORT_ALL, totals=None):
    """The four getters against the reference statement on `world` (the oracle chain after the step); `state` moves on by one step."""
    step = body_report_ref.advance(state, world, thresholds, dt)
    island = island_states = None
    if flags & wire.BODY_REPORT_ISLANDS:
        island, island_states = body_report_ref.islands(world, step)
        assert_records_equal(s.world_islands(expected=max(len(island_states), 1)), island_states, what + ": islands")
    if flags & wire.BODY_REPORT_STATES:
        want = body_report_ref.states(world, step, bool(flags & wire.BODY_REPORT_MOVED_ONLY), island, island_states)
        assert_records_equal(s.world_body_states(expected=max(len(want), 1)), want, what + ": states")
    if flags & wire.BODY_REPORT_REST:
        want_rested, want_woke = body_report_ref.events(step)
        rested, woke = s.world_body_rest_events()
        assert rested.tolist() == want_rested.tolist(), what + ": rested"
        assert woke.tolist() == want_woke.tolist(), what + ": woke"
    want_summary = body_report_ref.summary(world, step, island_states)
    summary = s.world_body_summary()
    assert summary.tobytes() == want_summary.tobytes(), "%s: summary %s, reference %s" % (what, summary, want_summary)
    if totals is not None:
        # (counted on the reference chain of the run)
        rested, woke = body_report_ref.events(step)
        totals["rested"] += len(rested)
        totals["woke"] += len(woke)
        totals["rested_high"] += int((rested >= 256).sum())
        totals["woke_high"] += int((woke >= 256).sum())
        totals["records"] += int(step["reported"].sum())
        totals["unmoved"] += int((step["reported"] & ~step["moved"]).sum())
        totals["last_moved"] = step["moved"]
        if island_states is not None:
            totals["islands"].append(len(island_states))
            totals["largest"] = max(totals["largest"], int(island_states["bodyCount"].max()) if len(island_states) else 0)
            low = set(island[:256][island[:256] >= 0].tolist())
            totals["spanning"] = max(totals["spanning"], len(low & set(island[256:][island[256:] >= 0].tolist())))
    return step
