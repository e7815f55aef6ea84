"""The scenes of the sensor-report tests (tests/test_sensor_report_host.py, tests/test_gpu_sensor_report.py), the loader and the
generator of their fixtures tests/golden/sensor_report/*.npz (python -m tests.sensor_report_world, with oracle/liboracle.so and
oracle/_ref/libs2ref.so built).  Test infrastructure only.

Three small worlds, each run for STEPS steps of the oracle chain (tests/world_chain.py) under TGS_Soft:
  ball     a ball dropping through three stacked fixed sensors -- a circle, a rounded box, a segment with a margin -- and carrying a
           pick-up radius of its own past a static marker
  pyramid  a base-3 pyramid at rest with a sensor attached to a brick and one attached to the ground with SKIP_STATIC (a static post
           stands inside it), a fixed box over its top, and a brick without contacts flying through all three
  chain    a chain of six jointed links swung round its anchor through a fixed capsule sensor, the last link carrying a sensor
A fixture holds the world, the sensors and what the statement (tests/sensor_report_ref.py) answers on the chain in pool order: "before"
at the upload and per step the inside lists, both event lists and the states -- settings and results only.  The lists are recorded under
a clearance condition (robust_lists): they are the same with every sensor 1 mm larger and 1 mm smaller, so a chain swept in another
constraint order, whose poses differ in their last bits, has the same lists."""
import os

import numpy as np

from solver2d_amd import synthetic, wire
from tests import common

f32 = np.float32
ALL = 0xFFFFFFFF
STEPS = 12
SCENES = ("ball", "pyramid", "chain")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensor_report")
WORLD_KEYS = ("bodies", "contacts", "joints", "shapes", "pairs", "origins")
CLEARANCE = f32(1e-3)


def params():
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    return wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)


def make_sensor(vertices, radius, position=(0.0, 0.0), angle=0.0, margin=0.0, body=-1, flags=0, mask=ALL):
    q = np.zeros(1, dtype=wire.sensor_dtype)[0]
    q["vertices"][:len(vertices)] = vertices
    q["count"], q["radius"], q["position"] = len(vertices), radius, position
    q["rot"] = (np.sin(angle), np.cos(angle))
    q["margin"], q["maskBits"], q["body"], q["flags"] = margin, mask, body, flags
    return q


def box_vertices(hx, hy):
    return [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)]


def _no_contacts():
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    return contacts, pairs


def _shape(sh, slot, body, body_type, kind, vertices, radius):
    sh["body"], sh["type"] = body, kind
    sh["categoryBits"], sh["maskBits"], sh["groupIndex"] = 1, 0, 0
    sh["proxyKey"] = (slot << 4) | int(body_type)
    sh["count"], sh["radius"] = len(vertices), radius
    sh["vertices"][:len(vertices)] = vertices


def _finish(bodies, contacts, joints, shapes, pairs):
    from tests import oraclebind
    origins = np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()
    oraclebind.refit_shapes(bodies, shapes, origins)
    shapes["enlarged"] = 0
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": shapes, "pairs": pairs, "origins": origins}


def ball_scene():
    bodies = np.zeros(3, dtype=wire.body_dtype)
    synthetic._static_body(bodies[0], 0.0, 0.0)
    synthetic._dynamic_body(bodies[1], 0.0, 5.9, 1.0, 0.5)
    bodies[1]["linearVelocity"] = (0.0, -20.0)
    bodies[2]["type"] = wire.BODY_FREE
    shapes = np.zeros(4, dtype=wire.shape_dtype)
    shapes["type"], shapes["body"] = wire.SHAPE_FREE, -1
    synthetic._box_shape(shapes[0], 0, wire.BODY_STATIC, 5.0, 0.25, 0.0, 0.0, 0)   # the ground
    # a marker beside the ball's path, on the ground's body (the refit leaves static shapes alone: its boxes are made here)
    synthetic._box_shape(shapes[1], 0, wire.BODY_STATIC, 0.1, 0.1, 0.9, 3.5, 1)
    shapes[1]["vertices"][:4] += f32((0.9, 3.5))
    shapes[1]["maskBits"] = 0
    _shape(shapes[3], 3, 1, wire.BODY_DYNAMIC, wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.25)  # the ball (slot 2 is free)
    shapes[0]["maskBits"] = 0
    contacts, pairs = _no_contacts()
    world = _finish(bodies, contacts, np.zeros(0, dtype=wire.joint_dtype), shapes, pairs)
    sensors = np.array([
        make_sensor([(0.0, 0.0)], 0.3, (0.0, 5.0)),                                   # a circle
        make_sensor(box_vertices(0.4, 0.1), 0.1, (0.0, 4.0), angle=0.2),              # a rounded box
        make_sensor([(-0.5, 0.0), (0.5, 0.0)], 0.0, (0.0, 3.0), margin=0.2),          # a segment with a margin
        make_sensor([(0.0, 0.0)], 1.0, (0.0, 0.0), body=1),                           # the ball's pick-up radius: never its own shape
        make_sensor([(0.0, 0.0)], 0.3, (0.0, 5.0), flags=wire.SENSOR_DISABLED),       # the first one again, switched off
        make_sensor([(0.0, 0.0)], 5.0, (0.0, 0.0), body=2),                           # on a free body slot
    ], dtype=wire.sensor_dtype)
    return world, sensors


def pyramid_scene():
    base = synthetic.pyramid_world(3)
    nb = len(base["bodies"])
    bodies = np.zeros(nb + 2, dtype=wire.body_dtype)
    bodies[:nb] = base["bodies"]
    flyer, post = nb, nb + 1
    synthetic._dynamic_body(bodies[flyer], -3.7, 1.5, 1.0, 0.5, gravity_scale=0.0)
    bodies[flyer]["linearVelocity"] = (36.0, 0.0)
    synthetic._static_body(bodies[post], 1.8, 2.6)
    shapes = np.zeros(nb + 2, dtype=wire.shape_dtype)
    shapes[:nb] = base["shapes"]
    synthetic._box_shape(shapes[flyer], flyer, wire.BODY_DYNAMIC, 0.2, 0.2, -3.7, 1.5, flyer)
    synthetic._box_shape(shapes[post], post, wire.BODY_STATIC, 0.1, 0.1, 1.8, 2.6, post)
    shapes["maskBits"][[flyer, post]] = 0  # (no pair is ever made for them: stage 1 is not part of the chain)
    world = _finish(bodies, base["contacts"], base["joints"], shapes, base["pairs"])
    brick = 5  # the middle brick of the second row
    assert bodies[brick]["type"] == wire.BODY_DYNAMIC and abs(float(bodies[brick]["position"][1]) - 1.5) < 1e-6
    sensors = np.array([
        make_sensor([(0.0, 0.0)], 0.7, (0.0, 0.0), body=brick),                                                  # carried by a brick
        make_sensor(box_vertices(2.2, 1.6), 0.0, (0.0, 2.7), body=0, flags=wire.SENSOR_SKIP_STATIC, margin=0.05),  # on the ground
        make_sensor(box_vertices(0.6, 0.4), 0.05, (0.0, 2.6)),                                                   # fixed, over the top brick
        make_sensor(box_vertices(2.2, 1.6), 0.0, (0.0, 2.7), body=0, margin=0.05),                                 # the second, static shapes too
    ], dtype=wire.sensor_dtype)
    return world, sensors


def chain_scene():
    links = 6
    bodies = np.zeros(links + 1, dtype=wire.body_dtype)
    synthetic._static_body(bodies[0], 0.0, 5.0)
    omega = -8.0
    for i in range(1, links + 1):
        synthetic._dynamic_body(bodies[i], 0.8 * i, 5.0, 0.5, 0.05)
        bodies[i]["linearVelocity"], bodies[i]["angularVelocity"] = (0.0, omega * 0.8 * i), omega  # omega x r about the anchor
    joints = np.zeros(links, dtype=wire.joint_dtype)
    for i in range(links):
        j = joints[i]
        j["type"], j["bodyA"], j["bodyB"] = wire.JOINT_REVOLUTE, i, i + 1
        j["localOriginAnchorA"], j["localOriginAnchorB"] = ((0.0, 0.0) if i == 0 else (0.4, 0.0)), ((-0.8, 0.0) if i == 0 else (-0.4, 0.0))
    shapes = np.zeros(links + 1, dtype=wire.shape_dtype)
    _shape(shapes[0], 0, 0, wire.BODY_STATIC, wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.1)
    shapes[0]["aabb"], shapes[0]["fatAABB"] = (-0.12, 4.88, 0.12, 5.12), (-0.2, 4.8, 0.2, 5.2)  # (the refit leaves static shapes alone)
    for i in range(1, links + 1):
        _shape(shapes[i], i, i, wire.BODY_DYNAMIC, wire.SHAPE_CAPSULE, [(-0.3, 0.0), (0.3, 0.0)], 0.08)
    contacts, pairs = _no_contacts()
    world = _finish(bodies, contacts, joints, shapes, pairs)
    sensors = np.array([
        make_sensor([(-1.2, 0.0), (1.2, 0.0)], 0.25, (2.6, 3.1), angle=-0.8),   # a capsule across the swing
        make_sensor([(0.0, 0.0)], 1.0, (0.0, 0.0), body=links),                 # carried by the last link: holds its neighbour
        make_sensor([(0.0, 0.0)], 0.5, (0.0, 4.0), angle=0.5),                  # a circle under the anchor
    ], dtype=wire.sensor_dtype)
    return world, sensors


BUILDERS = {"ball": ball_scene, "pyramid": pyramid_scene, "chain": chain_scene}


def sweep_world(slots):
    """`slots` shape slots, every eleventh one free, for the capacities at which the kernels take another path: a static ground (body 0,
    slot 0), one free body slot (the last), and per live slot a body in free fall on a half-metre lattice sixteen wide -- no contacts, no
    joints --, moving sideways and down at 6 m/s so that every step takes some across the edges of sweep_sensors.  Shape types cycle
    through circle, capsule, box, triangle, rounded octagon and segment.  Column c of the lattice holds slots k = c mod 16: a sensor over
    a few columns holds shapes of every wave of every tile."""
    from tests import shape_report_world
    shapes = np.zeros(slots, dtype=wire.shape_dtype)
    shapes["type"], shapes["body"] = wire.SHAPE_FREE, -1
    body_list = [np.zeros(1, dtype=wire.body_dtype)[0]]
    synthetic._static_body(body_list[0], 4.0, -1.0)
    synthetic._box_shape(shapes[0], 0, wire.BODY_STATIC, 6.0, 0.25, 4.0, -1.0, 0)
    shapes[0]["maskBits"] = 0
    for k in range(1, slots):
        if k % 11 == 5:
            continue
        b = np.zeros(1, dtype=wire.body_dtype)[0]
        synthetic._dynamic_body(b, 0.5 * (k % 16), 1.0 + 0.5 * (k // 16), 1.0, 0.5)
        angle = 0.1 * k
        b["rot"] = (np.sin(angle), np.cos(angle))
        b["linearVelocity"], b["angularVelocity"] = ((6.0 if k % 2 else -6.0), -6.0), 0.5 - 0.01 * (k % 100)
        body_list.append(b)
        kind, verts, radius = shape_report_world._geometry(k % 6)
        _shape(shapes[k], k, len(body_list) - 1, wire.BODY_DYNAMIC, kind, verts, radius)
    free = np.zeros(1, dtype=wire.body_dtype)[0]
    free["type"] = wire.BODY_FREE
    body_list.append(free)
    contacts, pairs = _no_contacts()
    return _finish(np.array(body_list, dtype=wire.body_dtype), contacts, np.zeros(0, dtype=wire.joint_dtype), shapes, pairs)


def sweep_sensors(world, count):
    """`count` sensors that repeat seven distinct ones: a tall fixed box over four lattice columns (every wave of every tile), a fixed
    circle with a margin, one carried by a falling body (its own shape lies inside it), one on the ground with SKIP_STATIC, a DISABLED
    copy of the first, one on the free body slot, and a fixed rounded triangle that passes category 2 only (nothing)."""
    bodies, shapes = world["bodies"], world["shapes"]
    carrier = int(shapes["body"][min(70, len(shapes) - 1)]) if shapes["type"][min(70, len(shapes) - 1)] != wire.SHAPE_FREE else 1
    tall = make_sensor(box_vertices(1.0, 12.0), 0.0, (3.6, 11.0))
    off = tall.copy()
    off["flags"] = wire.SENSOR_DISABLED
    distinct = [
        tall,
        make_sensor([(0.0, 0.0)], 1.0, (2.0, 2.0), margin=0.3),
        make_sensor([(0.0, 0.0)], 0.8, (0.1, 0.0), angle=0.3, body=carrier),
        make_sensor([(-3.0, 1.6), (3.0, 1.6)], 0.4, (0.0, 0.0), body=0, flags=wire.SENSOR_SKIP_STATIC),
        off,
        make_sensor([(0.0, 0.0)], 50.0, (0.0, 0.0), body=len(bodies) - 1),
        make_sensor([(-1.0, -1.0), (1.0, -1.0), (0.0, 1.0)], 0.1, (5.0, 2.0), mask=2),
    ]
    assert bodies["type"][carrier] == wire.BODY_DYNAMIC and bodies["type"][len(bodies) - 1] == wire.BODY_FREE
    return np.array([distinct[i % len(distinct)] for i in range(count)], dtype=wire.sensor_dtype)


def resized(sensors, delta):
    """Every sensor `delta` larger (smaller, for a negative one): by its margin where that stays >= 0, else by its radius"""
    out = sensors.copy()
    for q in out:
        if float(q["margin"]) + delta >= 0.0 and float(q["margin"]) > 0.0:
            q["margin"] = f32(q["margin"]) + f32(delta)
        else:
            assert float(q["radius"]) + delta >= 0.0, "a sensor too small for the clearance condition"
            q["radius"] = f32(q["radius"]) + f32(delta)
    return out


def robust_lists(world, sensors):
    """The statement's inside lists, asserted to be those of the sensors CLEARANCE larger and smaller as well"""
    from tests import sensor_report_ref as ref
    lists = ref.inside_lists(world, sensors)
    assert lists == ref.inside_lists(world, resized(sensors, float(CLEARANCE))) == ref.inside_lists(world, resized(sensors, -float(CLEARANCE))), \
        "a shape within %g of a sensor's boundary: move the scene" % CLEARANCE
    return lists


def run_statement(world, sensors, steps=STEPS, robust=True):
    """The chain in pool order -> fixture entries: before_*, and per step k inside_offsets_k, inside_shapes_k, entered_k, left_k, states_k"""
    from tests import sensor_report_ref as ref, world_chain
    lists_of = robust_lists if robust else ref.inside_lists
    w = world_chain.copy_world(world)
    before = lists_of(w, sensors)
    out = {}
    out["before_offsets"], out["before_shapes"] = ref.csr(before)
    p = params()
    for k in range(steps):
        world_chain.oracle_world_step(p, w)
        now = lists_of(w, sensors)
        out["inside_offsets_%d" % k], out["inside_shapes_%d" % k] = ref.csr(now)
        out["entered_%d" % k], out["left_%d" % k] = ref.events(before, now, w, sensors)
        out["states_%d" % k] = ref.states(w, sensors, before, now)
        before = now
    return out


def fixture_path(name):
    return os.path.join(GOLDEN, "%s.npz" % name)


def load_fixture(name):
    d = np.load(fixture_path(name))
    return {k: np.ascontiguousarray(d[k]) for k in d.files}


def fixture_world(fx):
    return {k: fx[k].copy() for k in WORLD_KEYS}


def fixture_lists(fx, key, step=None):
    """The recorded inside lists: key "before", or "inside" with a step"""
    from tests import sensor_report_ref as ref
    suffix = "" if step is None else "_%d" % step
    return ref.from_csr(fx["%s_offsets%s" % (key, suffix)], fx["%s_shapes%s" % (key, suffix)])


def condition(fx):
    """What every scene must show by the statement alone: (entered events, left events, inside entries of fixed sensors, inside entries
    of attached sensors, steps without any event)"""
    sensors = fx["sensors"]
    entered = sum(len(fx["entered_%d" % k]) for k in range(STEPS))
    left = sum(len(fx["left_%d" % k]) for k in range(STEPS))
    fixed = attached = 0
    for k in range(STEPS):
        counts = np.diff(fx["inside_offsets_%d" % k])
        fixed += int(counts[sensors["body"] < 0].sum())
        attached += int(counts[sensors["body"] >= 0].sum())
    quiet = sum(1 for k in range(STEPS) if len(fx["entered_%d" % k]) + len(fx["left_%d" % k]) == 0)
    return entered, left, fixed, attached, quiet


def assert_condition(fx, what):
    got = condition(fx)
    assert all(x >= 1 for x in got), "%s: (entered, left, fixed inside, attached inside, quiet steps) = %r" % (what, got)


def build_fixture(name):
    world, sensors = BUILDERS[name]()
    fx = {k: world[k] for k in WORLD_KEYS}
    fx["sensors"] = sensors
    fx.update(run_statement(world, sensors))
    return fx


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for scene in SCENES:
        built = build_fixture(scene)
        assert_condition(built, scene)
        np.savez_compressed(fixture_path(scene), **built)
        print("%s: %d sensors, (entered, left, fixed inside, attached inside, quiet steps) = %r, per step %s, %d bytes" % (
            scene, len(built["sensors"]), condition(built),
            [(len(built["entered_%d" % k]), len(built["left_%d" % k]), len(built["inside_shapes_%d" % k])) for k in range(STEPS)],
            os.path.getsize(fixture_path(scene))))
