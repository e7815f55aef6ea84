"""The synthetic world of the shape-report tests (tests/test_shape_report_host.py checks it on the CPU, tests/test_gpu_shape_report.py
runs it on the device): the smallest input that crosses both kernel boundaries of solver2d_amd/csrc/shape_report.hip.  Test
infrastructure only.

331 shape slots (two tiles of 256), every eleventh one free; a static ground inside the view; bodies in free fall, no contacts (nothing
collides: maskBits = 0) and no joints, in four families that cross the edges of VIEW during 12 steps of 1/60 s: down through the lower
edge, down through the upper edge, out through the right edge, in through the left edge, each family staggered over seven start
positions.  Shape types cycle through circle, capsule, box, triangle, rounded octagon and segment; one dynamic body has mass 0; one body
carries two shapes (slots 12 and 330)."""
import numpy as np

from solver2d_amd import synthetic, wire
from tests import oraclebind

VIEW = (-4.0, 0.0, 4.0, 8.0)
SLOTS = 331
BAD_SLOT, TWIN_OF, TWIN_SLOT = 8, 12, 330
f32 = np.float32


def _ngon(n, r):
    ang = 2.0 * np.pi * np.arange(n) / n
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).astype(f32)


def _geometry(kind):
    """(type, vertices, radius) -- every shape stays within 0.25 of its body's origin"""
    if kind == 0:
        return wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.25
    if kind == 1:
        return wire.SHAPE_CAPSULE, [(-0.125, 0.0), (0.125, 0.0)], 0.125
    if kind == 2:
        return wire.SHAPE_POLYGON, [(-0.2, -0.125), (0.2, -0.125), (0.2, 0.125), (-0.2, 0.125)], 0.0
    if kind == 3:
        return wire.SHAPE_POLYGON, _ngon(3, 0.25), 0.0
    if kind == 4:
        return wire.SHAPE_POLYGON, _ngon(8, 0.1875), 0.0625
    return wire.SHAPE_SEGMENT, [(-0.25, 0.0), (0.25, 0.0)], 0.0


def synthetic_world():
    shapes = np.zeros(SLOTS, dtype=wire.shape_dtype)
    shapes["type"], shapes["body"] = wire.SHAPE_FREE, -1
    body_list = []

    def new_body():
        body_list.append(np.zeros(1, dtype=wire.body_dtype)[0])
        return len(body_list) - 1, body_list[-1]

    def put_shape(slot, body, kind):
        sh = shapes[slot]
        t, verts, radius = _geometry(kind)
        sh["body"], sh["type"] = body, t
        sh["categoryBits"], sh["maskBits"], sh["groupIndex"] = 1, 0, 0
        sh["proxyKey"] = (slot << 4) | int(body_list[body]["type"])
        sh["count"], sh["radius"] = len(verts), radius
        sh["vertices"][:len(verts)] = verts

    _, ground = new_body()
    synthetic._static_body(ground, 0.0, 0.5)
    synthetic._box_shape(shapes[0], 0, wire.BODY_STATIC, 3.0, 0.125, 0.0, 0.5, 0)
    shapes[0]["maskBits"] = 0
    body_of_slot = {}
    for k in range(1, SLOTS - 1):
        if k % 11 == 5:
            continue  # a free slot
        i, b = new_body()
        body_of_slot[k] = i
        family, stagger = k % 4, 0.05 * (k % 7)
        spread = -3.0 + 6.0 * ((k * 37) % 101) / 100.0
        if family == 0:    # leaves through the lower edge
            x, y, vx, vy = spread, 0.1 + stagger, 0.25, -4.0
        elif family == 1:  # enters through the upper edge
            x, y, vx, vy = spread, 8.4 + stagger, -0.25, -4.0
        elif family == 2:  # leaves through the right edge
            x, y, vx, vy = 3.7 + stagger, 4.0 + 0.5 * spread, 4.0, 0.0
        else:              # enters through the left edge
            x, y, vx, vy = -4.4 - stagger, 4.0 + 0.5 * spread, 4.0, 0.0
        synthetic._dynamic_body(b, x, y, 1.0, 0.5)
        angle = 0.1 * k
        b["rot"] = (np.sin(angle), np.cos(angle))
        b["linearVelocity"], b["angularVelocity"] = (vx, vy), 0.5 - 0.01 * (k % 100)
        if k == BAD_SLOT:
            # (at rest in the middle of the view: a dynamic body without mass is s2World_Draw's "bad body", not a case of the solvers)
            b["mass"], b["invMass"], b["I"], b["invI"] = 0.0, 0.0, 0.0, 0.0
            b["position"], b["linearVelocity"], b["angularVelocity"], b["gravityScale"] = (0.0, 4.0), (0.0, 0.0), 0.0, 0.0
        put_shape(k, i, k % 6)
    put_shape(TWIN_SLOT, body_of_slot[TWIN_OF], 0)
    shapes[TWIN_SLOT]["vertices"][0] = (0.125, 0.0)
    shapes[TWIN_SLOT]["radius"] = 0.125
    bodies = np.array(body_list, dtype=wire.body_dtype)
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    origins = np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()
    oraclebind.refit_shapes(bodies, shapes, origins)
    shapes["enlarged"] = 0
    return {"bodies": bodies, "contacts": contacts, "joints": np.zeros(0, dtype=wire.joint_dtype), "shapes": shapes, "pairs": pairs, "origins": origins}


def assert_world_is_what_it_says(world):
    shapes, bodies = world["shapes"], world["bodies"]
    live = shapes["type"] != wire.SHAPE_FREE
    assert len(shapes) > 256 and live[:256].any() and live[256:].any() and (~live[:256]).any() and (~live[256:]).any()
    polygons = shapes[live & (shapes["type"] == wire.SHAPE_POLYGON)]
    assert {3, 8} <= set(polygons["count"].tolist()) and (polygons["radius"] > 0).any()
    assert set(shapes["type"][live].tolist()) == {0, 1, 2, 3}
    bad = (bodies["type"] == wire.BODY_DYNAMIC) & (bodies["mass"] == 0)
    assert int(bad.sum()) == 1 and int(bad[shapes["body"][BAD_SLOT]]) == 1
    assert int(np.bincount(shapes["body"][live]).max()) == 2
    assert (world["pairs"]["shapeA"] < 0).all() and len(world["joints"]) == 0
    assert np.isfinite(shapes["aabb"][live]).all() and (shapes["aabb"][live][:, 2] > shapes["aabb"][live][:, 0]).all()
