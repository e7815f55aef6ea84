"""The statement of the force fields (include/solver2d_amd.h: s2amd_world_apply_fields, s2amd_world_set_fields,
s2amd_world_field_states), restated for the tests.  Test infrastructure only.

Active, the world transform and the candidate box are the sensor report's (tests/sensor_report_ref.py, `margin` read as `range`); the
scale, the magnitude and the three directions are numpy float32 scalar by scalar, every product, quotient and sum rounded on its own;
a term is applied through tests/world_edit_ref.apply, the statement of the two setters; the distance is the reference's OWN
s2ShapeDistance through tests/proximity_ref.py, so apply() needs oracle/_ref/libs2ref.so -- unless it is given the recorded distance
outputs of a fixture (tests/golden/force_fields/*.npz: record(), load_fixture()).  A world is a dict with "shapes", "bodies" and
"origins" (the keys of tests/world_chain.py); fields are wire.field_dtype records."""
import os

import numpy as np

from solver2d_amd import wire
from tests import proximity_ref, sensor_report_ref, world_edit_ref
from tests.scene_query_ref import _candidates

F = np.float32
available = proximity_ref.available
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "force_fields")
NORMALIZE_EPS = F(0.001) * F(1.19209290e-07)


def is_active(world, f):
    body = int(f["body"])
    if int(f["flags"]) & wire.FIELD_DISABLED:
        return False
    return body < 0 or (body < len(world["bodies"]) and int(world["bodies"]["type"][body]) != wire.BODY_FREE)


def as_query(world, f):
    """The active field as the proximity query it evaluates: its proxy under the world transform, maxDistance = range"""
    out = np.zeros(1, dtype=wire.proximity_query_dtype)[0]
    out["vertices"], out["count"], out["radius"] = f["vertices"], f["count"], f["radius"]
    out["maxDistance"], out["maskBits"] = f["range"], f["maskBits"]
    body = int(f["body"])
    if body < 0:
        out["position"], out["rot"] = f["position"], f["rot"]
    else:
        out["position"], out["rot"] = sensor_report_ref.mul_transforms(world["origins"][body], world["bodies"]["rot"][body], f["position"], f["rot"])
    return out


def poses(world, fields):
    """wire.field_state_dtype with field, body, active, the transform and the box; terms zero and lowestShape -1"""
    out = np.zeros(len(fields), dtype=wire.field_state_dtype)
    out["lowestShape"] = -1
    for i, f in enumerate(fields):
        out[i]["field"], out[i]["body"] = i, f["body"]
        if is_active(world, f):
            pq = as_query(world, f)
            out[i]["active"], out[i]["position"], out[i]["rot"] = 1, pq["position"], pq["rot"]
            out[i]["box"] = proximity_ref.query_box(pq)
    return out


def normalize(x, y):
    """s2Normalize, src/math.c:41-52: the zero vector below the length threshold"""
    x, y = F(x), F(y)
    length = F(np.sqrt(F(F(x * x) + F(y * y))))
    if length < NORMALIZE_EPS:
        return F(0.0), F(0.0)
    inv = F(F(1.0) / length)
    return F(inv * x), F(inv * y)


def candidates(world, f):
    """The candidate slots of an active field, ascending"""
    shapes, bodies = world["shapes"], world["bodies"]
    pq = as_query(world, f)
    out = []
    for slot in _candidates(shapes, proximity_ref.query_box(pq), f["maskBits"]):
        body = int(shapes["body"][slot])
        if body != int(f["body"]) and int(bodies["type"][body]) == wire.BODY_DYNAMIC:
            out.append(int(slot))
    return out


def distance(world, f, slot):
    """(distance, pointB.x, pointB.y) of D(field, slot) from the compiled reference"""
    pq = as_query(world, f)
    sh = world["shapes"][slot]
    body = int(sh["body"])
    d = proximity_ref.shape_distance(proximity_ref.make_proxy(pq["vertices"], int(pq["count"]), pq["radius"]), proximity_ref.transform(pq["position"], pq["rot"]),
                                     proximity_ref.shape_proxy(sh), proximity_ref.transform(world["origins"][body], world["bodies"]["rot"][body]))
    return F(d.distance), F(d.pointB.x), F(d.pointB.y)


def term(f, centre, d, point_b, body_record):
    """One term as the s2amd_world_edit record it is: (f, s) with D = (d, point_b) within reach, on the body record as it stands"""
    flags, kind, rng = int(f["flags"]), int(f["kind"]), F(f["range"])
    scale = F(1.0)
    if (flags & wire.FIELD_LINEAR_FALLOFF) and rng > 0:
        scale = F(F(1.0) - F(F(d) / rng))
    m = F(F(f["strength"]) * scale)
    point = (F(body_record["position"][0]), F(body_record["position"][1]))
    if kind == wire.FIELD_RADIAL:
        nx, ny = normalize(F(point_b[0] - F(centre[0])), F(point_b[1] - F(centre[1])))
        g = (F(m * nx), F(m * ny))
        point = point_b
    elif kind == wire.FIELD_UNIFORM:
        g = (F(m * F(f["direction"][0])), F(m * F(f["direction"][1])))
    else:
        assert kind == wire.FIELD_DRAG
        nm = F(-m)
        g = (F(nm * F(body_record["linearVelocity"][0])), F(nm * F(body_record["linearVelocity"][1])))
    return g, point


def apply(world, fields, recorded=None, record_into=None):
    """-> (bodies after, states, the terms as one wire.world_edit_dtype list in the order they were applied).  `world` is not changed.
    recorded: {(field, slot): (distance, pointB.x, pointB.y)} instead of the compiled reference; record_into: a dict that receives
    exactly that for every candidate."""
    bodies = world["bodies"].copy()
    no_joints = np.zeros(0, dtype=wire.joint_dtype)
    states = poses(world, fields)
    edits = []
    with np.errstate(all="ignore"):
        for i, f in enumerate(fields):
            if not is_active(world, f):
                continue
            centre = (F(states[i]["position"][0]), F(states[i]["position"][1]))
            for slot in candidates(world, f):
                d, bx, by = recorded[(i, slot)] if recorded is not None else distance(world, f, slot)
                if record_into is not None:
                    record_into[(i, slot)] = (d, bx, by)
                if not F(d) <= F(f["range"]):
                    continue
                body = int(world["shapes"]["body"][slot])
                g, point = term(f, centre, F(d), (F(bx), F(by)), bodies[body])
                if int(f["flags"]) & wire.FIELD_AS_IMPULSE:
                    e = wire.edit_apply_linear_impulse(body, g, point)
                else:
                    e = wire.edit_apply_force_to_center(body, g)
                assert world_edit_ref.apply(bodies, no_joints, [e]) == 0
                edits.append(e)
                states[i]["terms"] += 1
                if states[i]["lowestShape"] < 0:
                    states[i]["lowestShape"] = slot
    return bodies, states, wire.edit_list(edits)


def apply_in_place(world, fields):
    """The statement on a chain's world: its bodies replaced; -> the states"""
    bodies, states, _ = apply(world, fields)
    world["bodies"] = bodies
    return states


def in_reach(world, f):
    """The shape slots of one field's terms, ascending (needs the compiled reference)"""
    if not is_active(world, f):
        return []
    return [slot for slot in candidates(world, f) if distance(world, f, slot)[0] <= F(f["range"])]


def terms_per_body(world, edits):
    out = np.zeros(len(world["bodies"]), dtype=np.int64)
    np.add.at(out, edits["target"], 1)
    return out


# ---- fixtures: a committed world's name, a field list and the reference's recorded distance outputs for its candidates ----
FIXTURES = {"shapes_zoo40_PGS_NGS_Block": "zoo", "tumbler60_TGS_Soft": "drum", "mixed24_PGS": "mixed"}


def fixture_fields(name):
    """The field list of a fixture, made again from constants (every kind, both forms, falloff, an attached and a disabled field)"""
    if name == "shapes_zoo40_PGS_NGS_Block":
        return zoo_fields()
    if name == "tumbler60_TGS_Soft":
        return wire.field_list([wire.field_radial((0.0, 4.0), 6.0, -3.0), wire.field_drag((0.0, 4.0), 6.0, 0.25, flags=wire.FIELD_AS_IMPULSE),
                                wire.field_uniform((0.0, 4.0), 6.0, 1.5, (0.6, 0.8), flags=wire.FIELD_LINEAR_FALLOFF)])
    assert name == "mixed24_PGS"
    return wire.field_list([wire.field_radial((0.0, 2.0), 5.0, 2.0, flags=wire.FIELD_AS_IMPULSE | wire.FIELD_LINEAR_FALLOFF),
                            wire.field_drag((1.0, 3.0), 4.0, 0.5), wire.field_uniform((0.0, 0.0), 3.0, 1.0, (0.0, 1.0), flags=wire.FIELD_DISABLED)])


def zoo_fields():
    """shapes_zoo40: every kind in both forms, over three overlapping regions (a point, a point, a box with a rounding radius)"""
    box = ((-1.0, -0.5), (1.0, -0.5), (1.0, 0.5), (-1.0, 0.5))
    spots = (((-4.0, 1.0), 2.5), ((5.0, 3.0), 4.0), ((0.0, 2.0), 3.0))
    out = []
    for k, kind in enumerate((wire.FIELD_RADIAL, wire.FIELD_UNIFORM, wire.FIELD_DRAG)):
        for form in (0, wire.FIELD_AS_IMPULSE):
            position, reach = spots[(k + (1 if form else 0)) % 3]
            falloff = wire.FIELD_LINEAR_FALLOFF if (k + (1 if form else 0)) % 2 == 0 else 0
            out.append(wire.field(kind, position, reach, (-1.5, 2.0, 0.75)[k] * (0.25 if form else 4.0), flags=form | falloff, direction=(0.8, -0.6),
                                  vertices=box if kind == wire.FIELD_UNIFORM else ((0.0, 0.0),), radius=0.25 if kind == wire.FIELD_UNIFORM else 0.0))
    return wire.field_list(out)


def fixture_path(name):
    return os.path.join(GOLDEN, "%s.npz" % FIXTURES[name])


def load_fixture(name):
    """-> (fields, recorded) of a committed fixture"""
    with np.load(fixture_path(name)) as d:
        recorded = {(int(i), int(s)): (F(x), F(bx), F(by)) for i, s, x, (bx, by) in zip(d["field"], d["slot"], d["distance"], d["pointB"])}
        return d["fields"].copy(), recorded


def record(name, world):
    fields, into = fixture_fields(name), {}
    apply(world, fields, record_into=into)
    keys = sorted(into)
    return {"fields": fields, "field": np.array([k[0] for k in keys], dtype=np.int32), "slot": np.array([k[1] for k in keys], dtype=np.int32),
            "distance": np.array([into[k][0] for k in keys], dtype=np.float32), "pointB": np.array([into[k][1:] for k in keys], dtype=np.float32).reshape(-1, 2)}


def assert_zoo_condition(world, states, edits):
    """What keeps the shapes_zoo40 cases from passing vacuously: every field has at least 12 terms and at least 3 bodies with two terms,
    and at least 5 bodies are reached by two or more fields"""
    at, reach = 0, {}
    for i, n in enumerate(states["terms"]):
        targets, counts = np.unique(edits["target"][at:at + n], return_counts=True)
        at += n
        assert n >= 12 and (counts >= 2).sum() >= 3, (i, n, counts)
        for b in targets:
            reach.setdefault(int(b), set()).add(i)
    assert sum(len(v) >= 2 for v in reach.values()) >= 5
    static_six = [b for b in np.flatnonzero(world["bodies"]["type"] == wire.BODY_STATIC) if (world["shapes"]["body"] == b).sum() >= 6]
    assert static_six and not np.isin(edits["target"], static_six).any()


if __name__ == "__main__":
    from tests.world_chain import golden
    os.makedirs(GOLDEN, exist_ok=True)
    for world_name in FIXTURES:
        data = record(world_name, golden(world_name)[1])
        np.savez_compressed(fixture_path(world_name), **data)
        print(world_name, len(data["fields"]), "fields,", len(data["slot"]), "recorded distances,", os.path.getsize(fixture_path(world_name)), "bytes")
