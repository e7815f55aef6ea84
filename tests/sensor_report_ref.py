"""The statement of the sensor report (include/solver2d_amd.h: s2amd_world_set_sensors, s2amd_world_set_sensor_report and the three
getters), restated for the tests.  Test infrastructure only.

Active, the world transform (an fp32 restatement of s2MulTransforms, include/solver2d/math.h:368-374 with s2MulRot :291-300), the
candidate box, the candidate rule, the set differences and the CSR assembly are numpy float32 in the reference's operation order; the
distance is the reference's OWN s2ShapeDistance through tests/proximity_ref.py (shape_proxy, query_box, shape_distance), so inside_lists
needs oracle/_ref/libs2ref.so -- poses() and everything that starts from given lists do not.  A world is a dict with "shapes", "bodies"
and "origins" (the keys of tests/world_chain.py); sensors are wire.sensor_dtype records."""
import numpy as np

from solver2d_amd import wire
from tests import proximity_ref
from tests.scene_query_ref import _candidates, _csr

f32 = np.float32
available = proximity_ref.available


def mul_transforms(a_p, a_q, b_p, b_q):
    """s2MulTransforms(A, B) -> (p, q), q = {s, c}: C.q = s2MulRot(A.q, B.q), C.p = s2Add(s2RotateVector(A.q, B.p), A.p)"""
    a_s, a_c, b_s, b_c = f32(a_q[0]), f32(a_q[1]), f32(b_q[0]), f32(b_q[1])
    s = f32(f32(a_s * b_c) + f32(a_c * b_s))
    c = f32(f32(a_c * b_c) - f32(a_s * b_s))
    bx, by = f32(b_p[0]), f32(b_p[1])
    x = f32(f32(f32(a_c * bx) - f32(a_s * by)) + f32(a_p[0]))
    y = f32(f32(f32(a_s * bx) + f32(a_c * by)) + f32(a_p[1]))
    return (x, y), (s, c)


def is_active(world, q):
    body = int(q["body"])
    if int(q["flags"]) & wire.SENSOR_DISABLED:
        return False
    return body < 0 or (body < len(world["bodies"]) and int(world["bodies"]["type"][body]) != wire.BODY_FREE)


def as_query(world, q):
    """The active sensor as the proximity query it evaluates: its proxy under the world transform, maxDistance = margin"""
    out = np.zeros(1, dtype=wire.proximity_query_dtype)[0]
    out["vertices"], out["count"], out["radius"] = q["vertices"], q["count"], q["radius"]
    out["maxDistance"], out["maskBits"] = q["margin"], q["maskBits"]
    body = int(q["body"])
    if body < 0:
        out["position"], out["rot"] = q["position"], q["rot"]
    else:
        out["position"], out["rot"] = mul_transforms(world["origins"][body], world["bodies"]["rot"][body], q["position"], q["rot"])
    return out


def poses(world, sensors):
    """wire.sensor_state_dtype with sensor, body, active, the transform and the box; the counts zero and lowestShape -1"""
    out = np.zeros(len(sensors), dtype=wire.sensor_state_dtype)
    out["lowestShape"] = -1
    for i, q in enumerate(sensors):
        out[i]["sensor"], out[i]["body"] = i, q["body"]
        if is_active(world, q):
            pq = as_query(world, q)
            out[i]["active"], out[i]["position"], out[i]["rot"] = 1, pq["position"], pq["rot"]
            out[i]["box"] = proximity_ref.query_box(pq)
    return out


def inside(world, q):
    """The slots inside one sensor, ascending"""
    if not is_active(world, q):
        return []
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    pq = as_query(world, q)
    proxy_a = proximity_ref.make_proxy(pq["vertices"], int(pq["count"]), pq["radius"])
    xf_a = proximity_ref.transform(pq["position"], pq["rot"])
    skip_static = bool(int(q["flags"]) & wire.SENSOR_SKIP_STATIC)
    out = []
    for slot in _candidates(shapes, proximity_ref.query_box(pq), q["maskBits"]):
        sh = shapes[slot]
        body = int(sh["body"])
        if body == int(q["body"]) or (skip_static and int(bodies["type"][body]) == wire.BODY_STATIC):
            continue
        d = proximity_ref.shape_distance(proxy_a, xf_a, proximity_ref.shape_proxy(sh), proximity_ref.transform(origins[body], bodies["rot"][body]))
        if f32(d.distance) <= f32(q["margin"]):
            out.append(int(slot))
    return out


def inside_lists(world, sensors):
    return [inside(world, q) for q in sensors]


def csr(lists):
    return _csr(lists)


def from_csr(offsets, flat):
    return [[int(x) for x in flat[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]


def events(before, now, world, sensors):
    """(entered, left) as wire.sensor_event_dtype, ascending by (sensor, shape)"""
    def records(pairs):
        out = np.zeros(len(pairs), dtype=wire.sensor_event_dtype)
        for k, (i, slot) in enumerate(pairs):
            out[k] = (i, slot, world["shapes"]["body"][slot], sensors[i]["body"])
        return out
    entered = [(i, s) for i in range(len(sensors)) for s in now[i] if s not in set(before[i])]
    left = [(i, s) for i in range(len(sensors)) for s in before[i] if s not in set(now[i])]
    return records(entered), records(left)


def states(world, sensors, before, now):
    out = poses(world, sensors)
    for i in range(len(sensors)):
        b, n = set(before[i]), set(now[i])
        out[i]["inside"], out[i]["entered"], out[i]["left"] = len(n), len(n - b), len(b - n)
        out[i]["lowestShape"] = min(n) if n else -1
    return out
