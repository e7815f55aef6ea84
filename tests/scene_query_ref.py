"""The statement of the scene queries (include/solver2d_amd.h: s2amd_world_ray_cast, s2amd_world_point_probe, s2amd_world_query_boxes),
restated for the tests.  Test infrastructure only.

The candidate rules, the transforms and the selection are numpy float32 in the reference's operation order; the per-shape tests are the
reference's OWN functions -- s2RayCastCircle / Capsule / Segment / Polygon and s2PointInCircle / Capsule / Polygon of src/geometry.c --
called through ctypes from oracle/_ref/libs2ref.so, which exports them.  A world is a dict with "shapes", "bodies" and "origins" (the
keys of tests/world_chain.py)."""
import ctypes

import numpy as np

from solver2d_amd import wire
from tests import refbind

f32 = np.float32
ALL_BITS = 0xFFFFFFFF


class Vec2(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float)]


class RayCastInput(ctypes.Structure):  # include/solver2d/types.h:60-64
    _fields_ = [("p1", Vec2), ("p2", Vec2), ("maxFraction", ctypes.c_float)]


class RayCastOutput(ctypes.Structure):  # include/solver2d/types.h:66-73
    _fields_ = [("normal", Vec2), ("point", Vec2), ("fraction", ctypes.c_float), ("iterations", ctypes.c_int32), ("hit", ctypes.c_bool)]


class Circle(ctypes.Structure):  # include/solver2d/geometry.h:27-56
    _fields_ = [("point", Vec2), ("radius", ctypes.c_float)]


class Capsule(ctypes.Structure):
    _fields_ = [("point1", Vec2), ("point2", Vec2), ("radius", ctypes.c_float)]


class Polygon(ctypes.Structure):
    _fields_ = [("vertices", Vec2 * 8), ("normals", Vec2 * 8), ("radius", ctypes.c_float), ("count", ctypes.c_int32)]


class Segment(ctypes.Structure):
    _fields_ = [("point1", Vec2), ("point2", Vec2)]


class Box(ctypes.Structure):  # include/solver2d/types.h: s2Box
    _fields_ = [("lowerBound", Vec2), ("upperBound", Vec2)]


class ShapeId(ctypes.Structure):  # include/solver2d/id.h:27-32
    _fields_ = [("index", ctypes.c_int32), ("world", ctypes.c_int16), ("revision", ctypes.c_uint16)]


QUERY_FN = ctypes.CFUNCTYPE(ctypes.c_bool, ShapeId, ctypes.c_void_p)

_lib = None


def available():
    return refbind.available()


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(refbind.REF_SO)
        for name, shape in (("Circle", Circle), ("Capsule", Capsule), ("Segment", Segment), ("Polygon", Polygon)):
            fn = getattr(L, "s2RayCast" + name)
            fn.restype, fn.argtypes = RayCastOutput, [ctypes.POINTER(RayCastInput), ctypes.POINTER(shape)]
            if name != "Segment":
                fn = getattr(L, "s2PointIn" + name)
                fn.restype, fn.argtypes = ctypes.c_bool, [Vec2, ctypes.POINTER(shape)]
        L.s2World_QueryAABB.restype, L.s2World_QueryAABB.argtypes = None, [refbind.WorldId, Box, QUERY_FN, ctypes.c_void_p]
        L.s2Shape_TestPoint.restype, L.s2Shape_TestPoint.argtypes = ctypes.c_bool, [ShapeId, Vec2]
        _lib = L
    return _lib


# ---- the reference's own world query and pick (src/world.c:605-615, src/shape.c:110-137) ----
def ref_query_aabb(world_id, box):
    """The shape ids s2World_QueryAABB calls back for, in callback order"""
    ids = []

    def collect(shape_id, _context):
        ids.append(ShapeId(shape_id.index, shape_id.world, shape_id.revision))
        return True

    b = Box(Vec2(float(box[0]), float(box[1])), Vec2(float(box[2]), float(box[3])))
    lib().s2World_QueryAABB(world_id, b, QUERY_FN(collect), None)
    return ids


def ref_pick(world_id, p):
    """Picking as the reference's samples do it: s2World_QueryAABB with the box {p, p}, then s2Shape_TestPoint -> sorted shape slots"""
    point = Vec2(float(p[0]), float(p[1]))
    return sorted(i.index for i in ref_query_aabb(world_id, (p[0], p[1], p[0], p[1])) if lib().s2Shape_TestPoint(i, point))


# ---- geometry of a wire shape as the reference's structs ----
def _vec(v):
    return Vec2(float(v[0]), float(v[1]))


def _geometry(sh):
    t = int(sh["type"])
    v = sh["vertices"]
    if t == wire.SHAPE_CIRCLE:
        return Circle(_vec(v[0]), float(sh["radius"]))
    if t == wire.SHAPE_CAPSULE:
        return Capsule(_vec(v[0]), _vec(v[1]), float(sh["radius"]))
    if t == wire.SHAPE_SEGMENT:
        return Segment(_vec(v[0]), _vec(v[1]))
    poly = Polygon()
    for i in range(8):
        poly.vertices[i], poly.normals[i] = _vec(v[i]), _vec(sh["normals"][i])
    poly.radius, poly.count = float(sh["radius"]), min(max(int(sh["count"]), 0), 8)
    return poly


_RAY = {wire.SHAPE_CIRCLE: "s2RayCastCircle", wire.SHAPE_CAPSULE: "s2RayCastCapsule", wire.SHAPE_SEGMENT: "s2RayCastSegment",
        wire.SHAPE_POLYGON: "s2RayCastPolygon"}
_POINT = {wire.SHAPE_CIRCLE: "s2PointInCircle", wire.SHAPE_CAPSULE: "s2PointInCapsule", wire.SHAPE_POLYGON: "s2PointInPolygon"}


# ---- float32 in the reference's operation order ----
def _inv_transform(origin, rot, p):  # s2InvTransformPoint, include/solver2d/math.h:359-364; rot = {s, c}
    vx, vy = f32(p[0]) - f32(origin[0]), f32(p[1]) - f32(origin[1])
    s, c = f32(rot[0]), f32(rot[1])
    return f32(c * vx + s * vy), f32(-s * vx + c * vy)


def _rotate(rot, v):  # s2RotateVector, math.h:330-341
    s, c = f32(rot[0]), f32(rot[1])
    return f32(c * f32(v[0]) - s * f32(v[1])), f32(s * f32(v[0]) + c * f32(v[1]))


def _mul_add(a, s, b):  # s2MulAdd, math.h:121
    return f32(f32(a[0]) + f32(s) * f32(b[0])), f32(f32(a[1]) + f32(s) * f32(b[1]))


def _candidates(shapes, box, mask):
    """live, (categoryBits & maskBits) != 0, s2AABB_Overlaps(fatAABB, box) (include/solver2d/aabb.h:111-123) -> ascending slots"""
    fat = shapes["fatAABB"]
    lx, ly, ux, uy = (f32(x) for x in box)
    with np.errstate(invalid="ignore", over="ignore"):
        d1x, d1y = lx - fat[:, 2], ly - fat[:, 3]
        d2x, d2y = fat[:, 0] - ux, fat[:, 1] - uy
        apart = (d1x > 0) | (d1y > 0) | (d2x > 0) | (d2y > 0)
    ok = (shapes["type"] != wire.SHAPE_FREE) & ((shapes["categoryBits"] & np.uint32(mask)) != 0) & ~apart
    return np.nonzero(ok)[0]


def _csr(lists):
    offsets = np.zeros(len(lists) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    flat = np.array([s for x in lists for s in x], dtype=np.int32)
    return offsets, flat


def query_boxes(world, boxes):
    """-> (offsets, shapes) of wire.box_query_dtype queries"""
    return _csr([_candidates(world["shapes"], q["box"], q["maskBits"]).tolist() for q in boxes])


def point_probe(world, probes):
    """-> (offsets, shapes) of wire.point_probe_dtype queries"""
    L = lib()
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    out = []
    for q in probes:
        p = q["p"]
        hits = []
        for slot in _candidates(shapes, (p[0], p[1], p[0], p[1]), q["maskBits"]):
            sh = shapes[slot]
            name = _POINT.get(int(sh["type"]))
            if name is None:
                continue  # segments never hit
            body = int(sh["body"])
            local = _inv_transform(origins[body], bodies["rot"][body], p)
            if getattr(L, name)(_vec(local), ctypes.byref(_geometry(sh))):
                hits.append(int(slot))
        out.append(hits)
    return _csr(out)


def valid_ray(ray):  # s2IsValidRay, src/geometry.c:15-20
    vals = [ray["p1"][0], ray["p1"][1], ray["p2"][0], ray["p2"][1], ray["maxFraction"]]
    return bool(np.isfinite(vals).all()) and 0.0 <= ray["maxFraction"] < 100000.0


def ray_cast(world, rays):
    """-> wire.ray_hit_dtype[len(rays)]"""
    L = lib()
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    hits = np.zeros(len(rays), dtype=wire.ray_hit_dtype)
    for i, r in enumerate(rays):
        assert valid_ray(r), i
        p1, p2, max_fraction = r["p1"], r["p2"], f32(r["maxFraction"])
        d = (f32(p2[0]) - f32(p1[0]), f32(p2[1]) - f32(p1[1]))
        t = _mul_add(p1, max_fraction, d)  # src/dynamic_tree.c:1231-1238
        box = (p1[0] if p1[0] < t[0] else t[0], p1[1] if p1[1] < t[1] else t[1], p1[0] if p1[0] > t[0] else t[0], p1[1] if p1[1] > t[1] else t[1])
        best = None
        for slot in _candidates(shapes, box, r["maskBits"]):
            sh = shapes[slot]
            body = int(sh["body"])
            l1 = _inv_transform(origins[body], bodies["rot"][body], p1)
            l2 = _inv_transform(origins[body], bodies["rot"][body], p2)
            inp = RayCastInput(_vec(l1), _vec(l2), float(max_fraction))
            out = getattr(L, _RAY[int(sh["type"])])(ctypes.byref(inp), ctypes.byref(_geometry(sh)))
            if out.hit and (best is None or f32(out.fraction) < best[1]):  # float compare: -0 == +0, ties stay with the lower slot
                best = (int(slot), f32(out.fraction), (f32(out.normal.x), f32(out.normal.y)), body)
        h = hits[i]
        if best is None:
            h["shape"], h["body"], h["fraction"] = -1, -1, max_fraction
            continue
        slot, fraction, normal, body = best
        h["shape"], h["body"], h["fraction"] = slot, body, fraction
        h["point"] = _mul_add(p1, fraction, d)
        h["normal"] = _rotate(bodies["rot"][body], normal)
    return hits
