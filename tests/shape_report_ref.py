"""The shape report of include/solver2d_amd.h (s2amd_world_set_shape_report, s2amd_world_set_shape_view and their getters) stated in
numpy on a wire world dict as tests/world_chain.py keeps it: what the device's compaction (solver2d_amd/csrc/shape_report.hip) must
return, byte for byte.  `view` is None or (lower.x, lower.y, upper.x, upper.y).  Test infrastructure only."""
import numpy as np

from solver2d_amd import wire

f32 = np.float32


def in_view(world, view):
    """Per shape slot: live, and no view set or s2AABB_Overlaps(view, aabb) (include/solver2d/aabb.h:111-123): false only when one of the
    four differences is > 0, so a NaN is in view."""
    shapes = world["shapes"]
    live = shapes["type"] != wire.SHAPE_FREE
    if view is None:
        return live
    v = np.asarray(view, dtype=f32)
    box = shapes["aabb"].astype(f32)
    with np.errstate(invalid="ignore"):
        d1x, d1y = box[:, 0] - v[2], box[:, 1] - v[3]
        d2x, d2y = v[0] - box[:, 2], v[1] - box[:, 3]
        assert d1x.dtype == f32 and d2y.dtype == f32
        apart = (d1x > 0) | (d1y > 0) | (d2x > 0) | (d2y > 0)
    return live & ~apart


def events(prev_mask, world, view):
    """(entered, left) slot lists, ascending, of a step that took the slots from `prev_mask` to the state of `world` under `view`."""
    now = in_view(world, view)
    prev = np.asarray(prev_mask, dtype=bool)
    return np.flatnonzero(now & ~prev).astype(np.int32), np.flatnonzero(prev & ~now).astype(np.int32)


def body_class(bodies):
    """src/world.c:389-405: a dynamic body with mass == 0 is class 3 before anything else; 0 static, 1 kinematic, 2 otherwise."""
    t, m = bodies["type"], bodies["mass"]
    out = np.full(len(bodies), 2, dtype=np.int32)
    out[t == wire.BODY_STATIC] = 0
    out[t == wire.BODY_KINEMATIC] = 1
    out[(t == wire.BODY_DYNAMIC) & (m == f32(0))] = 3
    return out


def vertex_count(shapes):
    t = shapes["type"]
    out = np.zeros(len(shapes), dtype=np.int32)
    out[t == wire.SHAPE_POLYGON] = np.clip(shapes["count"][t == wire.SHAPE_POLYGON], 0, 8)
    out[(t == wire.SHAPE_CAPSULE) | (t == wire.SHAPE_SEGMENT)] = 2
    out[t == wire.SHAPE_CIRCLE] = 1
    return out


def draws(world, view):
    """s2amdShapeDraw of every live shape in view, ascending: vertices[i] = s2TransformPoint({origin, rot} of the body, vertices[i]) in
    float32, one rounding per operation, in the order of include/solver2d/math.h:350-356; axis = s2RotateVector(rot, {1, 0})."""
    slots = np.flatnonzero(in_view(world, view))
    sh = world["shapes"][slots]
    out = np.zeros(len(slots), dtype=wire.shape_draw_dtype)
    out["shape"], out["body"], out["type"] = slots, sh["body"], sh["type"]
    vc = vertex_count(sh)
    out["vertexCount"] = vc
    out["bodyClass"] = body_class(world["bodies"])[sh["body"]]
    out["radius"] = sh["radius"]
    origins = np.asarray(world["origins"], dtype=f32)
    ox, oy = origins[sh["body"], 0], origins[sh["body"], 1]
    rot = world["bodies"]["rot"][sh["body"]]
    qs, qc = rot[:, 0].astype(f32), rot[:, 1].astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        out["axis"][:, 0] = qc * f32(1) - qs * f32(0)
        out["axis"][:, 1] = qs * f32(1) + qc * f32(0)
        for i in range(8):
            px, py = sh["vertices"][:, i, 0], sh["vertices"][:, i, 1]
            x = (qc * px - qs * py) + ox
            y = (qs * px + qc * py) + oy
            assert x.dtype == f32 and y.dtype == f32
            out["vertices"][:, i, 0] = np.where(i < vc, x, f32(0))
            out["vertices"][:, i, 1] = np.where(i < vc, y, f32(0))
    out["aabb"], out["fatAABB"] = sh["aabb"], sh["fatAABB"]
    return out


def bounds(boxes):
    """From {+INF, +INF, -INF, -INF} over the boxes in order: lower = x < cur ? x : cur, upper = x > cur ? x : cur (a NaN never wins)."""
    cur = [f32(np.inf), f32(np.inf), f32(-np.inf), f32(-np.inf)]
    for b in np.asarray(boxes, dtype=f32).reshape(-1, 4):
        for k in (0, 1):
            cur[k] = b[k] if b[k] < cur[k] else cur[k]
        for k in (2, 3):
            cur[k] = b[k] if b[k] > cur[k] else cur[k]
    return np.array(cur, dtype=f32)


def summary(world, view):
    """s2amdShapeSummary"""
    shapes, bodies = world["shapes"], world["bodies"]
    live = shapes["type"] != wire.SHAPE_FREE
    seen = in_view(world, view)
    body = np.where(live, shapes["body"], 0)
    out = np.zeros(1, dtype=wire.shape_summary_dtype)[0]
    out["liveShapes"], out["inView"] = int(live.sum()), int(seen.sum())
    out["byType"] = [int((live & (shapes["type"] == t)).sum()) for t in range(4)]
    if len(bodies):
        out["badBodyShapes"] = int((live & (body_class(bodies)[body] == 3)).sum())
        movable = live & (bodies["type"][body] != wire.BODY_STATIC) & (bodies["type"][body] != wire.BODY_FREE)
    else:
        movable = np.zeros(len(shapes), dtype=bool)
    out["movableBounds"] = bounds(shapes["aabb"][movable])
    out["viewBounds"] = bounds(shapes["aabb"][seen])
    return out
