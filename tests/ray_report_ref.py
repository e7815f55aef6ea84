"""The statement of the ray report (include/solver2d_amd.h: s2amd_world_set_ray_sensors, s2amd_world_set_ray_report and the four
getters), restated for the tests.  Test infrastructure only.

Active, the world ray (an fp32 restatement of s2TransformPoint, include/solver2d/math.h:350-356), the segment box, the candidate rule
with its two exclusions, the selection and the events are numpy float32 in the reference's operation order; the per-shape casts are the
reference's OWN s2RayCastCircle / Capsule / Segment / Polygon through tests/scene_query_ref.py, so `hits` needs
oracle/_ref/libs2ref.so -- world_rays() and everything that starts from given hit shapes do not.  A world is a dict with "shapes",
"bodies" and "origins" (the keys of tests/world_chain.py); rays are wire.ray_sensor_dtype records.

states, ranges and events take exclusions=False: the same statement without the own-body and the static exclusion, which for a fixed
ray without flags is s2amd_world_ray_cast's."""
import ctypes

import numpy as np

from solver2d_amd import wire
from tests import scene_query_ref as sq

f32 = np.float32
available = sq.available


def transform_point(origin, rot, p):
    """s2TransformPoint({origin, rot}, p), rot = {s, c}: x = (c * p.x - s * p.y) + o.x, y = (s * p.x + c * p.y) + o.y"""
    s, c, px, py = f32(rot[0]), f32(rot[1]), f32(p[0]), f32(p[1])
    with np.errstate(invalid="ignore", over="ignore"):
        x = f32(f32(f32(c * px) - f32(s * py)) + f32(origin[0]))
        y = f32(f32(f32(s * px) + f32(c * py)) + f32(origin[1]))
    return x, y


def world_ray(world, q):
    """(active, P1, P2): the world ends of ray q; inactive rays have +0 ends"""
    zero = (f32(0.0), f32(0.0))
    body = int(q["body"])
    if int(q["flags"]) & wire.RAY_SENSOR_DISABLED:
        return False, zero, zero
    p1, p2 = (f32(q["p1"][0]), f32(q["p1"][1])), (f32(q["p2"][0]), f32(q["p2"][1]))
    if body >= 0:
        if body >= len(world["bodies"]) or int(world["bodies"]["type"][body]) == wire.BODY_FREE:
            return False, zero, zero
        origin, rot = world["origins"][body], world["bodies"]["rot"][body]
        p1, p2 = transform_point(origin, rot, p1), transform_point(origin, rot, p2)
    if not np.isfinite([p1[0], p1[1], p2[0], p2[1]]).all():  # s2IsValidRay on the world ray (maxFraction is the setter's)
        return False, zero, zero
    return True, p1, p2


def world_rays(world, rays):
    """The active rays as wire.ray_dtype records for s2amd_world_ray_cast, and their indices"""
    out, index = [], []
    for i, q in enumerate(rays):
        active, p1, p2 = world_ray(world, q)
        if active:
            out.append((p1, p2, q["maxFraction"], q["maskBits"]))
            index.append(i)
    return np.array(out, dtype=wire.ray_dtype) if out else np.zeros(0, dtype=wire.ray_dtype), index


def cast(world, q, exclusions=True):
    """One ray -> (active, P1, P2, best) with best = None or (slot, fraction, world normal, body, point)"""
    L = sq.lib()
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    active, p1, p2 = world_ray(world, q)
    if not active:
        return active, p1, p2, None
    max_fraction = f32(q["maxFraction"])
    with np.errstate(invalid="ignore", over="ignore"):
        d = (f32(p2[0] - p1[0]), f32(p2[1] - p1[1]))
        t = sq._mul_add(p1, max_fraction, d)  # src/dynamic_tree.c:1231-1238
    box = (p1[0] if p1[0] < t[0] else t[0], p1[1] if p1[1] < t[1] else t[1], p1[0] if p1[0] > t[0] else t[0], p1[1] if p1[1] > t[1] else t[1])
    own, skip_static = int(q["body"]), bool(int(q["flags"]) & wire.RAY_SENSOR_SKIP_STATIC)
    best = None
    for slot in sq._candidates(shapes, box, q["maskBits"]):
        sh = shapes[slot]
        body = int(sh["body"])
        if exclusions and ((own >= 0 and body == own) or (skip_static and int(bodies["type"][body]) == wire.BODY_STATIC)):
            continue
        l1 = sq._inv_transform(origins[body], bodies["rot"][body], p1)
        l2 = sq._inv_transform(origins[body], bodies["rot"][body], p2)
        inp = sq.RayCastInput(sq._vec(l1), sq._vec(l2), float(max_fraction))
        out = getattr(L, sq._RAY[int(sh["type"])])(ctypes.byref(inp), ctypes.byref(sq._geometry(sh)))
        if out.hit and (best is None or f32(out.fraction) < best[1]):  # float compare: -0 == +0, ties stay with the lower slot
            best = (int(slot), f32(out.fraction), (f32(out.normal.x), f32(out.normal.y)), body)
    if best is not None:
        slot, fraction, normal, body = best
        best = (slot, fraction, sq._rotate(bodies["rot"][body], normal), body, sq._mul_add(p1, fraction, d))
    return active, p1, p2, best


def hits(world, rays, exclusions=True):
    """The hit shape per ray (-1: a miss, or inactive)"""
    return [(-1 if best is None else best[0]) for _, _, _, best in (cast(world, q, exclusions) for q in rays)]


def states(world, rays, before, exclusions=True):
    """wire.ray_state_dtype[len(rays)]; `before` is the hit shape per ray of the evaluation before"""
    out = np.zeros(len(rays), dtype=wire.ray_state_dtype)
    for i, q in enumerate(rays):
        active, p1, p2, best = cast(world, q, exclusions)
        st = out[i]
        st["ray"], st["body"], st["active"], st["shapeBefore"] = i, q["body"], int(active), before[i]
        st["p1"], st["p2"] = p1, p2
        st["shape"], st["hitBody"], st["fraction"] = -1, -1, q["maxFraction"]
        if best is not None:
            st["shape"], st["fraction"], st["normal"], st["hitBody"], st["point"] = best
    return out


def ranges(world, rays, exclusions=True):
    return np.ascontiguousarray(states(world, rays, [-1] * len(rays), exclusions)["fraction"])


def events_of(before, now_states):
    """The events between the hit shapes `before` and the states of now, ascending by ray"""
    rows = [(i, before[i], int(st["shape"]), int(st["hitBody"])) for i, st in enumerate(now_states) if int(st["shape"]) != before[i]]
    return np.array(rows, dtype=wire.ray_event_dtype) if rows else np.zeros(0, dtype=wire.ray_event_dtype)


def events(world, rays, before, exclusions=True):
    return events_of(before, states(world, rays, before, exclusions))
