"""The statement of move-and-slide (include/solver2d_amd.h: s2amd_world_move_shapes), restated for the tests.  Test infrastructure only.

The loop, the graze test and the clip are numpy float32 in the reference's operation order; the swept box, the candidates and the
advancement C(q, s) are tests/shape_cast_ref.py's, whose every distance is the reference's OWN s2ShapeDistance (src/distance.c:485-636),
called through tests/proximity_ref.py from oracle/_ref/libs2ref.so.  A world is a dict with "shapes", "bodies" and "origins"."""
import numpy as np

from solver2d_amd import wire
from tests import proximity_ref as pref, shape_cast_ref as cref

f32 = np.float32
GRAZE = f32(1e-4)
ZERO = f32(0.0)


def available():
    return cref.available()


def valid_mover(m, body_capacity):
    """The library's list: the shape casts' checks of proxy, radius, position, rot and translation; maxIterations, flags, reserved,
    ignoreBody"""
    n = int(m["count"])
    if not 1 <= n <= 8:
        return False
    vals = [m["radius"]] + list(m["position"]) + list(m["rot"]) + list(m["translation"]) + list(m["vertices"][:n].ravel())
    if not (bool(np.isfinite(vals).all()) and m["radius"] >= 0):
        return False
    return (1 <= int(m["maxIterations"]) <= wire.MOVER_MAX_ITERATIONS and (int(m["flags"]) & ~wire.MOVER_STATIC_ONLY) == 0 and
            not np.any(m["reserved"]) and int(m["ignoreBody"]) < body_capacity)


def length(x, y):
    """s2Length, math.h:169-172"""
    x, y = f32(x), f32(y)
    return f32(np.sqrt(f32(f32(x * x) + f32(y * y))))


def dot(a, b):
    return f32(f32(f32(a[0]) * f32(b[0])) + f32(f32(a[1]) * f32(b[1])))


def grazes(r, n, graze=GRAZE):
    return dot(r, n) >= -f32(f32(graze) * length(r[0], r[1]))


def cast_of(m, p, r):
    """Step 1: the cast a mover makes from p with r left"""
    c = np.zeros(1, dtype=wire.shape_cast_dtype)[0]
    for key in ("vertices", "count", "radius", "rot", "maskBits"):
        c[key] = m[key]
    c["position"], c["translation"], c["maxFraction"] = p, r, 1.0
    return c


def move(world, m, graze=GRAZE, path=None):
    """One mover -> (result record, plane records[8]).  `path`, a list, takes one (p, r, t) per cast: the segment travelled (from p by
    t * r), for the tests that sample geometry along it."""
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    assert valid_mover(m, len(bodies))
    proxy_a = pref.make_proxy(m["vertices"], int(m["count"]), m["radius"])
    p = (f32(m["position"][0]), f32(m["position"][1]))
    r = (f32(m["translation"][0]), f32(m["translation"][1]))
    planes = np.zeros(wire.MOVER_MAX_ITERATIONS, dtype=wire.mover_plane_dtype)
    normals, slots = [], []
    advances, status, iterations = 0, wire.MOVER_OUT_OF_ITERATIONS, 0
    ignore, static_only = int(m["ignoreBody"]), bool(int(m["flags"]) & wire.MOVER_STATIC_ONLY)
    for b in range(int(m["maxIterations"])):
        iterations = b + 1
        c = cast_of(m, p, r)
        best = None
        for slot in cref.candidates(world, c):
            slot = int(slot)
            body = int(shapes["body"][slot])
            if slot in slots or (ignore >= 0 and body == ignore) or (static_only and bodies["type"][body] != wire.BODY_STATIC):
                continue
            hit = cref.cast_against(c, proxy_a, pref.shape_proxy(shapes[slot]), pref.transform(origins[body], bodies["rot"][body]))
            if hit is None:
                continue
            t, d, k = hit
            n = cref.normalize(f32(f32(d.pointA.x) - f32(d.pointB.x)), f32(f32(d.pointA.y) - f32(d.pointB.y)))
            if k == 0 and (n[0] != 0 or n[1] != 0) and grazes(r, n, graze):
                continue
            if best is None or f32(t) < f32(best[1]):
                best = (slot, t, d, k, n, body)
        if best is None:
            if path is not None:
                path.append((p, r, f32(1.0)))
            p, r, status = (f32(p[0] + r[0]), f32(p[1] + r[1])), (ZERO, ZERO), wire.MOVER_REACHED
            break
        slot, t, d, k, n, body = best
        if path is not None:
            path.append((p, r, f32(t)))
        p = cref.mul_add(p, t, r)
        left = f32(f32(1.0) - f32(t))
        rem = (f32(left * r[0]), f32(left * r[1]))
        advances += k
        pl = planes[len(slots)]
        pl["shape"], pl["body"], pl["fraction"], pl["distance"] = slot, body, t, d.distance
        pl["point"], pl["normal"] = (d.pointB.x, d.pointB.y), n
        slots.append(slot)
        if n[0] == 0 and n[1] == 0:
            r, status = rem, wire.MOVER_OVERLAPPED
            break
        into = dot(rem, n)
        if into < 0:
            rem = (f32(rem[0] - f32(into * n[0])), f32(rem[1] - f32(into * n[1])))
        r = rem
        if not all(grazes(rem, e, graze) for e in normals):
            status = wire.MOVER_CORNERED
            break
        normals.append(n)
        if rem[0] == 0 and rem[1] == 0:
            status = wire.MOVER_BLOCKED
            break
    out = np.zeros(1, dtype=wire.mover_result_dtype)[0]
    out["position"], out["remaining"] = p, r
    out["status"], out["planeCount"], out["iterations"], out["advances"] = status, len(slots), iterations, advances
    return out, planes


def move_shapes(world, movers, graze=GRAZE):
    """-> (wire.mover_result_dtype[len(movers)], wire.mover_plane_dtype[len(movers), 8])"""
    results = np.zeros(len(movers), dtype=wire.mover_result_dtype)
    planes = np.zeros((len(movers), wire.MOVER_MAX_ITERATIONS), dtype=wire.mover_plane_dtype)
    for i, m in enumerate(movers):
        results[i], planes[i] = move(world, m, graze)
    return results, planes
