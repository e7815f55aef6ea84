"""The statement of the shape casts (include/solver2d_amd.h: s2amd_world_cast_shape, s2amd_world_cast_shape_all), restated for the
tests.  Test infrastructure only.

The swept box, the candidate rule, the advancement loop, the selection and the CSR assembly are numpy float32 in the reference's
operation order; every distance is the reference's OWN s2ShapeDistance (src/distance.c:485-636), called through tests/proximity_ref.py
from oracle/_ref/libs2ref.so.  A world is a dict with "shapes", "bodies" and "origins" (the keys of tests/world_chain.py)."""
import numpy as np

from solver2d_amd import wire
from tests import proximity_ref as pref
from tests.scene_query_ref import _candidates, _csr

f32 = np.float32
LINEAR_SLOP = f32(0.005)                      # constants.h:7
SPECULATIVE = f32(f32(4.0) * LINEAR_SLOP)     # constants.h:8
TARGET = LINEAR_SLOP
TOLERANCE = f32(f32(0.25) * LINEAR_SLOP)
THRESHOLD = f32(TARGET + TOLERANCE)
CAP = 20
FLT_EPSILON = f32(1.19209290e-07)


def available():
    return pref.available()


def valid_cast(c):
    n = int(c["count"])
    if not 1 <= n <= 8:
        return False
    vals = [c["radius"], c["maxFraction"]] + list(c["position"]) + list(c["rot"]) + list(c["translation"]) + list(c["vertices"][:n].ravel())
    return bool(np.isfinite(vals).all()) and c["radius"] >= 0 and c["maxFraction"] >= 0


def normalize(x, y):
    """s2Normalize, src/math.c:41-52"""
    x, y = f32(x), f32(y)
    length = f32(np.sqrt(f32(f32(x * x) + f32(y * y))))
    if length < f32(f32(0.001) * FLT_EPSILON):
        return f32(0.0), f32(0.0)
    inv = f32(f32(1.0) / length)
    return f32(inv * x), f32(inv * y)


def mul_add(a, s, b):
    """s2MulAdd, math.h:121-124"""
    return f32(f32(a[0]) + f32(f32(s) * f32(b[0]))), f32(f32(a[1]) + f32(f32(s) * f32(b[1])))


def _bounds(c, p):
    """The bounds of s2TransformPoint({p, rot}, vertices[i]), folded from vertex 0 in index order with s2Min / s2Max"""
    s, co = f32(c["rot"][0]), f32(c["rot"][1])
    px, py = f32(p[0]), f32(p[1])
    lx = ly = ux = uy = None
    for i in range(int(c["count"])):
        vx, vy = f32(c["vertices"][i][0]), f32(c["vertices"][i][1])
        x = f32(f32(f32(co * vx) - f32(s * vy)) + px)  # math.h:350-356
        y = f32(f32(f32(s * vx) + f32(co * vy)) + py)
        if i == 0:
            lx, ly, ux, uy = x, y, x, y
            continue
        lx, ly = (lx if lx < x else x), (ly if ly < y else y)
        ux, uy = (ux if ux > x else x), (uy if uy > y else y)
    return lx, ly, ux, uy


def swept_box(c):
    with np.errstate(over="ignore", invalid="ignore"):
        a = _bounds(c, c["position"])
        b = _bounds(c, mul_add(c["position"], c["maxFraction"], c["translation"]))
        lx, ly = (a[0] if a[0] < b[0] else b[0]), (a[1] if a[1] < b[1] else b[1])
        ux, uy = (a[2] if a[2] > b[2] else b[2]), (a[3] if a[3] > b[3] else b[3])
        r = f32(f32(c["radius"]) + SPECULATIVE)
        return f32(lx - r), f32(ly - r), f32(ux + r), f32(uy + r)


def distance_at(c, proxy_a, t, proxy_b, xf_b):
    """D: s2ShapeDistance with transformA = {s2MulAdd(position, t, translation), rot}"""
    return pref.shape_distance(proxy_a, pref.transform(mul_add(c["position"], t, c["translation"]), c["rot"]), proxy_b, xf_b)


def cast_against(c, proxy_a, proxy_b, xf_b):
    """C(q, s) -> None (a miss) or (t_k, D_k, k)"""
    t = f32(0.0)
    tx, ty = f32(c["translation"][0]), f32(c["translation"][1])
    k = 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while True:
            d = distance_at(c, proxy_a, t, proxy_b, xf_b)
            dist = f32(d.distance)
            if dist < THRESHOLD or k == CAP:
                return t, d, k
            nx, ny = normalize(f32(f32(d.pointB.x) - f32(d.pointA.x)), f32(f32(d.pointB.y) - f32(d.pointA.y)))
            approach = f32(f32(tx * nx) + f32(ty * ny))
            if approach <= 0:
                return None
            nxt = f32(t + f32(f32(dist - TARGET) / approach))
            if not nxt <= f32(c["maxFraction"]):
                return None
            t, k = nxt, k + 1


def candidates(world, c):
    return _candidates(world["shapes"], swept_box(c), c["maskBits"])


def _record(slot, body, t, d, k):
    h = np.zeros(1, dtype=wire.shape_cast_hit_dtype)[0]
    h["shape"], h["body"], h["fraction"], h["distance"], h["iterations"] = slot, body, t, d.distance, k
    h["point"] = (d.pointB.x, d.pointB.y)
    h["normal"] = normalize(f32(f32(d.pointA.x) - f32(d.pointB.x)), f32(f32(d.pointA.y) - f32(d.pointB.y)))
    return h


def hits_of(world, c):
    """The hit records of one cast, ascending by slot"""
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    assert valid_cast(c)
    proxy_a = pref.make_proxy(c["vertices"], int(c["count"]), c["radius"])
    out = []
    for slot in candidates(world, c):
        sh = shapes[slot]
        body = int(sh["body"])
        r = cast_against(c, proxy_a, pref.shape_proxy(sh), pref.transform(origins[body], bodies["rot"][body]))
        if r is not None:
            out.append(_record(int(slot), body, *r))
    return out


def _flat(lists):
    offsets, _ = _csr([[h["shape"] for h in x] for x in lists])
    flat = [h for x in lists for h in x]
    return offsets, (np.array(flat, dtype=wire.shape_cast_hit_dtype) if flat else np.zeros(0, dtype=wire.shape_cast_hit_dtype))


def cast_shape_all(world, casts):
    """-> (offsets, hits) of wire.shape_cast_dtype casts"""
    return _flat([hits_of(world, c) for c in casts])


def both(world, casts):
    """-> (first hits, offsets, all hits): what the two calls answer, every cast run once"""
    lists = [hits_of(world, c) for c in casts]
    first = np.zeros(len(casts), dtype=wire.shape_cast_hit_dtype)
    for i, c in enumerate(casts):
        first[i] = first_of(c, lists[i])
    return (first,) + _flat(lists)


def first_of(c, hits):
    """The hit of least fraction, ties to the lowest slot (hits ascend by slot); none: shape = body = -1, fraction = maxFraction"""
    best = None
    for h in hits:
        if best is None or f32(h["fraction"]) < f32(best["fraction"]):
            best = h
    if best is None:
        best = np.zeros(1, dtype=wire.shape_cast_hit_dtype)[0]
        best["shape"], best["body"], best["fraction"] = -1, -1, c["maxFraction"]
    return best


def cast_shape(world, casts):
    """-> wire.shape_cast_hit_dtype[len(casts)]"""
    out = np.zeros(len(casts), dtype=wire.shape_cast_hit_dtype)
    for i, c in enumerate(casts):
        out[i] = first_of(c, hits_of(world, c))
    return out
