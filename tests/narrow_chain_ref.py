"""The statement of one step of stage 3 (s2amd_update_contacts; src/world.c:132-168) for an array of pairs, restated for the
narrow-chain tests (tests/test_narrow_chain_host.py, tests/test_gpu_narrow_chain.py).  Test infrastructure only.

Per live pair: the fat-box test in float32 with the reference's `> 0` (aabb.h:111-123); then the reference's OWN s2Collide* of the
ordered type pair (src/manifold.c), called through ctypes from oracle/_ref/libs2ref.so with the pair's CARRIED s2DistanceCache, not an
empty one; then s2UpdateContact's id matching (src/contact.c:296-358) on the wire records.  What it writes is what the wire format
holds: the status, the pair state (cache metric, count and indices, ids, persisted) and the contact; points at and beyond pointCount
are all zero bits, and bodyA, bodyB, friction and constraintIndex are kept.  The reference has no metric test on a carried cache (it
only writes s2DistanceCache.metric, src/distance.c:215-226): a stale simplex is simply where GJK starts."""
import ctypes

import numpy as np

from solver2d_amd import wire
from tests.contact_query_ref import REGISTERS, TAKES_CACHE, geometry, lib
from tests.proximity_ref import DistanceCache, transform

f32 = np.float32
POINT_VECTORS = ("localAnchorA", "localAnchorB", "frictionAnchorA", "frictionAnchorB", "frictionNormalA", "frictionNormalB")
CARRIED = ("frictionNormalA", "frictionNormalB", "frictionAnchorA", "frictionAnchorB", "normalImpulse", "tangentImpulse")


def function_name(shapes, pair):
    """The manifold function of a pair record's ordered type pair"""
    return REGISTERS[(int(shapes["type"][pair["shapeA"]]), int(shapes["type"][pair["shapeB"]]))]


def fat_boxes_overlap(a, b):
    """s2AABB_Overlaps of two float32 boxes (lx, ly, ux, uy): apart only where a difference is > 0, so boxes that touch overlap"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    d1x, d1y = f32(b[0] - a[2]), f32(b[1] - a[3])
    d2x, d2y = f32(a[0] - b[2]), f32(a[1] - b[3])
    if d1x > 0 or d1y > 0:
        return False
    if d2x > 0 or d2y > 0:
        return False
    return True


def collide(shape_a, xf_a, shape_b, xf_b, cache):
    """The s2Collide* of the ordered pair -> s2Manifold; `cache` (a DistanceCache) is read and written where the function takes one"""
    name = REGISTERS[(int(shape_a["type"]), int(shape_b["type"]))]
    args = [ctypes.byref(geometry(shape_a)), xf_a, ctypes.byref(geometry(shape_b)), xf_b]
    if name in TAKES_CACHE:
        args.append(ctypes.byref(cache))
    return getattr(lib(), name)(*args)


def _cache_of(pair):
    c = DistanceCache()
    c.metric, c.count = float(pair["cacheMetric"]), int(pair["cacheCount"])
    for k in range(3):
        c.indexA[k], c.indexB[k] = int(pair["cacheIndexA"][k]), int(pair["cacheIndexB"][k])
    return c


def _point_of(mp):
    """A manifold point as the manifold function returned it, before the matching: no impulses"""
    q = np.zeros(1, dtype=wire.manifold_point_dtype)[0]
    for f in POINT_VECTORS:
        v = getattr(mp, f)
        q[f] = (v.x, v.y)
    q["separation"] = mp.separation
    return q


def match(pair, contact, points, ids, normal):
    """s2UpdateContact after the manifold function: `points` / `ids` are the new manifold's.  Each new point looks for its id among the
    old manifold's points, first to last, and takes the first match's friction frame and impulses; friction persists only where the
    count is unchanged and every point found its id."""
    old_count, old_ids, old_points = int(contact["pointCount"]), pair["id"].copy(), contact["points"].copy()
    friction_persisted = 1 if len(points) == old_count else 0
    contact["pointCount"], contact["normal"] = len(points), normal
    contact["points"] = np.zeros(2, dtype=wire.manifold_point_dtype)
    pair["id"], pair["persisted"] = 0, 0
    for i, (q, new_id) in enumerate(zip(points, ids)):
        persisted = 0
        for j in range(old_count):
            if int(old_ids[j]) == new_id:
                for f in CARRIED:
                    q[f] = old_points[j][f]
                persisted = 1
                break
        if not persisted:
            friction_persisted = 0
        contact["points"][i], pair["id"][i], pair["persisted"][i] = q, new_id, persisted
    contact["frictionPersisted"] = friction_persisted


def update_contacts(bodies, origins, shapes, pairs, contacts):
    """One step of stage 3 on wire arrays, in place -> status int32[len(pairs)] (wire.PAIR_*)"""
    status = np.zeros(len(pairs), dtype=np.int32)
    for i in range(len(pairs)):
        pair, contact = pairs[i], contacts[i]
        a, b = int(pair["shapeA"]), int(pair["shapeB"])
        if a < 0 or b < 0:
            status[i] = wire.PAIR_FREE
            continue
        sa, sb = shapes[a], shapes[b]
        if not fat_boxes_overlap(sa["fatAABB"], sb["fatAABB"]):
            status[i] = wire.PAIR_SEPARATED
            continue
        status[i] = wire.PAIR_UPDATED
        ba, bb = int(sa["body"]), int(sb["body"])
        cache = _cache_of(pair)
        m = collide(sa, transform(origins[ba], bodies["rot"][ba]), sb, transform(origins[bb], bodies["rot"][bb]), cache)
        count = int(m.pointCount)
        match(pair, contact, [_point_of(m.points[k]) for k in range(count)], [int(m.points[k].id) for k in range(count)],
              (m.normal.x, m.normal.y))
        pair["cacheMetric"], pair["cacheCount"] = cache.metric, cache.count
        for k in range(3):
            pair["cacheIndexA"][k], pair["cacheIndexB"][k] = cache.indexA[k], cache.indexB[k]
    return status
