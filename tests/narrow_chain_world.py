"""Inputs of the narrow-chain tests (tests/test_narrow_chain_host.py, tests/test_gpu_narrow_chain.py), what the two share, and the
generator of their fixtures tests/golden/narrow_chain/*.npz (python -m tests.narrow_chain_world, with oracle/_ref/libs2ref.so built).
Test infrastructure only.

`chains`: PAIRS pairs, PER_TYPE of each of the nine ordered type pairs, every pair with two bodies and two shapes of its own on a coarse
grid, driven through POSES poses with the pair state and the contact CARRIED from pose to pose, so that GJK starts from warm caches of
1, 2 and 3 vertices and the id matching sees manifolds that change.  `directed`: one pose of degenerate and edge cases, each stated
where it is made.  A fixture holds the shapes, per pose the origins, rotations and fat boxes, the stamped pre-state, and what the
statement (tests/narrow_chain_ref.py) answers: status, pairs_post, contacts_post.  Arrays are [pair, pose, ...]; `chains` is cut into
PARTS files by pair ranges to keep every file small."""
import os

import numpy as np

from solver2d_amd import wire
from tests import contact_query_ref as cq
from tests.contact_query_world import make_query, shape_vertices

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "narrow_chain")
CAPSULE, CIRCLE, POLYGON, SEGMENT = wire.SHAPE_CAPSULE, wire.SHAPE_CIRCLE, wire.SHAPE_POLYGON, wire.SHAPE_SEGMENT
TYPE_PAIRS = list(cq.REGISTERS)  # the nine ordered type pairs, in the register table's order
PER_TYPE, POSES, PARTS = 32, 12, 3
PAIRS = PER_TYPE * len(TYPE_PAIRS)
GRID, COLUMNS = 8.0, 18         # pair i lives around (GRID * (i % COLUMNS), GRID * (i // COLUMNS)); no shape is 2 m across
FRICTION, FIRST_CONSTRAINT = 0.6, 1000  # what a slot keeps: friction, and constraintIndex = FIRST_CONSTRAINT + pair
# the offset of body B along the pair's direction, pose after pose (each pair starts SHIFT poses into it, see chain_inputs)
SCHEDULE = ("deep", "mid", "shallow", "touch", "band", "beyond", "band", "clear", "shallow", "deep", "band", "touch")
# ... for the pairs placed by distance: the gap between the shapes (touch: 0; negative: that far short of touching)
GAP = {"mid": -0.05, "shallow": -0.004, "touch": 0.0, "band": 0.01, "beyond": 0.026, "clear": 3.0}
# ... for the axis-aligned pairs, in exact binary fractions, so that SAT and clipping meet exact ties
ALIGNED_GAP = {"deep": -0.125, "mid": -0.0625, "shallow": -1.0 / 256, "touch": 0.0, "band": 1.0 / 128, "beyond": 1.0 / 32, "clear": 4.0}
QUARTER_TURNS = ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))  # (sin, cos) of 0, 90, 180, 270 degrees, exactly
TURN_PER_POSE, SPIN_PER_POSE = 0.04, 0.11  # radians: the direction turns slowly; body B turns enough to stale the cached simplex
STAMPED = ("normalImpulse", "tangentImpulse", "frictionAnchorA", "frictionAnchorB", "frictionNormalA", "frictionNormalB")
SPECULATIVE = cq.SPECULATIVE


# ---- shapes, poses, fat boxes ----
def make_shape(shape_type, vertices, radius=0.0):
    """A wire shape without a body or boxes yet; a polygon gets s2MakePolygon's normals"""
    q = make_query(shape_type, vertices, radius, (0.0, 0.0), 0.0)
    sh = np.zeros(1, dtype=wire.shape_dtype)[0]
    sh["type"], sh["count"], sh["radius"] = shape_type, len(vertices), radius
    sh["vertices"], sh["normals"] = q["vertices"], q["normals"]
    sh["categoryBits"], sh["maskBits"] = 1, 0xFFFFFFFF
    return sh


def box(hx, hy, radius=0.0):
    return make_shape(POLYGON, [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)], radius)


def rot_of(angle):
    return (f32(np.sin(angle)), f32(np.cos(angle)))


def fat_box(sh, origin, rot):
    """contact_query_ref.query_box's rule: s2Shape_ComputeAABB at {origin, rot} grown by the speculative distance"""
    return cq.query_box({"rot": rot, "position": origin, "type": sh["type"], "vertices": sh["vertices"], "count": sh["count"],
                         "radius": sh["radius"]})


def fresh(n):
    """n new contacts: pair i between shapes and bodies 2i and 2i + 1, an empty cache and an empty manifold"""
    pairs, contacts = np.zeros(n, dtype=wire.pair_state_dtype), np.zeros(n, dtype=wire.contact_dtype)
    pairs["shapeA"] = contacts["bodyA"] = 2 * np.arange(n)
    pairs["shapeB"] = contacts["bodyB"] = 2 * np.arange(n) + 1
    contacts["friction"], contacts["constraintIndex"] = FRICTION, FIRST_CONSTRAINT + np.arange(n)
    return pairs, contacts


def stamp_value(pose, pair, point, k):
    """The value written into float k (0..9) of the stamped fields of a live point before `pose`: whole, non-zero, below 2^24, and
    different for every (pose, pair, point, k), so that a carried value tells where it came from"""
    return f32(((pose + 1) * 512 + pair) * 32 + point * 16 + k)


def stamp(contacts, pose):
    """Before every pose: distinct non-zero values in the impulses and the friction frame of every live point, as a solver would
    leave them behind"""
    for i in np.flatnonzero(contacts["pointCount"] > 0):
        for p in range(int(contacts["pointCount"][i])):
            q, k = contacts["points"][i][p], 0
            for f in STAMPED:
                width = 1 if q[f].ndim == 0 else 2
                q[f] = [stamp_value(pose, i, p, k + c) for c in range(width)] if width == 2 else stamp_value(pose, i, p, k)
                k += width
            contacts["points"][i][p] = q


def advance(pairs, contacts, status, pose):
    """From the result of pose - 1 to the pre-state of `pose`: a pair stage 3 reported SEPARATED becomes a fresh contact (the reference
    destroys the contact and creates a new one when the boxes meet again), then every live point is stamped"""
    gone = np.flatnonzero(status == wire.PAIR_SEPARATED)
    new_pairs, new_contacts = fresh(len(pairs))
    pairs[gone], contacts[gone] = new_pairs[gone], new_contacts[gone]
    stamp(contacts, pose)


def world_at(fx, pose):
    """(bodies, origins, shapes) of a pose: body and shape 2i and 2i + 1 are pair i's; stage 3 reads rot, origins and fatAABB"""
    n = len(fx["shapes"])
    bodies = np.zeros(n, dtype=wire.body_dtype)
    origins = np.ascontiguousarray(fx["origins"][:, pose].reshape(n, 2))
    bodies["rot"], bodies["position"], bodies["type"] = fx["rots"][:, pose].reshape(n, 2), origins, wire.BODY_DYNAMIC
    bodies["mass"] = bodies["invMass"] = bodies["I"] = bodies["invI"] = 1.0
    shapes = fx["shapes"].copy()
    shapes["fatAABB"] = fx["fat"][:, pose].reshape(n, 4)
    return bodies, origins, shapes


def type_pair_name(fx, pair):
    return cq.REGISTERS[(int(fx["shapes"]["type"][2 * pair]), int(fx["shapes"]["type"][2 * pair + 1]))]


def first_difference(fx, pose, status, pairs, contacts, pre_pairs, pre_contacts):
    """None where the result of one pose equals the fixture -- the status of every pair, every byte of the pair state and the contact
    of an UPDATED pair, the untouched bytes of a SEPARATED one -- else a message naming the pose, the first pair and its type pair"""
    want_status = fx["status"][:, pose]
    for i in range(len(status)):
        what = None
        if int(status[i]) != int(want_status[i]):
            what = "status %d, the fixture has %d" % (status[i], want_status[i])
        else:
            updated = status[i] == wire.PAIR_UPDATED
            want_p, want_c = (fx["pairs_post"][i, pose], fx["contacts_post"][i, pose]) if updated else (pre_pairs[i], pre_contacts[i])
            if pairs[i].tobytes() != want_p.tobytes():
                what = "pair state %s, want %s" % (pairs[i], want_p)
            elif contacts[i].tobytes() != want_c.tobytes():
                bad = [f for f in contacts.dtype.names if contacts[i][f].tobytes() != want_c[f].tobytes()]
                what = "contact fields %s: %s, want %s" % (bad, contacts[i], want_c)
            if what and not updated:
                what = "a SEPARATED slot was written: " + what
        if what:
            return "pose %d, pair %d (%s): %s" % (pose, i, type_pair_name(fx, i), what)
    return None


def run_chain(update, fx, check=True):
    """Carry `update`'s (update_contacts(bodies, origins, shapes, pairs, contacts) -> status) OWN output through every pose with the
    fixture's stamping and resets.  With `check` the first pose that differs from the fixture raises; returns the pair-poses whose
    status, pair state or contact differ from the fixture (0 with `check`)."""
    n, poses = fx["status"].shape
    pairs, contacts = fx["pairs_pre"][:, 0].copy(), fx["contacts_pre"][:, 0].copy()
    differing = 0
    for pose in range(poses):
        if pose > 0:
            advance(pairs, contacts, status, pose)
        pre_pairs, pre_contacts = pairs.copy(), contacts.copy()
        assert pre_pairs.tobytes() == np.ascontiguousarray(fx["pairs_pre"][:, pose]).tobytes(), "pose %d: the driver's pre-state" % pose
        assert pre_contacts.tobytes() == np.ascontiguousarray(fx["contacts_pre"][:, pose]).tobytes(), "pose %d: the driver's pre-state" % pose
        status = update(*world_at(fx, pose), pairs, contacts)
        message = first_difference(fx, pose, status, pairs, contacts, pre_pairs, pre_contacts)
        if message and check:
            raise AssertionError(message)
        if message:  # a mutation run: count, then go on from the fixture's state as the next pre-state is the fixture's
            updated = fx["status"][:, pose] == wire.PAIR_UPDATED
            want_p, want_c = pre_pairs.copy(), pre_contacts.copy()
            want_p[updated], want_c[updated] = fx["pairs_post"][updated, pose], fx["contacts_post"][updated, pose]
            differing += int(sum(status[i] != fx["status"][i, pose] or pairs[i].tobytes() != want_p[i].tobytes() or
                                 contacts[i].tobytes() != want_c[i].tobytes() for i in range(n)))
            pairs, contacts, status = want_p.copy(), want_c.copy(), fx["status"][:, pose].astype(np.int32)
    return differing


# ---- chains ----
def _aligned_shape(shape_type, rng):
    """A box, a level capsule or a level segment in exact binary fractions -> (shape, half width, half height)"""
    hx, hy = 0.25 * rng.randint(1, 4), 0.25 * rng.randint(1, 4)
    if shape_type == POLYGON:
        return box(hx, hy), hx, hy
    if shape_type == CAPSULE:
        return make_shape(CAPSULE, [(-hx, 0.0), (hx, 0.0)], 0.25), hx + 0.25, 0.25
    return make_shape(SEGMENT, [(-hx, 0.0), (hx, 0.0)]), hx, 0.0


def _random_shape(shape_type, j, which, rng):
    """Polygons of 3 to 8 vertices (every third one rounded), capsules and circles with radii, segments; pair 5 of the polygon pairs
    is two rounded 8-gons"""
    count = 3 + (j + 3 * which) % 6
    radius = 0.0
    if shape_type in (CAPSULE, CIRCLE) or (shape_type == POLYGON and j % 3 == 1):
        radius = 0.05 + 0.2 * rng.rand()
    if shape_type == POLYGON and j == 5:
        count, radius = 8, 0.1
    return make_shape(shape_type, shape_vertices(rng, shape_type, count, 1.0), radius)


def _distance(sa, pa, ra, sb, pb, rb):
    from tests import proximity_ref as pr
    return pr.shape_distance(pr.shape_proxy(sa), pr.transform(pa, ra), pr.shape_proxy(sb), pr.transform(pb, rb)).distance


def _offset_for_gap(sa, pa, ra, sb, rb, direction, gap):
    """How far along `direction` from A's origin B's origin lies when the reference's s2ShapeDistance between them is `gap` (0: where
    they begin to part): bisection, the distance being 0 while they overlap and growing from there"""
    lo, hi = 0.0, 6.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        pb = (f32(pa[0] + mid * direction[0]), f32(pa[1] + mid * direction[1]))
        if _distance(sa, pa, ra, sb, pb, rb) > gap:
            hi = mid
        else:
            lo = mid
    return lo if gap > 0 else hi


def chain_inputs():
    """-> shapes [2 PAIRS], origins, rots [PAIRS, POSES, 2, 2], fat [PAIRS, POSES, 2, 4].  Pair i has type pair i % 9 and is number
    j = i // 9 of it; it starts (5 j) % 12 poses into SCHEDULE and wraps, so every pose holds the whole mix.  Body A stays; body B's
    origin lies along a direction that turns TURN_PER_POSE a pose, at the schedule's gap, and B turns SPIN_PER_POSE a pose.  Every
    fourth pair of the five polygon-path type pairs is axis-aligned in exact binary fractions: straight up, B a quarter turn further
    every third pose."""
    rng = np.random.RandomState(20)
    shapes = np.zeros(2 * PAIRS, dtype=wire.shape_dtype)
    origins, rots = np.zeros((PAIRS, POSES, 2, 2), dtype=f32), np.zeros((PAIRS, POSES, 2, 2), dtype=f32)
    fat = np.zeros((PAIRS, POSES, 2, 4), dtype=f32)
    for i in range(PAIRS):
        (ta, tb), j = TYPE_PAIRS[i % len(TYPE_PAIRS)], i // len(TYPE_PAIRS)
        aligned = j % 4 == 0 and cq.REGISTERS[(ta, tb)] in cq.TAKES_CACHE
        centre = (f32(GRID * (i % COLUMNS)), f32(GRID * (i // COLUMNS)))
        shift = (5 * j) % POSES
        if aligned:
            sa, _, half_a = _aligned_shape(ta, rng)
            sb, half_bx, half_by = _aligned_shape(tb, rng)
            side = 0.25 * rng.randint(0, 2)
        else:
            sa, sb = _random_shape(ta, j, 0, rng), _random_shape(tb, j, 1, rng)
            pa = (f32(centre[0] + rng.rand() - 0.5), f32(centre[1] + rng.rand() - 0.5))
            angle_a, angle_b, heading = 6.28 * rng.rand(), 6.28 * rng.rand(), 6.28 * rng.rand()
        for pose in range(POSES):
            kind = SCHEDULE[(pose + shift) % POSES]
            if aligned:
                turns = pose // 3 if tb == POLYGON else 0
                pa, ra, rb = centre, QUARTER_TURNS[0], QUARTER_TURNS[turns % 4]
                reach = half_a + (half_bx if turns % 2 else half_by) + ALIGNED_GAP[kind]
                pb = (f32(centre[0] + side), f32(centre[1] + reach))
            else:
                ra, rb = rot_of(angle_a), rot_of(angle_b + SPIN_PER_POSE * pose)
                direction = (np.cos(heading + TURN_PER_POSE * pose), np.sin(heading + TURN_PER_POSE * pose))
                touch = _offset_for_gap(sa, pa, ra, sb, rb, direction, 0.0)
                if kind == "deep":
                    reach = 0.6 * touch
                elif GAP[kind] <= 0 or kind == "clear":
                    reach = max(touch + GAP[kind], 0.0)
                else:
                    reach = _offset_for_gap(sa, pa, ra, sb, rb, direction, GAP[kind])
                pb = (f32(pa[0] + reach * direction[0]), f32(pa[1] + reach * direction[1]))
            origins[i, pose], rots[i, pose] = (pa, pb), (ra, rb)
            fat[i, pose] = (fat_box(sa, pa, ra), fat_box(sb, pb, rb))
        sa["body"], sb["body"] = 2 * i, 2 * i + 1
        sa["proxyKey"], sb["proxyKey"] = ((2 * i) << 4) | wire.BODY_DYNAMIC, ((2 * i + 1) << 4) | wire.BODY_DYNAMIC
        shapes[2 * i], shapes[2 * i + 1] = sa, sb
    return shapes, origins, rots, fat


# ---- directed ----
def _touching_boxes(axis, side, want):
    """Two unit boxes whose fat boxes, by fat_box's own float32 arithmetic, differ on `axis` by exactly 0 (want "touch") or by one ulp
    (want "ulp"), B on the positive (`side` 1: the test's d1) or the negative (-1: d2) side of A -> (origin of A, origin of B)"""
    sh, level = box(0.5, 0.5), QUARTER_TURNS[0]
    for step_a in range(64):
        pa = [f32(0.0), f32(0.0)]
        pa[axis] = f32(step_a / 64.0)
        fa = fat_box(sh, pa, level)
        coord = f32(pa[axis] + side * 1.04)
        for _ in range(64):
            coord = np.nextafter(coord, f32(-side * np.inf))  # from a little inside, outwards
        for _ in range(128):
            pb = [f32(0.3), f32(0.3)]
            pb[axis] = coord
            fb = fat_box(sh, pb, level)
            d = f32(fb[axis] - fa[axis + 2]) if side > 0 else f32(fa[axis] - fb[axis + 2])
            edge = fa[axis + 2] if side > 0 else fb[axis + 2]
            if (want == "touch" and d == 0) or (want == "ulp" and d > 0 and d == f32(np.nextafter(edge, f32(np.inf)) - edge)):
                return tuple(pa), tuple(pb)
            coord = np.nextafter(coord, f32(side * np.inf))
    raise AssertionError("no such placement")


def directed_cases():
    """[(what, shape A, (origin, angle) of A, shape B, (origin, angle) of B, status, point count or None, pre-state)]: the status and,
    where given, the point count are what the case is there for and are asserted in words; everything else is in the fixture's bytes.
    The pre-state is "fresh" (a new contact) but for two rows that enter with the manifold, the ids and the warm cache of a first update
    and stamped points: "same ids" has both old ids equal to the new point 0's, which no manifold function returns, but it is the one
    input that tells s2UpdateContact's first-match-wins search from any other order; "swapped ids" has the old ids exchanged, so
    that each new point takes the other old point's impulses."""
    U, S = wire.PAIR_UPDATED, wire.PAIR_SEPARATED
    unit, point = box(0.5, 0.5), [(0.0, 0.0)]
    circle = make_shape(CIRCLE, point, 0.3)
    capsule = make_shape(CAPSULE, [(-0.5, 0.0), (0.5, 0.0)], 0.2)
    segment = make_shape(SEGMENT, [(-1.0, 0.0), (1.0, 0.0)])
    octagon = make_shape(POLYGON, [(0.5 * np.cos(0.2 + np.pi * k / 4), 0.4 * np.sin(0.2 + np.pi * k / 4)) for k in range(8)], 0.1)
    inside = f32(f32(1.0) + SPECULATIVE)      # 1.02 rounds down: the gap 1.02f - 1 is just below 4 * linearSlop
    outside = np.nextafter(inside, f32(2.0))  # ... and one ulp further it is just above
    cases = [
        ("coincident circles: no direction between the centres, the zero normal", circle, ((0, 0), 0.3), circle, ((0, 0), 1.0), U, 1),
        ("a circle centred on a capsule's axis", capsule, ((0, 0), 0.4), circle, ((0.25 * np.cos(0.4), 0.25 * np.sin(0.4)), 0.0), U, 1),
        ("a circle centred on a segment", segment, ((0, 0), 0.0), circle, ((0.5, 0.0), 0.0), U, 1),
        ("a circle centred on a polygon's centre", unit, ((0, 0), 0.2), circle, ((0, 0), 0.0), U, 1),
        ("a circle centred on a polygon's vertex", unit, ((0, 0), 0.0), circle, ((0.5, 0.5), 0.0), U, 1),
        ("a circle centred on a rounded 8-gon's vertex", octagon, ((0, 0), 0.0), circle, (tuple(octagon["vertices"][3]), 0.0), U, 1),
        ("flush boxes: a whole face shared", unit, ((0, 0), 0.0), unit, ((1.0, 0.0), 0.0), U, 2),
        ("corner-to-corner boxes: one point in common", unit, ((0, 0), 0.0), unit, ((1.0, 1.0), 0.0), U, None),
        ("corner-to-corner boxes, one turned an eighth: vertex on vertex", unit, ((0, 0), 0.0), unit, ((0.5 + 0.5 * np.sqrt(2.0), 0.5), np.pi / 4), U, None),
        ("corner-to-corner boxes 0.01 apart each way: vertex to vertex, one speculative point", unit, ((0, 0), 0.0), unit, ((1.01, 1.01), 0.0), U, 1),
        ("coincident boxes", unit, ((0, 0), 0.0), unit, ((0, 0), 0.0), U, 2),
        ("coincident boxes, turned", unit, ((0, 0), 0.7), unit, ((0, 0), 0.7), U, 2),
        ("collinear capsules, end to end", capsule, ((0, 0), 0.0), capsule, ((1.3, 0.0), 0.0), U, None),
        ("collinear capsules, overlapping along the axis", capsule, ((0, 0), 0.0), capsule, ((0.5, 0.0), 0.0), U, None),
        ("parallel capsules, side by side", capsule, ((0, 0), 0.0), capsule, ((0.25, 0.35), 0.0), U, 2),
        ("crossing capsules", capsule, ((0, 0), 0.0), capsule, ((0, 0), np.pi / 2), U, None),
        ("crossing capsules, askew", capsule, ((0, 0), 0.3), capsule, ((0.1, 0.05), 1.2), U, None),
        ("a segment through a box", segment, ((0, 0), 0.0), unit, ((0, 0), 0.0), U, 2),
        ("a segment through a box, askew", segment, ((0, 0), 0.5), unit, ((0.1, 0.1), 0.0), U, 2),
        ("a segment along a box's edge", segment, ((0, 0), 0.0), unit, ((0, -0.5), 0.0), U, 2),
        ("a segment crossing a capsule", segment, ((0, 0), 0.0), capsule, ((0, 0), np.pi / 2), U, None),
        ("rounded 8-gons, overlapping", octagon, ((0, 0), 0.3), octagon, ((0.9, 0.2), 1.1), U, None),
        ("rounded 8-gons, in the speculative band", octagon, ((0, 0), 0.0), octagon, ((1.17, 0.0), np.pi / 8), U, None),
        ("a polygon on a capsule", unit, ((0, 0), 0.0), capsule, ((0, 0.69), 0.0), U, 2),
        ("box on box, both old points carry new point 0's id: the first one's impulses are taken", unit, ((0, 0), 0.0), unit, ((0.25, 0.995), 0.0), U, 2, "same ids"),
        ("box on box, the old points' ids exchanged: the impulses cross over", unit, ((0, 0), 0.0), unit, ((0.25, 0.995), 0.0), U, 2, "swapped ids"),
        ("boxes 5,000 m from the origin", unit, ((5000.0, 5000.0), 0.3), unit, ((5000.75, 5000.5), 0.9), U, None),
        ("a circle on a box 5,000 m from the origin", unit, ((-5000.0, 5000.0), 0.3), circle, ((-5000.5, 5000.5), 0.0), U, 1),
    ]
    # (left out: a zero-length capsule against a circle -- the reference divides 0 by 0 and its separation is NaN, whose sign and payload
    # need not agree between an x86 and the GPU; that would test nothing of ours)
    # the fat-box test at equality: the reference tests d > 0, so boxes that touch exactly are updated, and one ulp apart they are not
    for axis, side, want, status in ((0, 1, "touch", U), (1, -1, "touch", U), (1, 1, "ulp", S), (0, -1, "ulp", S)):
        pa, pb = _touching_boxes(axis, side, want)
        cases.append(("fat boxes that %s on axis %d, B on side %+d" % ("touch exactly" if want == "touch" else "miss by one ulp", axis, side),
                      unit, (pa, 0.0), unit, (pb, 0.0), status, 0 if status == U else None))
    # the speculative band, B above A and B below A: box on box at separations -0.005, 0, +0.01, just inside and just outside 4 * linearSlop
    for side in (1.0, -1.0):
        for what, y, points in (("0.005 deep", f32(0.995), 2), ("touching", f32(1.0), 2), ("0.01 apart", f32(1.01), 2),
                                ("just inside the speculative distance", inside, 2), ("just outside the speculative distance", outside, 0)):
            cases.append(("box %s box, %s" % ("on" if side > 0 else "under", what), unit, ((0, 0), 0.0), unit, ((0.0, side * y), 0.0), U, points))
    return [c if len(c) == 8 else c + ("fresh",) for c in cases]


BAND_ROWS = 10      # the last rows of directed_cases()
FAT_BOX_ROWS = 4    # ... and the rows before those


def directed_inputs():
    cases = directed_cases()
    n = len(cases)
    shapes = np.zeros(2 * n, dtype=wire.shape_dtype)
    origins, rots, fat = np.zeros((n, 1, 2, 2), dtype=f32), np.zeros((n, 1, 2, 2), dtype=f32), np.zeros((n, 1, 2, 4), dtype=f32)
    for i, (_, sa, (pa, angle_a), sb, (pb, angle_b), _, _, _) in enumerate(cases):
        # (no grid here: stage 3 looks at the named pair alone, and the edge rows need their coordinates exactly as stated)
        sa, sb = sa.copy(), sb.copy()
        pa, pb = (f32(pa[0]), f32(pa[1])), (f32(pb[0]), f32(pb[1]))
        ra, rb = (QUARTER_TURNS[0] if angle_a == 0 else rot_of(angle_a)), (QUARTER_TURNS[0] if angle_b == 0 else rot_of(angle_b))
        origins[i, 0], rots[i, 0], fat[i, 0] = (pa, pb), (ra, rb), (fat_box(sa, pa, ra), fat_box(sb, pb, rb))
        sa["body"], sb["body"] = 2 * i, 2 * i + 1
        shapes[2 * i], shapes[2 * i + 1] = sa, sb
    return shapes, origins, rots, fat


# ---- fixtures ----
INPUTS = {"chains": chain_inputs, "directed": directed_inputs}


def build_fixture(name):
    """The inputs and the statement's answers, the statement's own output carried from pose to pose"""
    from tests import narrow_chain_ref as ref
    shapes, origins, rots, fat = INPUTS[name]()
    n, poses = origins.shape[:2]
    fx = {"shapes": shapes, "origins": origins, "rots": rots, "fat": fat, "status": np.zeros((n, poses), dtype=np.int8)}
    for key, dtype in (("pairs_pre", wire.pair_state_dtype), ("pairs_post", wire.pair_state_dtype), ("contacts_pre", wire.contact_dtype),
                       ("contacts_post", wire.contact_dtype)):
        fx[key] = np.zeros((n, poses), dtype=dtype)
    pairs, contacts = fresh(n)
    if name == "directed":
        first_p, first_c = fresh(n)
        ref.update_contacts(*world_at(fx, 0), first_p, first_c)
        for i, case in enumerate(directed_cases()):
            if case[7] != "fresh":
                pairs[i], contacts[i] = first_p[i], first_c[i]
                pairs["id"][i] = first_p["id"][i][0] if case[7] == "same ids" else first_p["id"][i][::-1]
        stamp(contacts, 0)
    for pose in range(poses):
        if pose > 0:
            advance(pairs, contacts, status, pose)
        fx["pairs_pre"][:, pose], fx["contacts_pre"][:, pose] = pairs, contacts
        status = ref.update_contacts(*world_at(fx, pose), pairs, contacts)
        fx["status"][:, pose], fx["pairs_post"][:, pose], fx["contacts_post"][:, pose] = status, pairs, contacts
    return fx


def parts_of(name):
    return PARTS if name == "chains" else 1


def fixture_path(name, part):
    return os.path.join(GOLDEN, "%s_%d.npz" % (name, part) if parts_of(name) > 1 else "%s.npz" % name)


def part_slices(name, n):
    edges = np.linspace(0, n, parts_of(name) + 1).astype(int)
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def load_fixture(name):
    loaded = [np.load(fixture_path(name, part)) for part in range(parts_of(name))]
    return {k: np.ascontiguousarray(np.concatenate([d[k] for d in loaded])) for k in loaded[0].files}


def save_fixture(name, fx):
    os.makedirs(GOLDEN, exist_ok=True)
    n = len(fx["status"])
    for part, rows in enumerate(part_slices(name, n)):
        shape_rows = slice(2 * rows.start, 2 * rows.stop)
        np.savez_compressed(fixture_path(name, part), **{k: v[shape_rows if k == "shapes" else rows] for k, v in fx.items()})


def _floats(a):
    if a.dtype.names:
        return np.concatenate([_floats(a[f]) for f in a.dtype.names])
    return a.ravel().astype(np.float64) if a.dtype.kind == "f" else np.zeros(0)


def coverage(fx):
    """What a fixture holds, from the fixture alone (the counts the host test's conditions are about)"""
    status, pre_p, post_p, pre_c, post_c = (fx[k] for k in ("status", "pairs_pre", "pairs_post", "contacts_pre", "contacts_post"))
    n, poses = status.shape
    updated = status == wire.PAIR_UPDATED
    names = np.array([type_pair_name(fx, i) for i in range(n)])
    out = {"pair-poses": n * poses, "finite": bool(all(np.isfinite(_floats(fx[k])).all() for k in fx)),
           "separated": int((status == wire.PAIR_SEPARATED).sum()),
           "updated per type pair": {fn: int(updated[names == fn].sum()) for fn in sorted(set(names.tolist()))}}
    out["entering cache counts"] = {fn: [int((updated & (pre_p["cacheCount"] == c))[names == fn].sum()) for c in range(4)] for fn in sorted(cq.TAKES_CACHE)}
    out["point counts"] = {fn: [int((updated & (post_c["pointCount"] == c))[names == fn].sum()) for c in range(3)] for fn in sorted(cq.TAKES_CACHE)}
    out["count changes"] = {"%d->%d" % (a, b): int((updated & (pre_c["pointCount"] == a) & (post_c["pointCount"] == b)).sum())
                            for a in range(3) for b in range(3) if a != b}
    carried = 0
    for i, pose in zip(*np.nonzero(updated)):
        for p in range(int(post_c["pointCount"][i, pose])):
            if post_p["persisted"][i, pose][p]:
                value = post_c["points"][i, pose][p]["normalImpulse"]
                carried += int(value != 0 and any(value == stamp_value(pose, i, j, 0) for j in range(2)))
    out["persisted points with their stamped impulses"] = carried
    same = updated & (pre_c["pointCount"] == post_c["pointCount"]) & (post_c["pointCount"] > 0)
    out["same count, an id lost"] = int((same & (post_c["frictionPersisted"] == 0)).sum())
    out["one point persisted beside one that is not"] = int((updated & (post_c["pointCount"] == 2) & (post_p["persisted"].sum(axis=-1) == 1)).sum())
    out["born mid-chain"] = int((updated[:, 1:] & (status[:, :-1] == wire.PAIR_SEPARATED)).sum())
    return out


if __name__ == "__main__":
    for fixture in INPUTS:
        built = build_fixture(fixture)
        save_fixture(fixture, built)
        sizes = [os.path.getsize(fixture_path(fixture, part)) for part in range(parts_of(fixture))]
        print("%s: %d pairs, %d poses, files of %s bytes" % (fixture, built["status"].shape[0], built["status"].shape[1], sizes))
        for key, value in coverage(built).items():
            print("  %s: %s" % (key, value))
