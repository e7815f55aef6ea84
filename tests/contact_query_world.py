"""Query batches of the contact-query tests (tests/test_contact_query_host.py, tests/test_gpu_contact_query.py) and the generator of
their fixtures tests/golden/contact_query/*.npz (python -m tests.contact_query_world, with oracle/_ref/libs2ref.so built).  Test
infrastructure only.

The worlds are the three of tests/scene_query_world.py, read from its fixtures (zoo: 54 shapes of all four types in one tile; pyramid30:
466 polygons resting on each other in two tiles; synthetic: 335 slots with rotated bodies, free slots and the directed cases).  A
fixture here holds one fixed batch of QUERIES queries and what the statement (tests/contact_query_ref.py) answers: the collide-shape
lists and the deepest-contact records."""
import os

import numpy as np

from solver2d_amd import wire
from tests import scene_query_world as sq

f32 = np.float32
ALL = 0xFFFFFFFF
FIXTURES = sq.FIXTURES
QUERIES = 256
RESULT_KEYS = ("offsets", "hits", "deepest")
SEEDS = {"zoo": 31, "pyramid30": 32, "synthetic": 33}
SCALES = {"zoo": 1.0, "pyramid30": 0.4, "synthetic": 0.3}  # the query sizes: the denser the world, the smaller, to keep the lists short
CROWD = {"zoo": None, "pyramid30": None, "synthetic": 9}    # ... and in a world of stacked families, only shapes with few neighbours are aimed at
CAPSULE, CIRCLE, POLYGON, SEGMENT = wire.SHAPE_CAPSULE, wire.SHAPE_CIRCLE, wire.SHAPE_POLYGON, wire.SHAPE_SEGMENT
BOX = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]


def fixture_path(name):
    return os.path.join(sq.GOLDEN, "contact_query", "%s.npz" % name)


def load_fixture(name):
    """The contact-query fixture with the world of the scene-query fixture of the same name beside it (bodies, shapes, origins)"""
    d = np.load(fixture_path(name))
    fx = {k: np.ascontiguousarray(d[k]) for k in d.files}
    world = sq.load_fixture(name)
    fx.update({k: world[k] for k in ("bodies", "shapes", "origins")})
    return fx


def edge_normals(vertices):
    """s2Normalize(s2CrossVS(edge, 1)) per edge of a counter-clockwise polygon, as s2MakePolygon computes them (src/geometry.c:22-60)"""
    v = np.asarray(vertices, dtype=f32)
    edge = np.roll(v, -1, axis=0) - v
    normal = np.stack([edge[:, 1], -edge[:, 0]], axis=1).astype(f32)
    return (normal / np.sqrt((normal * normal).sum(axis=1, dtype=f32))[:, None]).astype(f32)


def make_query(shape_type, vertices, radius, position, angle, mask=ALL):
    q = np.zeros(1, dtype=wire.contact_query_dtype)[0]
    q["vertices"][:len(vertices)] = vertices
    q["type"], q["radius"], q["position"] = shape_type, radius, position
    if shape_type == POLYGON:
        q["count"] = len(vertices)
        q["normals"][:len(vertices)] = edge_normals(vertices)
    q["rot"] = (np.sin(angle), np.cos(angle))
    q["maskBits"] = mask
    return q


def shape_vertices(rng, shape_type, count, size):
    """A shape of the type in its own frame, about `size` across: a point near the origin, a slanted segment, or a convex polygon
    (counter-clockwise points on an ellipse)"""
    if shape_type == CIRCLE:
        return [tuple((rng.rand(2) * 0.2 - 0.1) * size)]
    if shape_type in (CAPSULE, SEGMENT):
        h = (0.3 + 0.4 * rng.rand()) * size
        return [(-h, 0.1 * size), (h, -0.1 * size)]
    a0, rx, ry = rng.rand() * 6.28, (0.3 + 0.3 * rng.rand()) * size, (0.2 + 0.3 * rng.rand()) * size
    return [(rx * np.cos(a0 + 2 * np.pi * i / count), ry * np.sin(a0 + 2 * np.pi * i / count)) for i in range(count)]


def special_cases():
    """The directed queries of the synthetic world and the shape each must name as deepest (-1: none; None: not stated), see
    sq.synthetic_world(): two identical circles in both tiles, a masked-out shape that would otherwise win, a box on a box, the
    speculative band from both sides, candidates without a hit, no candidate"""
    point = [(0.0, 0.0)]
    cases = [
        (make_query(CIRCLE, point, 0.1, (20.0, 20.0), 0.0), sq.TIE_LOW),            # the same manifold from both: the lower slot
        (make_query(CAPSULE, [(-0.2, 0.0), (0.2, 0.0)], 0.1, (20.0, 20.5), 0.4), sq.TIE_LOW),
        (make_query(CIRCLE, point, 0.8, (20.8, 30.0), 0.0), sq.MASKED_NEAR),        # every category: the nearer circle is deeper
        (make_query(CIRCLE, point, 0.8, (20.8, 30.0), 0.0, 1), sq.MASKED_FAR),      # the nearer one masked out
        (make_query(CIRCLE, point, 0.8, (20.8, 30.0), 0.0, 4), -1),                 # both masked out
        (make_query(POLYGON, BOX, 0.0, (30.0, 30.995), 0.0), sq.BIG_BOX),           # a box resting on the box: two points, 0.005 deep
        (make_query(POLYGON, BOX, 0.0, (30.0, 31.0), 0.0), sq.BIG_BOX),             # touching
        (make_query(POLYGON, BOX, 0.0, (30.0, 31.01), 0.0), sq.BIG_BOX),            # inside the speculative band: separation +0.01
        (make_query(POLYGON, BOX, 0.0, (30.0, 31.03), 0.0), -1),                    # beyond it: a candidate, no hit
        (make_query(CIRCLE, point, 0.1, (30.61, 30.0), 0.0), sq.BIG_BOX),           # a circle 0.01 off the box's face
        (make_query(CIRCLE, point, 0.1, (30.7, 30.7), 0.0), -1),                    # off its corner: boxes overlap, no hit
        (make_query(SEGMENT, [(-1.0, 0.0), (1.0, 0.0)], 0.0, (30.0, 30.5), 0.0), sq.BIG_BOX),  # a segment along the box's upper edge
        (make_query(SEGMENT, [(-1.0, 0.0), (1.0, 0.0)], 0.0, (30.0, 20.0), 0.7), sq.BIG_CIRCLE),
        (make_query(CAPSULE, [(-0.3, 0.0), (0.3, 0.0)], 0.2, (40.0, 20.6), 0.0), sq.FAR_CIRCLE),
        (make_query(POLYGON, BOX, 0.1, (1000.0, 1000.0), 0.3), -1),                 # no candidate
        (make_query(CIRCLE, point, 0.25, (0.0, 0.0), 0.0), None),                   # on the zeroed boxes of the free slots: never a free slot
        (make_query(SEGMENT, [(0.0, 0.0), (1.0, 1.0)], 0.0, (30.51, 30.51), 0.0), sq.BIG_BOX),  # its end 0.014 off the box's corner: one point
    ]
    return np.array([c[0] for c in cases], dtype=wire.contact_query_dtype), [c[1] for c in cases]


def _extent(sh):
    fat = sh["fatAABB"]
    return 0.5 * float(min(fat[2] - fat[0], fat[3] - fat[1]))


def make_batch(world, count, seed, special=None, scale=1.0, crowd=None):
    """A fixed batch.  Query i has type i % 4 (capsule, circle, polygon, segment); polygons have 3 + (i // 4) % 6 vertices and a radius
    when (i // 8) is odd; capsules and circles always have one.  Fifteen of sixteen are placed relative to a shape (the world's shape
    types in turn, (i // 4) % types): its centre plus an offset that runs from 0 to a little more than the shape's half width plus
    the query's, so that most overlap, some touch and some lie in the speculative band or just beyond; the rest lie clear above a
    shape.  Every 32nd query has a narrow mask."""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = np.nonzero(shapes["type"] != wire.SHAPE_FREE)[0]
    small = live[(shapes["fatAABB"][live][:, 2] - shapes["fatAABB"][live][:, 0]) < 20.0]
    if crowd is not None:
        fat = shapes["fatAABB"][live]
        near = [int(((fat[:, 0] <= shapes["fatAABB"][s][2]) & (shapes["fatAABB"][s][0] <= fat[:, 2]) & (fat[:, 1] <= shapes["fatAABB"][s][3]) &
                     (shapes["fatAABB"][s][1] <= fat[:, 3])).sum()) - 1 for s in small]
        small = small[np.array(near) <= crowd]
    by_type = [small[shapes["type"][small] == t] for t in sorted(set(shapes["type"][small].tolist()))]
    queries = np.zeros(count, dtype=wire.contact_query_dtype)
    for i in range(count):
        shape_type = (CAPSULE, CIRCLE, POLYGON, SEGMENT)[i % 4]
        group = by_type[(i // 4) % len(by_type)]
        slot = int(group[rng.randint(len(group))])
        extent = _extent(shapes[slot])
        size = scale * min(max(extent, 0.2), 0.6)
        radius = 0.0
        if shape_type in (CAPSULE, CIRCLE) or (shape_type == POLYGON and (i // 8) % 2 == 1):
            radius = (0.1 + 0.3 * rng.rand()) * size
        angle = 0.0 if i % 3 == 0 else rng.rand() * 6.28
        reach = [0.0, 0.4, 0.8, 1.0, 1.1, 1.2, 1.3][(i // 4) % 7] * (extent + 0.5 * size * rng.rand())
        direction = rng.rand() * 6.28 if i % 5 else 1.5708 * rng.randint(4)
        position = sq._centre(world, slot) + f32(reach) * np.array([np.cos(direction), np.sin(direction)], dtype=f32)
        if i % 16 == 15:
            position = sq._centre(world, slot) + np.array([0.0, 50.0 + i], dtype=f32)
        queries[i] = make_query(shape_type, shape_vertices(rng, shape_type, 3 + (i // 4) % 6, size), radius, position.astype(f32), angle)
        if i % 32 == 17:
            queries[i]["maskBits"] = [1, 2, 0xFFFF0000, 0][(i // 32) % 4]
    if special is not None:
        queries[:len(special)] = special
    return queries


def expected(world, queries):
    from tests import contact_query_ref as ref
    offsets, hits = ref.collide_shape(world, queries)
    return {"offsets": offsets, "hits": hits, "deepest": ref.deepest_contact(world, queries)}


def build_fixture(name):
    world = sq.fixture_world(sq.load_fixture(name))
    queries = make_batch(world, QUERIES, SEEDS[name], special_cases()[0] if name == "synthetic" else None, SCALES[name], CROWD[name])
    fx = {"queries": queries}
    fx.update(expected(world, queries))
    return fx


if __name__ == "__main__":
    os.makedirs(os.path.dirname(fixture_path("zoo")), exist_ok=True)
    for fixture in FIXTURES:
        built = build_fixture(fixture)
        np.savez_compressed(fixture_path(fixture), **built)
        hits, counts = built["hits"], np.diff(built["offsets"])
        print("%s: %d queries, %d with a hit, %d entries (%d with two points, %d speculative), longest list %d, %d bytes" % (
            fixture, len(counts), int((counts > 0).sum()), len(hits), int((hits["pointCount"] == 2).sum()),
            int((hits["points"]["separation"][:, 0] > 0).sum()), int(counts.max()), os.path.getsize(fixture_path(fixture))))
