"""Query batches of the proximity-query tests (tests/test_proximity_host.py, tests/test_gpu_proximity.py) and the generator of their
fixtures tests/golden/proximity/*.npz (python -m tests.proximity_world, with oracle/_ref/libs2ref.so built).  Test infrastructure only.

The worlds are the three of tests/scene_query_world.py, read from its fixtures (zoo: 54 shapes of all four types in one tile; pyramid30:
466 polygons resting on each other in two tiles; synthetic: 335 slots with rotated bodies, free slots and the directed cases).  A
fixture here holds one fixed batch of QUERIES queries and what the statement (tests/proximity_ref.py) answers: the closest-shape
records and the in-range lists with their distances."""
import os

import numpy as np

from solver2d_amd import wire
from tests import scene_query_world as sq

f32 = np.float32
ALL = 0xFFFFFFFF
FIXTURES = sq.FIXTURES
QUERIES = 256
RESULT_KEYS = ("hits", "range_offsets", "range_shapes", "range_distances")
SEEDS = {"zoo": 21, "pyramid30": 22, "synthetic": 23}


def fixture_path(name):
    return os.path.join(sq.GOLDEN, "proximity", "%s.npz" % name)


def load_fixture(name):
    """The proximity fixture with the world of the scene-query fixture of the same name beside it (bodies, shapes, origins)"""
    d = np.load(fixture_path(name))
    fx = {k: np.ascontiguousarray(d[k]) for k in d.files}
    world = sq.load_fixture(name)
    fx.update({k: world[k] for k in ("bodies", "shapes", "origins")})
    return fx


def make_query(vertices, radius, position, angle, max_distance, mask=ALL):
    q = np.zeros(1, dtype=wire.proximity_query_dtype)[0]
    q["vertices"][:len(vertices)] = vertices
    q["count"], q["radius"], q["position"] = len(vertices), radius, position
    q["rot"] = (np.sin(angle), np.cos(angle))
    q["maxDistance"], q["maskBits"] = max_distance, mask
    return q


def proxy_vertices(rng, count):
    """A proxy of `count` vertices in its own frame: a point near the origin, a segment, or a convex polygon (counter-clockwise points
    on an ellipse), up to about half a metre across"""
    if count == 1:
        return [tuple(rng.rand(2) * 0.2 - 0.1)]
    if count == 2:
        h = 0.1 + 0.4 * rng.rand()
        return [(-h, 0.05), (h, -0.05)]
    a0, rx, ry = rng.rand() * 6.28, 0.15 + 0.3 * rng.rand(), 0.1 + 0.2 * rng.rand()
    return [(rx * np.cos(a0 + 2 * np.pi * i / count), ry * np.sin(a0 + 2 * np.pi * i / count)) for i in range(count)]


def special_cases():
    """The directed queries of the synthetic world and the shape each must name as closest (-1: none), see sq.synthetic_world():
    two identical circles in both tiles, a masked-out shape that would otherwise win, a shape just beyond maxDistance, free slots"""
    point = [(0.0, 0.0)]
    beyond = np.nextafter(f32(1.5), f32(0.0))
    cases = [
        (make_query(point, 0.1, (17.0, 20.0), 0.0, 5.0), sq.TIE_LOW),              # the same distance to both: the lower slot
        (make_query(point, 0.1, (20.0, 20.0), 0.0, 0.0), sq.TIE_LOW),              # inside both: distance 0 twice
        (make_query(point, 0.0, (19.0, 30.0), 0.0, 5.0), sq.MASKED_NEAR),          # every category: the nearer circle
        (make_query(point, 0.0, (19.0, 30.0), 0.0, 5.0, 1), sq.MASKED_FAR),        # the nearer one masked out
        (make_query(point, 0.0, (19.0, 30.0), 0.0, 5.0, 4), -1),                   # both masked out
        (make_query(point, 0.0, (38.0, 20.0), 0.0, 1.5), sq.FAR_CIRCLE),           # the circle at (40, 20), radius 0.5: exactly 1.5 away
        (make_query(point, 0.0, (38.0, 20.0), 0.0, beyond), -1),                   # ... and one ulp less reaches nothing
        (make_query(point, 0.0, (0.0, 0.0), 0.0, 0.0), None),                      # on the zeroed boxes of the free slots: never a free slot
        (make_query(point, 0.25, (0.0, 0.0), 0.0, 3.0), None),
        (make_query([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)], 0.0, (31.0, 30.0), 0.0, 0.0), sq.BIG_BOX),  # two boxes sharing an edge
        (make_query([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)], 0.0, (31.5, 30.0), 0.0, 0.25), -1),
    ]
    return np.array([c[0] for c in cases], dtype=wire.proximity_query_dtype), [c[1] for c in cases]


def _extent(sh):
    fat = sh["fatAABB"]
    return 0.5 * float(np.hypot(fat[2] - fat[0], fat[3] - fat[1]))


def make_batch(world, count, seed, special=None):
    """A fixed batch.  Query i has 1 + i % 8 proxy vertices, a radius when (i // 8) is odd, and an angle unless i % 3 == 0.  Seven of
    eight are placed relative to a shape (the shape types in turn): its centre plus an offset shorter than the shape's extent plus
    maxDistance -- a quarter of them at the centre itself; the rest lie clear above a shape or anywhere over the shapes, with maxDistance
    2.  Otherwise maxDistance runs through 0, 0.1, 0.5, 1, 2."""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = np.nonzero(shapes["type"] != wire.SHAPE_FREE)[0]
    small = live[(shapes["fatAABB"][live][:, 2] - shapes["fatAABB"][live][:, 0]) < 20.0]
    slo, shi = shapes["fatAABB"][small][:, :2].min(axis=0) - 1.0, shapes["fatAABB"][small][:, 2:].max(axis=0) + 1.0
    by_type = [small[shapes["type"][small] == t] for t in sorted(set(shapes["type"][small].tolist()))]
    # the spots two extents above a shape's centre that no fat box covers
    fat = shapes["fatAABB"][live]
    above = [sq._centre(world, int(s)) + np.array([0.0, 2.0 * _extent(shapes[s])], dtype=f32) for s in small]
    clear = [p for p in above if not ((fat[:, 0] <= p[0]) & (p[0] <= fat[:, 2]) & (fat[:, 1] <= p[1]) & (p[1] <= fat[:, 3])).any()]
    queries = np.zeros(count, dtype=wire.proximity_query_dtype)
    for i in range(count):
        n = 1 + i % 8
        radius = 0.0 if (i // 8) % 2 == 0 else 0.05 + 0.25 * rng.rand()
        angle = 0.0 if i % 3 == 0 else rng.rand() * 6.28
        max_distance = [0.0, 0.1, 0.5, 1.0, 2.0][(i // 2) % 5]
        placement = (i // 8 + i) % 8
        if placement < 7:
            group = by_type[i % len(by_type)]
            slot = int(group[rng.randint(len(group))])
            reach = (_extent(shapes[slot]) + max_distance) * rng.rand()
            if placement < 2:
                reach = 0.0
            direction = rng.rand() * 6.28
            position = sq._centre(world, slot) + f32(reach) * np.array([np.cos(direction), np.sin(direction)], dtype=f32)
        elif i % 16 < 8 and len(clear):
            # (a pile is dense: only what lies clear of it finds its shapes at a distance)
            position = clear[rng.randint(len(clear))] + (rng.rand(2) * 0.2 - 0.1)
            max_distance = 2.0
        else:
            position = slo + (shi - slo) * rng.rand(2)
            max_distance = 2.0
        queries[i] = make_query(proxy_vertices(rng, n), radius, position.astype(f32), angle, max_distance)
        if i % 32 == 17:
            queries[i]["maskBits"] = [1, 2, 0xFFFF0000, 0][(i // 32) % 4]
    if special is not None:
        queries[:len(special)] = special
    return queries


def placed_relative_to_a_shape(count):
    return sum(1 for i in range(count) if (i // 8 + i) % 8 < 7)


def expected(world, queries):
    from tests import proximity_ref as ref
    offsets, shapes, distances = ref.shapes_in_range(world, queries)
    return {"hits": ref.closest_shape(world, queries), "range_offsets": offsets, "range_shapes": shapes, "range_distances": distances}


def build_fixture(name):
    world = sq.fixture_world(sq.load_fixture(name))
    queries = make_batch(world, QUERIES, SEEDS[name], special_cases()[0] if name == "synthetic" else None)
    fx = {"queries": queries}
    fx.update(expected(world, queries))
    return fx


def zero_ties(fx):
    """Queries whose in-range list holds two or more shapes at distance 0"""
    o, d = fx["range_offsets"], fx["range_distances"]
    return sum(1 for i in range(len(fx["queries"])) if (d[o[i]:o[i + 1]] == 0).sum() >= 2)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(fixture_path("zoo")), exist_ok=True)
    for fixture in FIXTURES:
        built = build_fixture(fixture)
        np.savez_compressed(fixture_path(fixture), **built)
        hits = built["hits"]
        print("%s: %d queries, %d name a shape (%d at distance 0, %d beyond), %d lists non-empty, %d entries, %d ties at 0, %d bytes" % (
            fixture, len(hits), int((hits["shape"] >= 0).sum()), int(((hits["shape"] >= 0) & (hits["distance"] == 0)).sum()),
            int(((hits["shape"] >= 0) & (hits["distance"] > 0)).sum()), int((np.diff(built["range_offsets"]) > 0).sum()), len(built["range_shapes"]),
            zero_ties(built), os.path.getsize(fixture_path(fixture))))
