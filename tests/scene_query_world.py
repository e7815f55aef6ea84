"""Worlds and query batches of the scene-query tests (tests/test_scene_queries_host.py, tests/test_gpu_scene_queries.py), and the
generator of their fixtures tests/golden/scene_query/*.npz (python -m tests.scene_query_world, with oracle/_ref/libs2ref.so built).
Test infrastructure only.

A fixture holds the wire arrays of a world the queries read (bodies, shapes, origins), one fixed batch of queries and what the statement
(tests/scene_query_ref.py) answers:
  zoo        the reference's shapes_zoo after 30 steps: 54 shapes of all four types in one tile; 512 rays, 256 probes, 64 boxes
  pyramid30  the reference's pyramid 30 after 20 steps: 466 shapes in two tiles, hits in both and winners in the second
  synthetic  tests/shape_report_world.py's 331 slots (rotated bodies, free slots, two tiles) with polygon normals and the directed
             cases of `special_cases` added."""
import os

import numpy as np

from solver2d_amd import synthetic, wire
from tests import oraclebind, shape_report_world

f32 = np.float32
ALL = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("zoo", "pyramid30", "synthetic")
BATCH = {"zoo": (512, 256, 64), "pyramid30": (512, 256, 64), "synthetic": (384, 192, 48)}
QUERY_KEYS = ("rays", "probes", "boxes")
RESULT_KEYS = ("hits", "probe_offsets", "probe_shapes", "box_offsets", "box_shapes")

# the directed part of the synthetic world: slots in both tiles, well away from the falling families
TIE_LOW, TIE_HIGH = 5, 331            # two identical circles on one body, first tile and second tile
MASKED_NEAR, MASKED_FAR = 16, 332     # the nearer one has category 2
BIG_CIRCLE, BIG_BOX = 27, 333         # rays start inside them; a probe sits on the box's corner
FAR_CIRCLE = 334                      # beyond a ray's maxFraction
SYNTHETIC_SLOTS = 335


def fixture_path(name):
    return os.path.join(GOLDEN, "scene_query", "%s.npz" % name)


def load_fixture(name):
    d = np.load(fixture_path(name))
    return {k: np.ascontiguousarray(d[k]) for k in d.files}


def empty_world(bodies, shapes, origins):
    """The six arrays s2amd_world_upload takes, around the three the queries read: no joints, four free contact slots"""
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    return {"bodies": bodies, "contacts": contacts, "joints": np.zeros(0, dtype=wire.joint_dtype), "shapes": shapes, "pairs": pairs,
            "origins": np.ascontiguousarray(origins, dtype=np.float32)}


def fixture_world(fx):
    return empty_world(fx["bodies"], fx["shapes"], fx["origins"])


def polygon_normals(shapes):
    """Edge normals of the polygons that have none yet: s2Normalize(s2CrossVS(edge, 1)) as s2MakePolygon computes them (src/geometry.c:22-60)"""
    for sh in shapes:
        n = int(sh["count"])
        if sh["type"] != wire.SHAPE_POLYGON or n < 3 or np.any(sh["normals"][:n] != 0):
            continue
        v = sh["vertices"][:n]
        edge = np.roll(v, -1, axis=0) - v
        normal = np.stack([edge[:, 1], -edge[:, 0]], axis=1).astype(f32)
        sh["normals"][:n] = (normal / np.sqrt((normal * normal).sum(axis=1, dtype=f32))[:, None]).astype(f32)


def synthetic_world():
    """shape_report_world.synthetic_world() with polygon normals, and SYNTHETIC_SLOTS slots holding the directed cases"""
    base = shape_report_world.synthetic_world()
    shapes = np.zeros(SYNTHETIC_SLOTS, dtype=wire.shape_dtype)
    shapes["type"], shapes["body"] = wire.SHAPE_FREE, -1
    shapes[:shape_report_world.SLOTS] = base["shapes"]
    bodies = list(base["bodies"])

    def still_body(x, y, angle=0.0):
        b = np.zeros(1, dtype=wire.body_dtype)[0]
        synthetic._dynamic_body(b, x, y, 1.0, 0.5, gravity_scale=0.0)  # at rest, weightless: it stays where it is
        b["rot"] = (np.sin(angle), np.cos(angle))
        bodies.append(b)
        return len(bodies) - 1

    def put(slot, body, shape_type, verts, radius, category=1, normals=None):
        sh = shapes[slot]
        assert sh["type"] == wire.SHAPE_FREE, slot
        sh["body"], sh["type"] = body, shape_type
        sh["categoryBits"], sh["maskBits"], sh["groupIndex"] = category, 0, 0
        sh["proxyKey"] = (slot << 4) | wire.BODY_DYNAMIC
        sh["count"], sh["radius"] = len(verts), radius
        sh["vertices"][:len(verts)] = verts
        if normals is not None:
            sh["normals"][:len(normals)] = normals

    tie = still_body(20.0, 20.0, 0.3)
    put(TIE_LOW, tie, wire.SHAPE_CIRCLE, [(0.25, 0.0)], 0.5)
    put(TIE_HIGH, tie, wire.SHAPE_CIRCLE, [(0.25, 0.0)], 0.5)
    put(MASKED_NEAR, still_body(20.0, 30.0), wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.5, category=2)
    put(MASKED_FAR, still_body(22.0, 30.0), wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.5, category=1)
    put(BIG_CIRCLE, still_body(30.0, 20.0), wire.SHAPE_CIRCLE, [(0.0, 0.0)], 1.0)
    put(BIG_BOX, still_body(30.0, 30.0), wire.SHAPE_POLYGON, [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)], 0.0,
        normals=[(0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0)])
    put(FAR_CIRCLE, still_body(40.0, 20.0), wire.SHAPE_CIRCLE, [(0.0, 0.0)], 0.5)
    polygon_normals(shapes)
    bodies = np.array(bodies, dtype=wire.body_dtype)
    origins = np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()
    oraclebind.refit_shapes(bodies, shapes, origins)
    shapes["enlarged"] = 0
    world = dict(base)
    world.update(bodies=bodies, shapes=shapes, origins=origins)
    return world


def special_cases():
    """(rays, probes, boxes) of the directed cases, and for the rays what each must answer: the shape slot, or -1"""
    rays = [
        ((17.0, 20.0), (23.0, 20.0), 1.0, ALL, TIE_LOW),          # two identical circles: the lower slot
        ((17.0, 30.0), (25.0, 30.0), 1.0, ALL, MASKED_NEAR),      # every category: the nearer circle
        ((17.0, 30.0), (25.0, 30.0), 1.0, 1, MASKED_FAR),         # the nearer one masked out
        ((17.0, 30.0), (25.0, 30.0), 1.0, 4, -1),                 # both masked out
        ((30.0, 20.0), (33.0, 20.0), 1.0, ALL, -1),               # starts inside a circle: no hit (src/geometry.c:432-438)
        ((30.0, 30.0), (33.0, 30.0), 1.0, ALL, -1),               # starts inside a polygon: no hit (:720)
        ((28.0, 20.0), (28.0, 20.0), 1.0, ALL, -1),               # zero length
        ((30.0, 20.5), (30.0, 20.5), 1.0, ALL, -1),               # zero length, inside
        ((33.0, 20.0), (37.0, 20.0), 1.0, ALL, -1),               # the nearest hit (40, 20) lies beyond maxFraction
        ((33.0, 20.0), (37.0, 20.0), 2.0, ALL, FAR_CIRCLE),       # ... and within twice the segment
        ((27.0, 30.0), (33.0, 30.0), 0.0, ALL, -1),               # maxFraction 0
        ((27.0, 30.0), (33.0, 30.0), 1.0, ALL, BIG_BOX),
        ((27.0, 30.5), (33.0, 30.5), 1.0, ALL, BIG_BOX),          # along the box's upper edge: enters through the left face's plane
        ((30.5, 27.0), (30.5, 33.0), 1.0, ALL, BIG_BOX),          # along its right edge
        ((27.0, 20.0), (33.0, 20.0), 1.0, ALL, BIG_CIRCLE),
    ]
    out = np.zeros(len(rays), dtype=wire.ray_dtype)
    for r, (p1, p2, max_fraction, mask, _) in zip(out, rays):
        r["p1"], r["p2"], r["maxFraction"], r["maskBits"] = p1, p2, max_fraction, mask
    probes = np.zeros(6, dtype=wire.point_probe_dtype)
    probes["maskBits"] = ALL
    probes["p"] = [(30.5, 30.5), (30.0, 30.0), (20.0, 30.0), (20.0, 30.0), (1000.0, 1000.0), (30.0, 21.0)]
    probes["maskBits"][3] = 1  # the circle at (20, 30) has category 2
    boxes = np.zeros(4, dtype=wire.box_query_dtype)
    boxes["maskBits"] = ALL
    boxes["box"] = [(1000.0, 1000.0, 1001.0, 1001.0), (19.0, 19.0, 31.0, 31.0), (-100.0, -100.0, 100.0, 100.0), (19.0, 29.0, 23.0, 31.0)]
    boxes["maskBits"][3] = 2
    return out, probes, boxes, [r[4] for r in rays]


def _world_point(world, slot, local):
    body = int(world["shapes"]["body"][slot])
    s, c = world["bodies"]["rot"][body]
    o = world["origins"][body]
    return np.array([c * local[0] - s * local[1] + o[0], s * local[0] + c * local[1] + o[1]], dtype=f32)


def _centre(world, slot):
    sh = world["shapes"][slot]
    n = {wire.SHAPE_CIRCLE: 1, wire.SHAPE_POLYGON: int(sh["count"])}.get(int(sh["type"]), 2)
    return _world_point(world, slot, sh["vertices"][:n].mean(axis=0))


def make_batch(world, counts, seed, special=None):
    """A fixed batch: rays from outside through shape centres, out of shape centres, along polygon edges, and random ones; probes at
    centres, on polygon vertices and at random; boxes around shapes, random ones, one over everything and one over nothing."""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = np.nonzero(shapes["type"] != wire.SHAPE_FREE)[0]
    fat = shapes["fatAABB"][live]
    lo, hi = fat[:, :2].min(axis=0), fat[:, 2:].max(axis=0)
    # (the zoo's and the pyramid's grounds are 100 m wide: aim where the shapes are)
    small = live[(shapes["fatAABB"][live][:, 2] - shapes["fatAABB"][live][:, 0]) < 20.0]
    slo, shi = shapes["fatAABB"][small][:, :2].min(axis=0) - 1.0, shapes["fatAABB"][small][:, 2:].max(axis=0) + 1.0
    polygons = small[shapes["type"][small] == wire.SHAPE_POLYGON]
    n_rays, n_probes, n_boxes = counts

    def anywhere():
        return (slo + (shi - slo) * rng.rand(2)).astype(f32)

    rays = np.zeros(n_rays, dtype=wire.ray_dtype)
    rays["maskBits"] = ALL
    rays["maxFraction"] = 1.0
    for i, r in enumerate(rays):
        kind = i % 8
        slot = int(small[rng.randint(len(small))])
        c = _centre(world, slot)
        if kind < 5:      # from somewhere through a shape's centre and on
            p1 = anywhere()
            r["p1"], r["p2"] = p1, (p1 + f32(1.5) * (c - p1)).astype(f32)
        elif kind == 5:   # out of a shape's centre
            r["p1"], r["p2"] = c, anywhere()
        elif kind == 6 and len(polygons):  # along a polygon's edge, a little longer than the edge
            slot = int(polygons[rng.randint(len(polygons))])
            sh = shapes[slot]
            k = rng.randint(int(sh["count"]))
            a, b = _world_point(world, slot, sh["vertices"][k]), _world_point(world, slot, sh["vertices"][(k + 1) % int(sh["count"])])
            r["p1"], r["p2"] = (a - f32(0.5) * (b - a)).astype(f32), (b + f32(0.5) * (b - a)).astype(f32)
        else:
            r["p1"], r["p2"] = anywhere(), anywhere()
        if i % 16 == 9:
            r["maxFraction"] = [0.5, 2.0, 0.25, 0.0][(i // 16) % 4]
        if i % 32 == 17:
            r["maskBits"] = [1, 2, 0xFFFF0000, 0][(i // 32) % 4]
    probes = np.zeros(n_probes, dtype=wire.point_probe_dtype)
    probes["maskBits"] = ALL
    for i, q in enumerate(probes):
        kind = i % 4
        slot = int(small[rng.randint(len(small))])
        if kind == 0:
            q["p"] = _centre(world, slot)
        elif kind == 1 and len(polygons):
            slot = int(polygons[rng.randint(len(polygons))])
            q["p"] = _world_point(world, slot, shapes[slot]["vertices"][rng.randint(int(shapes[slot]["count"]))])
        elif kind == 2:
            q["p"] = (_centre(world, slot) + (rng.rand(2) - 0.5) * 0.6).astype(f32)
        else:
            q["p"] = anywhere()
        if i % 16 == 11:
            q["maskBits"] = [1, 2, 0][(i // 16) % 3]
    boxes = np.zeros(n_boxes, dtype=wire.box_query_dtype)
    boxes["maskBits"] = ALL
    for i, q in enumerate(boxes):
        if i == 0:
            q["box"] = (lo[0] - 1, lo[1] - 1, hi[0] + 1, hi[1] + 1)      # everything
        elif i == 1:
            q["box"] = (hi[0] + 500, hi[1] + 500, hi[0] + 501, hi[1] + 501)  # nothing
        elif i % 3 == 0:
            c = _centre(world, int(small[rng.randint(len(small))]))
            q["box"] = (c[0], c[1], c[0], c[1])                           # a point
        else:
            a, size = anywhere(), (rng.rand(2) * 3.0).astype(f32)
            q["box"] = (a[0], a[1], a[0] + size[0], a[1] + size[1])
        if i % 8 == 5:
            q["maskBits"] = [1, 2, 0][(i // 8) % 3]
    if special is not None:
        s_rays, s_probes, s_boxes = special
        rays[:len(s_rays)], probes[:len(s_probes)], boxes[2:2 + len(s_boxes)] = s_rays, s_probes, s_boxes
    return rays, probes, boxes


def random_boxes(world, count, seed):
    """`count` random boxes over where the world's shapes are, sizes from a point to the whole (for the pin to s2World_QueryAABB)"""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = shapes["type"] != wire.SHAPE_FREE
    small = live & ((shapes["fatAABB"][:, 2] - shapes["fatAABB"][:, 0]) < 20.0)
    lo, hi = shapes["fatAABB"][small][:, :2].min(axis=0) - 1.0, shapes["fatAABB"][small][:, 2:].max(axis=0) + 1.0
    boxes = np.zeros(count, dtype=wire.box_query_dtype)
    boxes["maskBits"] = ALL
    for i, q in enumerate(boxes):
        a = (lo + (hi - lo) * rng.rand(2)).astype(f32)
        size = ((hi - lo) * rng.rand(2) ** 2).astype(f32) if i % 5 else np.zeros(2, dtype=f32)
        q["box"] = (a[0], a[1], a[0] + size[0], a[1] + size[1])
    return boxes


def reference_world(scene, p0, steps):
    """(RefWorld, world) of a reference scene after `steps` s2World_Steps; the caller closes the RefWorld"""
    from tests import refbind
    w = refbind.RefWorld(scene, "TGS_Soft", p0)
    for _ in range(steps):
        w.step()
    bodies, _, _ = w.pack()
    shapes, origins = w.pack_shapes()
    return w, empty_world(bodies, shapes, origins)


def expected(world, rays, probes, boxes):
    from tests import scene_query_ref as ref
    probe_offsets, probe_shapes = ref.point_probe(world, probes)
    box_offsets, box_shapes = ref.query_boxes(world, boxes)
    return {"hits": ref.ray_cast(world, rays), "probe_offsets": probe_offsets, "probe_shapes": probe_shapes, "box_offsets": box_offsets,
            "box_shapes": box_shapes}


def build_fixture(name):
    if name == "synthetic":
        world = synthetic_world()
        batch = make_batch(world, BATCH[name], 3, special_cases()[:3])
    else:
        ref_world, world = reference_world(*{"zoo": ("shapes_zoo", 0, 30), "pyramid30": ("pyramid", 30, 20)}[name])
        ref_world.close()
        batch = make_batch(world, BATCH[name], {"zoo": 1, "pyramid30": 2}[name])
    fx = {"bodies": world["bodies"], "shapes": world["shapes"], "origins": world["origins"]}
    fx.update(zip(QUERY_KEYS, batch))
    fx.update(expected(world, *batch))
    return fx


if __name__ == "__main__":
    for fixture in FIXTURES:
        built = build_fixture(fixture)
        np.savez_compressed(fixture_path(fixture), **built)
        hit = int((built["hits"]["shape"] >= 0).sum())
        print("%s: %d shape slots, %d of %d rays hit, %d probe hits, %d box hits, %d bytes" % (
            fixture, len(built["shapes"]), hit, len(built["rays"]), len(built["probe_shapes"]), len(built["box_shapes"]),
            os.path.getsize(fixture_path(fixture))))
