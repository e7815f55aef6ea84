"""Mover batches of the move-and-slide tests (tests/test_mover_host.py, tests/test_gpu_mover.py) and the generator of their fixtures
tests/golden/mover/*.npz (python -m tests.mover_world, with oracle/_ref/libs2ref.so built).  Test infrastructure only.

zoo, pyramid30, synthetic: the worlds of tests/scene_query_world.py, read from its fixtures.  A fixture holds data only: one fixed batch
of MOVERS movers and what the statement (tests/mover_ref.py) answers, the results and the planes, and `first`, the indices of the movers
whose plane 0 must be the hit s2amd_world_cast_shape reports for the same cast.  The batch is the shape-cast batch of the same world
(tests/shape_cast_world.py) with translation * maxFraction as the displacement and four iterations, its last DIRECTED movers replaced by
directed ones (directed_movers()).

walk: three small worlds of static boxes -- a floor of 32 unit boxes laid edge to edge, the floor with a wall, the floor with a ramp --
walked by a box and a capsule for FRAMES frames, each frame starting where the last ended; the fixture keeps every frame's answer."""
import os

import numpy as np

from solver2d_amd import wire
from tests import scene_query_world as sq, shape_cast_world as cw

f32 = np.float32
ALL = 0xFFFFFFFF
FIXTURES = sq.FIXTURES
MOVERS = 256
DIRECTED = 36
ITERATIONS = 4
SEEDS = {"zoo": 51, "pyramid30": 52, "synthetic": 53}
RESULT_KEYS = ("results", "planes")
POINT = cw.POINT
BOX = cw.BOX
WALKER_BOX = [(-0.25, -0.5), (0.25, -0.5), (0.25, 0.5), (-0.25, 0.5)]
WALKER_CAPSULE = [(0.0, -0.25), (0.0, 0.25)]
FRAMES = 300
STEP = (0.05, -0.0027)
START = (0.0, 0.52)
WALKS = ("floor", "wall", "ramp")
WALKERS = ("box", "capsule")
WALL_FACE = 9.5
RAMP_ANGLE = np.deg2rad(25.0)
RAMP_CORNER = (5.0, -0.05)  # the upper left corner of the ramp: where its top face leaves the floor


def fixture_path(name):
    return os.path.join(sq.GOLDEN, "mover", "%s.npz" % name)


def load_fixture(name):
    """The mover fixture with the world of the scene-query fixture of the same name beside it (bodies, shapes, origins)"""
    d = np.load(fixture_path(name))
    fx = {k: np.ascontiguousarray(d[k]) for k in d.files}
    world = sq.load_fixture(name)
    fx.update({k: world[k] for k in ("bodies", "shapes", "origins")})
    return fx


def make_mover(vertices, radius, position, angle, translation, iterations=ITERATIONS, mask=ALL, ignore=-1, flags=0):
    m = np.zeros(1, dtype=wire.mover_dtype)[0]
    m["vertices"][:len(vertices)] = vertices
    m["count"], m["radius"], m["position"] = len(vertices), radius, position
    m["rot"] = (np.sin(angle), np.cos(angle))
    m["translation"], m["maxIterations"], m["maskBits"], m["ignoreBody"], m["flags"] = translation, iterations, mask, ignore, flags
    return m


def from_casts(casts, iterations=ITERATIONS):
    """The movers of a cast batch: the same proxy, start and mask; translation * maxFraction as the displacement"""
    movers = np.zeros(len(casts), dtype=wire.mover_dtype)
    for key in ("vertices", "count", "radius", "position", "rot", "maskBits"):
        movers[key] = casts[key]
    movers["translation"] = (casts["translation"] * casts["maxFraction"][:, None]).astype(f32)
    movers["maxIterations"], movers["ignoreBody"] = iterations, -1
    return movers


def to_casts(movers):
    """The first cast of every mover (step 1 of the statement at b = 0)"""
    casts = np.zeros(len(movers), dtype=wire.shape_cast_dtype)
    for key in ("vertices", "count", "radius", "position", "rot", "translation", "maskBits"):
        casts[key] = movers[key]
    casts["maxFraction"] = 1.0
    return casts


def _pool(world, count, seed):
    """Candidates for the directed movers, eight iterations each.  By i % 4: a circle, a capsule or a box aimed from outside at a shape
    and wanting to go half as far again (it has to get round the shape, or into the corner behind it); the same proxies dropped
    straight down or pushed straight sideways at a shape's centre line (head-on where the shape's face or a circle lies square to it)"""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = np.nonzero(shapes["type"] != wire.SHAPE_FREE)[0]
    small = live[(shapes["fatAABB"][live][:, 2] - shapes["fatAABB"][live][:, 0]) < 20.0]
    proxies = [(POINT, 0.25), (WALKER_CAPSULE, 0.25), (WALKER_BOX, 0.0), (BOX, 0.0)]
    out = np.zeros(count, dtype=wire.mover_dtype)
    for i in range(count):
        verts, radius = proxies[rng.randint(len(proxies))]
        slot = int(small[rng.randint(len(small))])
        centre = sq._centre(world, slot).astype(f32)
        kind = i % 4
        if kind < 2:
            at = rng.rand() * 6.28
            away = 2.0 + 3.0 * rng.rand()
            start = (centre + f32(away) * np.array([np.cos(at), np.sin(at)], dtype=f32)).astype(f32)
            translation = ((centre - start) * f32(1.5)).astype(f32)
        elif kind == 2:
            start = np.array([centre[0], centre[1] + f32(3.0)], dtype=f32)
            translation = np.array([0.0, -4.0], dtype=f32)
        else:
            side = f32(-1.0 if rng.rand() < 0.5 else 1.0)
            start = np.array([centre[0] + side * f32(3.0), centre[1]], dtype=f32)
            translation = np.array([-side * f32(4.0), 0.0], dtype=f32)
        out[i] = make_mover(verts, radius, start, 0.0, translation, wire.MOVER_MAX_ITERATIONS)
    return out


def directed_movers(world, seed):
    """DIRECTED movers chosen from a seeded pool by what the statement answers for them (so the compiled reference is needed), in this
    order: 8 x one mover of three or more planes that takes four casts or more with maxIterations 1 .. 8; 4 other movers that meet
    something and do not end there, cut to one iteration (OUT_OF_ITERATIONS); 5 more of three or more planes; 5 BLOCKED (head-on into
    a face, or stopped dead in a corner); 4 CORNERED; 4 started inside a shape (OVERLAPPED); a mover with ignoreBody set to the body it
    would have stood on first, and to an unrelated body; one under STATIC_ONLY whose first plane was on a moving body; one whose mask
    leaves out the category of its first plane; 2 far from everything (REACHED in one cast without a plane)."""
    from tests import mover_ref as ref
    pool = _pool(world, 640, seed)
    results, planes = ref.move_shapes(world, pool)
    status, count, casts_made = results["status"], results["planeCount"], results["iterations"]
    used = set()

    def take(mask, n, what):
        idx = [int(i) for i in np.nonzero(mask)[0] if int(i) not in used][:n]
        assert len(idx) == n, "the pool holds %d of %d movers for: %s" % (len(idx), n, what)
        used.update(idx)
        return idx

    out = []
    series = take((count >= 3) & (casts_made >= 4), 1, "three planes in four casts")[0]
    for iterations in range(1, wire.MOVER_MAX_ITERATIONS + 1):
        m = pool[series].copy()
        m["maxIterations"] = iterations
        out.append(m)
    for i in take((count >= 1) & (casts_made >= 2), 4, "more than one cast"):
        m = pool[i].copy()
        m["maxIterations"] = 1
        out.append(m)
    out += [pool[i].copy() for i in take(count >= 3, 5, "three or more planes")]
    out += [pool[i].copy() for i in take(status == wire.MOVER_BLOCKED, 5, "BLOCKED")]
    out += [pool[i].copy() for i in take(status == wire.MOVER_CORNERED, 4, "CORNERED")]
    rng = np.random.RandomState(seed + 1000)
    shapes = world["shapes"]
    solid = np.nonzero((shapes["type"] == wire.SHAPE_POLYGON) | (shapes["type"] == wire.SHAPE_CIRCLE))[0]
    for k in range(4):
        slot = int(solid[rng.randint(len(solid))])
        out.append(make_mover(POINT, 0.05, sq._centre(world, slot).astype(f32), 0.0, (rng.rand(2) * 2.0 - 1.0).astype(f32), 2 + k))
    stood = take((count >= 2) & (planes["fraction"][:, 0] > 0), 1, "a mover that slides")[0]
    on = int(planes["body"][stood, 0])
    other = int(np.setdiff1d(world["shapes"]["body"][world["shapes"]["type"] != wire.SHAPE_FREE], planes["body"][stood, :count[stood]])[0])
    for ignore in (on, other):
        m = pool[stood].copy()
        m["ignoreBody"] = ignore
        out.append(m)
    moving = world["bodies"]["type"][np.maximum(planes["body"][:, 0], 0)] != wire.BODY_STATIC
    m = pool[take((count >= 1) & moving, 1, "a first plane on a moving body")[0]].copy()
    m["flags"] = wire.MOVER_STATIC_ONLY
    out.append(m)
    i = take(count >= 1, 1, "a first plane")[0]
    m = pool[i].copy()
    m["maskBits"] = ALL & ~int(shapes["categoryBits"][planes["shape"][i, 0]])
    out.append(m)
    far = shapes["fatAABB"][solid][:, 2:].max(axis=0) + 400.0
    out += [make_mover(BOX, 0.1, (far + 50.0 * k).astype(f32), 0.5, (rng.rand(2) * 4.0 - 2.0).astype(f32), 1 + 7 * k) for k in range(2)]
    assert len(out) == DIRECTED
    return np.array(out, dtype=wire.mover_dtype)


def make_batch(world, name):
    casts = cw.make_batch(world, cw.CASTS, cw.SEEDS[name], cw.special_cases()[0] if name == "synthetic" else None)
    movers = from_casts(casts)
    movers[MOVERS - DIRECTED:] = directed_movers(world, SEEDS[name])
    return movers


def expected(world, movers):
    from tests import mover_ref as ref
    return dict(zip(RESULT_KEYS, ref.move_shapes(world, movers)))


def first_hits(world, movers, planes):
    """The movers whose plane 0 is the first hit of their first cast, by the shape casts' statement"""
    from tests import shape_cast_ref as cref
    hits = cref.cast_shape(world, to_casts(movers))
    same = [i for i in range(len(movers)) if hits["shape"][i] >= 0 and hits["shape"][i] == planes["shape"][i, 0] and
            all(hits[k][i].tobytes() == planes[k][i, 0].tobytes() for k in ("body", "fraction", "distance", "point", "normal"))]
    return np.array(same, dtype=np.int32)


def build_fixture(name):
    world = sq.fixture_world(sq.load_fixture(name))
    movers = make_batch(world, name)
    fx = {"movers": movers}
    fx.update(expected(world, movers))
    fx["first"] = first_hits(world, movers, fx["planes"])
    return fx


# ---- the walk ----
def _static_box(bodies, shapes, k, hx, hy, x, y, angle=0.0):
    """A static body at (x, y) turned by `angle` with one box of half extents (hx, hy) around its origin; the fat box is the bounds of
    the turned vertices grown by 0.1"""
    from solver2d_amd import synthetic
    synthetic._static_body(bodies[k], x, y)
    bodies[k]["rot"] = (np.sin(angle), np.cos(angle))
    synthetic._box_shape(shapes[k], k, wire.BODY_STATIC, hx, hy, x, y, k)
    s, c = bodies[k]["rot"]
    v = shapes[k]["vertices"][:4]
    wx, wy = c * v[:, 0] - s * v[:, 1] + f32(x), s * v[:, 0] + c * v[:, 1] + f32(y)
    shapes[k]["aabb"] = (wx.min() - f32(0.02), wy.min() - f32(0.02), wx.max() + f32(0.02), wy.max() + f32(0.02))
    shapes[k]["fatAABB"] = (wx.min() - f32(0.1), wy.min() - f32(0.1), wx.max() + f32(0.1), wy.max() + f32(0.1))


def walk_world(kind):
    """32 unit boxes with their tops at y = 0 from x = -1 to 31; "wall": a 1 x 4 box standing on them with its face at x = 9.5;
    "ramp": a 6 x 1 box turned by 25 degrees whose top face leaves the floor at x = 5"""
    n = 32 + (kind != "floor")
    bodies, shapes = np.zeros(n, dtype=wire.body_dtype), np.zeros(n, dtype=wire.shape_dtype)
    for k in range(32):
        _static_box(bodies, shapes, k, 0.5, 0.5, k - 0.5, -0.5)
    if kind == "wall":
        _static_box(bodies, shapes, 32, 0.5, 2.0, WALL_FACE + 0.5, 2.0)
    elif kind == "ramp":
        s, c = np.sin(RAMP_ANGLE), np.cos(RAMP_ANGLE)
        # the box's corner (-3, 0.5) lies at RAMP_CORNER
        _static_box(bodies, shapes, 32, 3.0, 0.5, RAMP_CORNER[0] + 3.0 * c + 0.5 * s, RAMP_CORNER[1] + 3.0 * s - 0.5 * c, RAMP_ANGLE)
    return sq.empty_world(bodies, shapes, bodies["position"].copy())


def walker(which, position):
    verts, radius = (WALKER_BOX, 0.0) if which == "box" else (WALKER_CAPSULE, 0.25)
    return make_mover(verts, radius, position, 0.0, STEP)


def walk(world, which, move, frames=FRAMES):
    """`frames` calls of move(movers[1]) -> (results[1], planes[1, 8]), each from where the last one ended"""
    results = np.zeros(frames, dtype=wire.mover_result_dtype)
    planes = np.zeros((frames, wire.MOVER_MAX_ITERATIONS), dtype=wire.mover_plane_dtype)
    position = START
    for f in range(frames):
        r, p = move(np.array([walker(which, position)], dtype=wire.mover_dtype))
        results[f], planes[f] = r[0], p[0]
        position = r[0]["position"]
    return results, planes


def statement_walk(kind, which, graze=None, frames=FRAMES):
    from tests import mover_ref as ref
    world = walk_world(kind)
    return walk(world, which, lambda m: ref.move_shapes(world, m, ref.GRAZE if graze is None else f32(graze)), frames)


def build_walk_fixture():
    fx = {}
    for kind in WALKS:
        for which in WALKERS:
            fx["%s_%s_results" % (kind, which)], fx["%s_%s_planes" % (kind, which)] = statement_walk(kind, which)
    return fx


def load_walk_fixture():
    d = np.load(fixture_path("walk"))
    return {k: np.ascontiguousarray(d[k]) for k in d.files}


if __name__ == "__main__":
    os.makedirs(os.path.dirname(fixture_path("zoo")), exist_ok=True)
    built = build_walk_fixture()
    np.savez_compressed(fixture_path("walk"), **built)
    for kind in WALKS:
        for which in WALKERS:
            res = built["%s_%s_results" % (kind, which)]
            print("walk %s %s: ends at (%.4f, %.4f), least y %.5f (after frame 1 %.5f), greatest y %.4f, statuses %s" % (
                kind, which, res["position"][-1][0], res["position"][-1][1], res["position"][:, 1].min(), res["position"][0][1],
                res["position"][:, 1].max(), np.bincount(res["status"], minlength=5).tolist()))
    print("walk: %d bytes" % os.path.getsize(fixture_path("walk")))
    for fixture in FIXTURES:
        built = build_fixture(fixture)
        np.savez_compressed(fixture_path(fixture), **built)
        res, pl = built["results"], built["planes"]
        print("%s: %d movers, statuses %s, %d with a plane, %d with three or more, %d whose second plane follows a slide, %d first hits, "
              "iterations %s, %d bytes" % (
                  fixture, len(res), np.bincount(res["status"], minlength=5).tolist(), int((res["planeCount"] >= 1).sum()),
                  int((res["planeCount"] >= 3).sum()), int(((res["planeCount"] >= 2) & (pl["fraction"][:, 1] > 0)).sum()), len(built["first"]),
                  np.bincount(res["iterations"], minlength=9).tolist(), os.path.getsize(fixture_path(fixture))))
