"""Cast batches of the shape-cast tests (tests/test_shape_cast_host.py, tests/test_gpu_shape_cast.py) and the generator of their
fixtures tests/golden/shape_cast/*.npz (python -m tests.shape_cast_world, with oracle/_ref/libs2ref.so built).  Test infrastructure only.

The worlds are the three of tests/scene_query_world.py, read from its fixtures (zoo: 54 shapes of all four types in one tile; pyramid30:
466 polygons resting on each other in two tiles; synthetic: 335 slots with rotated bodies, free slots and the directed cases).  A
fixture here holds data only: one fixed batch of CASTS casts and what the statement (tests/shape_cast_ref.py) answers, the first-hit
records and the all-hits lists."""
import os

import numpy as np

from solver2d_amd import wire
from tests import proximity_world as pw, scene_query_world as sq

f32 = np.float32
ALL = 0xFFFFFFFF
FIXTURES = sq.FIXTURES
CASTS = 256
RESULT_KEYS = ("first", "all_offsets", "all_hits")
SEEDS = {"zoo": 31, "pyramid30": 32, "synthetic": 33}
POINT = [(0.0, 0.0)]
BOX = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
# the fraction at which a point cast by (4, 0) from 1.5 away stops: one advance, (1.5 - target) / 4 (see special_cases)
ONE_ADVANCE = f32(f32(f32(1.5) - f32(0.005)) / f32(4.0))


def fixture_path(name):
    return os.path.join(sq.GOLDEN, "shape_cast", "%s.npz" % name)


def load_fixture(name):
    """The shape-cast fixture with the world of the scene-query fixture of the same name beside it (bodies, shapes, origins)"""
    d = np.load(fixture_path(name))
    fx = {k: np.ascontiguousarray(d[k]) for k in d.files}
    world = sq.load_fixture(name)
    fx.update({k: world[k] for k in ("bodies", "shapes", "origins")})
    return fx


def make_cast(vertices, radius, position, angle, translation, max_fraction=1.0, mask=ALL):
    c = np.zeros(1, dtype=wire.shape_cast_dtype)[0]
    c["vertices"][:len(vertices)] = vertices
    c["count"], c["radius"], c["position"] = len(vertices), radius, position
    c["rot"] = (np.sin(angle), np.cos(angle))
    c["translation"], c["maxFraction"], c["maskBits"] = translation, max_fraction, mask
    return c


def special_cases():
    """The directed casts of the synthetic world and the shape each must name first (-1: none, None: not stated), see
    sq.synthetic_world(): two identical circles in both tiles, a masked-out shape that would otherwise be hit first, a sweep that ends
    one ulp short of its hit, free slots under the path, starts inside shapes, a zero translation"""
    short = np.nextafter(ONE_ADVANCE, f32(0.0))
    cases = [
        (make_cast(POINT, 0.1, (17.0, 20.0), 0.0, (6.0, 0.0)), sq.TIE_LOW),                 # both at the same fraction: the lower slot
        (make_cast(POINT, 0.0, (17.0, 30.0), 0.0, (8.0, 0.0)), sq.MASKED_NEAR),             # every category: the nearer circle
        (make_cast(POINT, 0.0, (17.0, 30.0), 0.0, (8.0, 0.0), 1.0, 1), sq.MASKED_FAR),      # the nearer one masked out
        (make_cast(POINT, 0.0, (17.0, 30.0), 0.0, (8.0, 0.0), 1.0, 4), -1),                 # both masked out
        (make_cast(POINT, 0.0, (38.0, 20.0), 0.0, (4.0, 0.0), ONE_ADVANCE), sq.FAR_CIRCLE),  # the circle at (40, 20), radius 0.5: 1.5 away
        (make_cast(POINT, 0.0, (38.0, 20.0), 0.0, (4.0, 0.0), short), -1),                  # ... and one ulp less ends short of it
        (make_cast(POINT, 0.0, (-1.0, 0.0), 0.0, (2.0, 0.0)), None),                        # over the zeroed boxes of the free slots
        (make_cast(POINT, 0.25, (0.0, -1.0), 0.0, (0.0, 2.0)), None),
        (make_cast(BOX, 0.0, (30.25, 30.0), 0.0, (3.0, 0.0)), sq.BIG_BOX),  # starts inside the box
        (make_cast(POINT, 0.1, (30.0, 20.5), 0.0, (0.0, 0.0)), sq.BIG_CIRCLE),              # no translation, inside: a hit at 0
        (make_cast(POINT, 0.1, (30.0, 21.15), 0.0, (0.0, 0.0)), -1),                        # no translation, 0.05 off: a miss
        (make_cast(POINT, 0.1, (30.0, 21.15), 0.0, (0.0, 3.0)), -1),                        # moving away
    ]
    return np.array([c[0] for c in cases], dtype=wire.shape_cast_dtype), [c[1] for c in cases]


def _first_box_met(fat, verts, grow, start, direction, reach):
    """How far along `direction` from `start` (in steps of 0.02, up to `reach`) the proxy's own box -- its vertices' bounds grown by
    `grow` -- first overlaps one of the fat boxes; `reach` if it never does.  Box arithmetic only: no distance function is asked."""
    lo, hi = verts.min(axis=0) - grow, verts.max(axis=0) + grow
    along = np.arange(0.0, reach, 0.02)
    at = start[None, :] + along[:, None] * direction[None, :]
    apart = ((at[:, None, 0] + lo[0] > fat[None, :, 2]) | (at[:, None, 1] + lo[1] > fat[None, :, 3]) |
             (fat[None, :, 0] > at[:, None, 0] + hi[0]) | (fat[None, :, 1] > at[:, None, 1] + hi[1]))
    met = np.nonzero(~apart.all(axis=1))[0]
    return float(along[met[0]]) if len(met) else float(reach)


def make_batch(world, count, seed, special=None):
    """A fixed batch.  Cast i has 1 + i % 8 proxy vertices, a radius when (i // 8) is odd, and an angle unless i % 3 == 0.  All but the
    casts of kind 5 start on a ring outside the bounds of the world's (small) shapes, on a line towards a point near a shape's centre;
    `met` is how far along that line the proxy's box first overlaps a fat box.  By kind (i // 8 + i) % 8:
      0-3  the sweep ends half a metre beyond `met`;  4  a metre beyond it (through several shapes)
      5    starts at a shape's centre and sweeps anywhere
      6    starts at `met` -- where the box has just come to overlap a fat box, the shape inside it still a margin away -- and sweeps
           back outwards, or forwards with maxFraction 0
      7    starts on the ring and sweeps outwards, or starts and ends far from everything."""
    rng = np.random.RandomState(seed)
    shapes = world["shapes"]
    live = np.nonzero(shapes["type"] != wire.SHAPE_FREE)[0]
    fat = shapes["fatAABB"][live].astype(np.float64)
    small = live[(shapes["fatAABB"][live][:, 2] - shapes["fatAABB"][live][:, 0]) < 20.0]
    slo, shi = shapes["fatAABB"][small][:, :2].min(axis=0), shapes["fatAABB"][small][:, 2:].max(axis=0)
    # (aimed at shapes whose fat box overlaps at most six others: the lists stay short where a world piles shapes on one spot)
    sf = shapes["fatAABB"][small].astype(np.float64)
    near = ~((sf[:, None, 0] > fat[None, :, 2]) | (sf[:, None, 1] > fat[None, :, 3]) | (fat[None, :, 0] > sf[:, None, 2]) | (fat[None, :, 1] > sf[:, None, 3]))
    aimed = small[near.sum(axis=1) <= 7]
    middle, ring = 0.5 * (slo + shi), 0.5 * float(np.hypot(*(shi - slo))) + 2.0
    casts = np.zeros(count, dtype=wire.shape_cast_dtype)
    for i in range(count):
        n = 1 + i % 8
        radius = 0.0 if (i // 8) % 2 == 0 else 0.05 + 0.25 * rng.rand()
        angle = 0.0 if i % 3 == 0 else rng.rand() * 6.28
        kind = (i // 8 + i) % 8
        slot = int(aimed[rng.randint(len(aimed))])
        aim = sq._centre(world, slot) + (rng.rand(2) * 0.4 - 0.2)
        at = rng.rand() * 6.28
        start = middle + ring * np.array([np.cos(at), np.sin(at)])
        verts = np.array(pw.proxy_vertices(rng, n), dtype=np.float64)
        turned = verts @ np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
        reach = float(np.hypot(*(aim - start)))
        direction = (aim - start) / reach
        met = _first_box_met(fat, turned, radius + 0.02, start, direction, reach)
        max_fraction = 1.0
        if kind < 5:
            translation = direction * (met + (0.5 if kind < 4 else 1.0))
        elif kind == 5:
            start, translation = sq._centre(world, slot), (rng.rand(2) * 2.0 - 1.0)
        elif kind == 6:
            start = start + met * direction
            translation, max_fraction = (-2.0 * direction, 1.0) if i % 16 < 8 else (direction, 0.0)
        elif i % 16 < 8:
            translation = 0.5 * (start - middle)
        else:
            start, translation = shi + 400.0 + 50.0 * rng.rand(2), rng.rand(2) * 4.0 - 2.0
        if i % 16 == 9:
            max_fraction = [0.5, 2.0, 0.75, 4.0][(i // 16) % 4]
        casts[i] = make_cast(verts, radius, start.astype(f32), angle, translation.astype(f32), max_fraction)
        if i % 32 == 17:
            casts[i]["maskBits"] = [1, 2, 0xFFFF0000, 0][(i // 32) % 4]
    if special is not None:
        casts[:len(special)] = special
    return casts


def expected(world, casts):
    from tests import shape_cast_ref as ref
    return dict(zip(RESULT_KEYS, ref.both(world, casts)))


def build_fixture(name):
    world = sq.fixture_world(sq.load_fixture(name))
    casts = make_batch(world, CASTS, SEEDS[name], special_cases()[0] if name == "synthetic" else None)
    fx = {"casts": casts}
    fx.update(expected(world, casts))
    return fx


def candidate_counts(world, casts):
    from tests import shape_cast_ref as ref
    return np.array([len(ref.candidates(world, c)) for c in casts])


def least_sampled_distance(world, casts, first, limit=64, most=12, samples=64):
    """The statement against geometry, independent of its own loop: for the first `limit` casts and up to `most` candidates each, the
    reference's distance at `samples` evenly spaced fractions j / samples of the way to where the statement says the sweep against that
    candidate ends -- its hit fraction, or maxFraction on a miss.  (A sweep that starts within reach has gone no way: nothing to
    sample.)  -> the least distance seen, and how many were taken"""
    from tests import proximity_ref as pref, shape_cast_ref as ref
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    least, taken = np.inf, 0
    for c in casts[:limit]:
        proxy_a = pref.make_proxy(c["vertices"], int(c["count"]), c["radius"])
        for slot in ref.candidates(world, c)[:most]:
            sh = shapes[slot]
            body = int(sh["body"])
            proxy_b, xf_b = pref.shape_proxy(sh), pref.transform(origins[body], bodies["rot"][body])
            r = ref.cast_against(c, proxy_a, proxy_b, xf_b)
            end = f32(c["maxFraction"]) if r is None else r[0]
            if end == 0:
                continue
            for j in range(samples):
                d = ref.distance_at(c, proxy_a, f32(end * f32(j) / f32(samples)), proxy_b, xf_b)
                least, taken = min(least, float(d.distance)), taken + 1
    return least, taken


if __name__ == "__main__":
    os.makedirs(os.path.dirname(fixture_path("zoo")), exist_ok=True)
    for fixture in FIXTURES:
        built = build_fixture(fixture)
        np.savez_compressed(fixture_path(fixture), **built)
        first, won = built["first"], built["first"]["shape"] >= 0
        w = sq.fixture_world(sq.load_fixture(fixture))
        cands = candidate_counts(w, built["casts"])
        sampled, taken = least_sampled_distance(w, built["casts"], first)
        print("%s: %d casts, %d name a shape (%d at fraction 0, %d beyond; %d with no advance, %d with two or more, at most %d), "
              "%d with candidates and no hit, %d without a candidate, %d entries, least sampled distance %.6f over %d samples, %d bytes" % (
                  fixture, len(first), int(won.sum()), int((won & (first["fraction"] == 0)).sum()), int((won & (first["fraction"] > 0)).sum()),
                  int((won & (first["iterations"] == 0)).sum()), int((won & (first["iterations"] >= 2)).sum()),
                  int(built["all_hits"]["iterations"].max()), int(((cands > 0) & ~won).sum()), int((cands == 0).sum()), len(built["all_hits"]),
                  sampled, taken, os.path.getsize(fixture_path(fixture))))
