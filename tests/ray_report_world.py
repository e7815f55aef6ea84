"""The scenes of the ray-report tests (tests/test_ray_report_host.py, tests/test_gpu_ray_report.py), the loader and the generator of
their fixtures tests/golden/ray_report/*.npz (python -m tests.ray_report_world, with oracle/liboracle.so and oracle/_ref/libs2ref.so
built).  Test infrastructure only.

The three small worlds of tests/sensor_report_world.py (ball, base-3 pyramid, six-link chain), each run for STEPS steps of the oracle
chain (tests/world_chain.py) under TGS_Soft, with per world: a fixed fan, a fan of 8 mounted on a moving body (the ball, the flying
brick, the last link) that starts outside the body's own shape and points through it, one SKIP_STATIC ray aimed through a static shape
at a dynamic one, one DISABLED ray and one ray that misses everything.  A fixture holds the world, the rays and what the statement
(tests/ray_report_ref.py) answers on the chain in pool order: the hit shape per ray at the upload and per step, and the events --
settings and discrete results only.  The hit shapes are recorded under a clearance condition (robust_hits): they are the same with
every ray displaced 1 mm to either side along its own normal and with maxFraction scaled by 1 +- 1e-3, so a chain swept in another
constraint order, whose poses differ in their last bits, records the same shapes."""
import os

import numpy as np

from solver2d_amd import wire
from tests import sensor_report_world as sw

f32 = np.float32
ALL = 0xFFFFFFFF
STEPS = sw.STEPS
SCENES = sw.SCENES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_report")
WORLD_KEYS = sw.WORLD_KEYS
CLEARANCE = f32(1e-3)
COVERAGE = ("miss to hit", "hit to miss", "shape to shape", "fixed hits", "mounted hits", "mounted differ", "skip-static differ", "quiet steps")
params = sw.params


def make_ray(p1, p2, max_fraction=1.0, body=-1, flags=0, mask=ALL):
    q = np.zeros(1, dtype=wire.ray_sensor_dtype)[0]
    q["p1"], q["p2"], q["maxFraction"], q["maskBits"], q["body"], q["flags"] = p1, p2, max_fraction, mask, body, flags
    return q


def fan(origin, targets, **kw):
    return [make_ray(origin, t, **kw) for t in targets]


def ball_rays():
    rays = fan((-2.0, 4.4), [(2.0, 5.4), (2.0, 4.9), (2.0, 4.4), (2.0, 3.9), (2.0, 3.4)])              # fixed, across the ball's path
    rays.append(make_ray((-2.0, 3.5), (2.0, 3.5)))                                                     # through the ball's path onto the marker
    rays += fan((0.0, 0.6), [(0.1 * (j - 3.5), -3.0) for j in range(8)], body=1)                       # on the ball, down through it
    rays.append(make_ray((2.0, 3.5), (-2.0, 3.5), flags=wire.RAY_SENSOR_SKIP_STATIC))                  # through the marker at the ball
    rays.append(make_ray((-2.0, 3.5), (2.0, 3.5), flags=wire.RAY_SENSOR_DISABLED))
    rays.append(make_ray((10.0, 10.0), (11.0, 11.0)))                                                  # misses everything
    return rays


def pyramid_rays(world):
    flyer = len(world["bodies"]) - 2
    rays = [make_ray((-2.5, 3.0), (-2.5, 1.0)), make_ray((-1.9, 3.0), (-1.9, -0.5)),                   # fixed, across the flyer's path
            make_ray((0.1, 4.0), (0.1, 0.0)), make_ray((0.9, 4.0), (0.7, 0.0))]                        # ... and onto the pyramid
    rays += fan((-0.45, 0.0), [(1.45, 0.05 * (j - 3.5)) for j in range(8)], body=flyer)                 # on the flyer, ahead through it
    rays.append(make_ray((3.0, 2.6), (-1.0, 2.6), flags=wire.RAY_SENSOR_SKIP_STATIC))                  # through the post at the top brick
    rays.append(make_ray((3.0, 2.6), (-1.0, 2.6), flags=wire.RAY_SENSOR_DISABLED))
    rays.append(make_ray((-3.0, 8.0), (3.0, 9.0)))
    return rays


def chain_rays():
    links = 6
    rays = [make_ray((3.0, 6.0), (3.0, 0.0)), make_ray((1.0, 4.0), (1.0, 0.5)), make_ray((2.0, 5.6), (2.0, 3.0))]  # fixed, across the swing
    rays += fan((1.0, 0.0), [(-1.6, 0.012 * (j - 3.5)) for j in range(8)], body=links)                 # on the last link, back through it
    rays.append(make_ray((0.0, 6.0), (0.0, 0.0), flags=wire.RAY_SENSOR_SKIP_STATIC))                   # through the anchor at the hanging chain
    rays.append(make_ray((0.0, 6.0), (0.0, 0.0), flags=wire.RAY_SENSOR_DISABLED))
    rays.append(make_ray((-3.0, 8.0), (3.0, 9.0)))
    return rays


def scene(name):
    """-> (world, rays)"""
    world, _sensors = sw.BUILDERS[name]()
    rays = {"ball": ball_rays, "pyramid": lambda: pyramid_rays(world), "chain": chain_rays}[name]()
    return world, np.array(rays, dtype=wire.ray_sensor_dtype)


def displaced(rays, delta):
    """Every ray moved `delta` along its own normal (the left normal of p2 - p1, in the frame the ray is given in)"""
    out = rays.copy()
    d = (rays["p2"] - rays["p1"]).astype(np.float64)
    length = np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-12)
    normal = np.stack([-d[:, 1] / length, d[:, 0] / length], axis=1)
    out["p1"] = (rays["p1"] + delta * normal).astype(np.float32)
    out["p2"] = (rays["p2"] + delta * normal).astype(np.float32)
    return out


def scaled(rays, factor):
    out = rays.copy()
    out["maxFraction"] = (rays["maxFraction"].astype(np.float64) * factor).astype(np.float32)
    return out


def variations(rays):
    c = float(CLEARANCE)
    return [displaced(rays, c), displaced(rays, -c), scaled(rays, 1.0 + c), scaled(rays, 1.0 - c)]


def robust_hits(world, rays, exclusions=True):
    """The statement's hit shapes, asserted to be those of the four variations as well"""
    from tests import ray_report_ref as ref
    hits = ref.hits(world, rays, exclusions)
    for k, other in enumerate(variations(rays)):
        got = ref.hits(world, other, exclusions)
        assert got == hits, "variation %d: rays %s within %g of a change of their hit shape: move the scene" % (
            k, [i for i in range(len(rays)) if got[i] != hits[i]], CLEARANCE)
    return hits


def run_statement(world, rays, steps=STEPS, robust=True):
    """The chain in pool order -> fixture entries: before, and per step k hits_k, events_k, plain_k (the hit shapes without the exclusions)"""
    from tests import ray_report_ref as ref, world_chain
    hits_of = robust_hits if robust else ref.hits
    w = world_chain.copy_world(world)
    before = hits_of(w, rays)
    out = {"before": np.array(before, dtype=np.int32)}
    p = params()
    for k in range(steps):
        world_chain.oracle_world_step(p, w)
        now = hits_of(w, rays)
        st = ref.states(w, rays, before)
        assert st["shape"].tolist() == now
        out["hits_%d" % k] = np.array(now, dtype=np.int32)
        out["events_%d" % k] = ref.events_of(before, st)
        out["plain_%d" % k] = np.array(hits_of(w, rays, False), dtype=np.int32)
        before = now
    return out


def fixture_path(name):
    return os.path.join(GOLDEN, "%s.npz" % name)


def load_fixture(name):
    d = np.load(fixture_path(name))
    return {k: np.ascontiguousarray(d[k]) for k in d.files}


def fixture_world(fx):
    return {k: fx[k].copy() for k in WORLD_KEYS}


def coverage(fx):
    """What every scene must show by the statement alone, in the order of COVERAGE"""
    rays = fx["rays"]
    fixed, mounted = rays["body"] < 0, rays["body"] >= 0
    skip = (rays["flags"] & wire.RAY_SENSOR_SKIP_STATIC) != 0
    events = [fx["events_%d" % k] for k in range(STEPS)]
    every = np.concatenate(events)
    counts = [int(((every["shapeBefore"] < 0) & (every["shapeNow"] >= 0)).sum()), int(((every["shapeBefore"] >= 0) & (every["shapeNow"] < 0)).sum()),
              int(((every["shapeBefore"] >= 0) & (every["shapeNow"] >= 0)).sum())]
    hits = np.stack([fx["hits_%d" % k] for k in range(STEPS)])
    plain = np.stack([fx["plain_%d" % k] for k in range(STEPS)])
    counts += [int((hits[:, fixed] >= 0).sum()), int((hits[:, mounted] >= 0).sum()), int((hits[:, mounted] != plain[:, mounted]).sum()),
               int((hits[:, skip] != plain[:, skip]).sum()), sum(1 for e in events if len(e) == 0)]
    return tuple(counts)


def assert_coverage(fx, what):
    got = coverage(fx)
    assert all(x >= 1 for x in got), "%s: %s" % (what, dict(zip(COVERAGE, got)))


def build_fixture(name):
    world, rays = scene(name)
    fx = {k: world[k] for k in WORLD_KEYS}
    fx["rays"] = rays
    fx.update(run_statement(world, rays))
    return fx


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for name in SCENES:
        built = build_fixture(name)
        print("%s: %d rays, %s" % (name, len(built["rays"]), dict(zip(COVERAGE, coverage(built)))))
        for step in range(STEPS):
            print("  step %2d hits %s events %s" % (step, built["hits_%d" % step].tolist(), [tuple(int(x) for x in e) for e in built["events_%d" % step]]))
        assert_coverage(built, name)
        np.savez_compressed(fixture_path(name), **built)
        print("  %d bytes" % os.path.getsize(fixture_path(name)))
