"""The ray report without a GPU: the interface as declared and bound with the header's sizes and offsets, the statement
(tests/ray_report_ref.py) against the scene queries' statement, the fixtures tests/golden/ray_report/*.npz with the two conditions
every scene must meet, the compiler's resource report of the new kernels, and the host side under ASan + UBSan on the stand-in HIP
runtime of tests/hostcheck (a stand-alone program, nothing preloaded)."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import wire
from tests import hostcheck_util, proximity_ref, ray_report_ref as ref, ray_report_world as rw, scene_query_ref, world_chain

needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_set_ray_sensors", "s2amd_world_set_ray_report", "s2amd_world_ray_states", "s2amd_world_ray_ranges", "s2amd_world_export_ray_ranges",
         "s2amd_world_ray_events")
f32 = np.float32


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    fields = {"s2amdRaySensor": wire.ray_sensor_dtype, "s2amdRayState": wire.ray_state_dtype, "s2amdRayEvent": wire.ray_event_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, fields)
    assert (wire.RAY_SENSOR_SIZE, wire.RAY_STATE_SIZE, wire.RAY_EVENT_SIZE) == (48, 64, 16)


def test_header_flags_and_bindings():
    defines = {"S2AMD_MAX_RAY_SENSORS": 16384, "S2AMD_RAY_SENSOR_DISABLED": 1, "S2AMD_RAY_SENSOR_SKIP_STATIC": 2, "S2AMD_RAY_REPORT_STATES": 1,
               "S2AMD_RAY_REPORT_RANGES": 2, "S2AMD_RAY_REPORT_EVENTS": 4, "S2AMD_API_VERSION": 5}
    hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_RAY_SENSORS, wire.RAY_SENSOR_DISABLED, wire.RAY_SENSOR_SKIP_STATIC) == (16384, 1, 2)
    assert (wire.RAY_REPORT_STATES, wire.RAY_REPORT_RANGES, wire.RAY_REPORT_EVENTS, wire.RAY_REPORT_ALL) == (1, 2, 4, 7)
    assert wire.API_VERSION == 5 and wire.SENSOR_REPORT_ALL == 7 and wire.MAX_SENSORS == 1024  # the other flag spaces and the API version are untouched


def test_transform_point_by_hand():
    assert ref.transform_point((1.0, 2.0), (0.0, 1.0), (0.5, -0.25)) == (f32(1.5), f32(1.75))   # no rotation
    assert ref.transform_point((1.0, 2.0), (1.0, 0.0), (0.5, -0.25)) == (f32(1.25), f32(2.5))   # a quarter turn: (x, y) -> (-y, x)
    assert all(isinstance(v, np.float32) for v in ref.transform_point((1.0, 2.0), (0.6, 0.8), (0.5, -0.25)))


@needs_reference
def test_transform_point_is_the_reference_operation_order():
    """s2TransformPoint is inline in the reference's headers; s2ComputeCircleAABB (src/geometry.c:288-295) applies it to the circle's
    centre and subtracts the radius: with radius 0 its lower bound is the transformed point's own bits."""
    L = ctypes.CDLL(scene_query_ref.refbind.REF_SO)
    L.s2ComputeCircleAABB.restype = scene_query_ref.Box
    L.s2ComputeCircleAABB.argtypes = [ctypes.POINTER(scene_query_ref.Circle), proximity_ref.Transform]
    rng = np.random.RandomState(11)
    for _ in range(300):
        angle = rng.rand() * 6.28
        origin, rot, p = f32(rng.rand(2) * 40 - 20), (f32(np.sin(angle)), f32(np.cos(angle))), f32(rng.rand(2) * 6 - 3)
        circle = scene_query_ref.Circle(scene_query_ref.Vec2(float(p[0]), float(p[1])), 0.0)
        box = L.s2ComputeCircleAABB(ctypes.byref(circle), proximity_ref.transform(origin, rot))
        x, y = ref.transform_point(origin, rot, p)
        assert (f32(box.lowerBound.x).tobytes(), f32(box.lowerBound.y).tobytes()) == (x.tobytes(), y.tobytes())


def test_world_rays_of_inactive_rays_are_zero():
    fx = rw.load_fixture("ball")
    world, rays = rw.fixture_world(fx), fx["rays"].copy()
    off = int(np.flatnonzero(rays["flags"] & wire.RAY_SENSOR_DISABLED)[0])
    mounted = int(np.flatnonzero(rays["body"] >= 0)[0])
    assert ref.world_ray(world, rays[off]) == (False, (0.0, 0.0), (0.0, 0.0))
    active, p1, p2 = ref.world_ray(world, rays[mounted])
    assert active and p1 == ref.transform_point(world["origins"][1], world["bodies"]["rot"][1], rays[mounted]["p1"])
    on_free = rays[mounted].copy()
    on_free["body"] = 2  # a free body slot
    assert not ref.world_ray(world, on_free)[0]
    outside = rays[mounted].copy()
    outside["body"] = len(world["bodies"])
    assert not ref.world_ray(world, outside)[0]
    world["origins"][1] = (np.nan, 0.0)  # a body with a non-finite pose switches its rays off
    assert ref.world_ray(world, rays[mounted]) == (False, (0.0, 0.0), (0.0, 0.0))
    assert ref.world_ray(world, rays[0])[0]


@needs_reference
@pytest.mark.parametrize("scene", rw.SCENES)
def test_without_exclusions_fixed_rays_are_the_scene_queries_ray_cast(scene):
    """With exclusions=False and every ray fixed in the world (the mounted ones by their world ends) the statement equals
    tests/scene_query_ref.ray_cast byte for byte, on the scene's first, fourth and last state of the chain"""
    fx = rw.load_fixture(scene)
    world, rays, params = rw.fixture_world(fx), fx["rays"], rw.params()
    for k in range(rw.STEPS + 1):
        if k in (0, 4, rw.STEPS):
            plain, index = ref.world_rays(world, rays)
            fixed = np.zeros(len(plain), dtype=wire.ray_sensor_dtype)
            for name in ("p1", "p2", "maxFraction", "maskBits"):
                fixed[name] = plain[name]
            fixed["body"] = -1
            st = ref.states(world, fixed, [-1] * len(fixed), exclusions=False)
            want = scene_query_ref.ray_cast(world, plain)
            for mine, theirs in (("shape", "shape"), ("hitBody", "body"), ("fraction", "fraction"), ("point", "point"), ("normal", "normal")):
                assert st[mine].tobytes() == want[theirs].tobytes(), (scene, k, mine)
            assert st["p1"].tobytes() == plain["p1"].tobytes() and st["p2"].tobytes() == plain["p2"].tobytes() and st["active"].all()
            assert ref.ranges(world, fixed, exclusions=False).tobytes() == want["fraction"].tobytes()
            # ... and the recorded "plain" hit shapes are these
            if k > 0:
                assert fx["plain_%d" % (k - 1)][index].tolist() == want["shape"].tolist(), (scene, k)
        if k < rw.STEPS:
            world_chain.oracle_world_step(params, world)


@needs_reference
@pytest.mark.parametrize("scene", rw.SCENES)
def test_recorded_fixtures_equal_the_statement(scene):
    fx = rw.load_fixture(scene)
    built = rw.build_fixture(scene)  # (asserts the clearance condition on the way)
    assert sorted(built) == sorted(fx)
    for key in built:
        assert np.ascontiguousarray(built[key]).tobytes() == fx[key].tobytes(), (scene, key)


@pytest.mark.parametrize("scene", rw.SCENES)
def test_every_scene_meets_the_coverage_condition(scene):
    """By the recorded statement alone: every count of ray_report_world.COVERAGE is >= 1; the events replayed over the steps reproduce
    the hit shapes from "before"; the rays are the five kinds the scenes promise."""
    fx = rw.load_fixture(scene)
    rw.assert_coverage(fx, scene)
    rays = fx["rays"]
    mounted = rays["body"] >= 0
    assert mounted.sum() == 8 and len(set(rays["body"][mounted].tolist())) == 1 and (~mounted).sum() >= 4
    assert ((rays["flags"] & wire.RAY_SENSOR_DISABLED) != 0).sum() == 1 and ((rays["flags"] & wire.RAY_SENSOR_SKIP_STATIC) != 0).sum() == 1
    shapes = fx["before"].copy()
    for k in range(rw.STEPS):
        events = fx["events_%d" % k]
        assert events["ray"].tolist() == sorted(set(events["ray"].tolist()))
        for e in events:
            assert shapes[e["ray"]] == e["shapeBefore"] != e["shapeNow"]
            assert e["bodyNow"] == (fx["shapes"]["body"][e["shapeNow"]] if e["shapeNow"] >= 0 else -1)
            shapes[e["ray"]] = e["shapeNow"]
        assert shapes.tolist() == fx["hits_%d" % k].tolist(), (scene, k)
        hits = fx["hits_%d" % k]
        own = int(rays["body"][mounted][0])
        assert all(h < 0 or fx["shapes"]["body"][h] != own for h in hits[mounted])  # a mounted ray never hits its own body
        assert (fx["plain_%d" % k][mounted] >= 0).all()  # ... which it points through: without the exclusions there is always a hit
        assert hits[(rays["flags"] & wire.RAY_SENSOR_DISABLED) != 0].tolist() == [-1] and hits[-1] == -1
        skip = hits[(rays["flags"] & wire.RAY_SENSOR_SKIP_STATIC) != 0][0]
        assert skip < 0 or fx["bodies"]["type"][fx["shapes"]["body"][skip]] != wire.BODY_STATIC


def test_clearance_variations_are_what_they_say():
    rays = np.array([rw.make_ray((0.0, 0.0), (2.0, 0.0)), rw.make_ray((1.0, 1.0), (1.0, -3.0), max_fraction=0.5)], dtype=wire.ray_sensor_dtype)
    up, down, longer, shorter = rw.variations(rays)
    assert np.allclose(up["p1"], [(0.0, 1e-3), (1.0 + 1e-3, 1.0)], atol=1e-7) and np.allclose(down["p2"], [(2.0, -1e-3), (1.0 - 1e-3, -3.0)], atol=1e-7)
    assert np.allclose(longer["maxFraction"], [1.001, 0.5005], atol=1e-7) and np.allclose(shorter["maxFraction"], [0.999, 0.4995], atol=1e-7)
    for v in (up, down):
        assert v["maxFraction"].tobytes() == rays["maxFraction"].tobytes()
    for v in (longer, shorter):
        assert v["p1"].tobytes() == rays["p1"].tobytes() and v["p2"].tobytes() == rays["p2"].tobytes()


def test_kernels_use_no_scratch():
    """hipcc's own report for ray_report.hip (make resources-ray-report), through tools/kernel_resources.py: every kernel of the file is
    there, none has a private frame or spills, and the candidates pass keeps three workgroups a CU beside its 44 KiB of LDS."""
    kernels = dict.fromkeys(("rayPoseKernel", "rayReportCandidatesKernel", "rayReportFinishKernelILb0E", "rayReportFinishKernelILb1E", "rayReportEventsKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-ray-report", "resources_ray_report.txt", kernels, floor=3, every_row=True)


@hostcheck_util.needs_sanitizers
def test_ray_report_host_code_under_asan_and_ubsan(tmp_path):
    """The setter with good and bad lists -> every flag combination 0..7 -> every getter (the device export among them) with too-small,
    exact and ample heap buffers of exactly the size passed -> the list replaced and cleared between steps -> uploads with other
    capacities, worlds without shape slots among them -> destroy, for 0, 1, 257 and 16,384 rays, on the sanitizer build of
    tests/test_hostcheck.py (kernels never run there: the program writes the head through the report state's head offset, and what is
    checked is that the host code touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "ray_report_main.cpp", "RAY REPORT MAIN OK", timeout=600)
