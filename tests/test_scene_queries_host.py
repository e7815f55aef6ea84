"""Scene queries on the resident world, the part that needs no GPU: the interface as declared and bound, and the statement the GPU tests
compare bytes against (tests/scene_query_ref.py) pinned to the reference's own s2World_QueryAABB and s2Shape_TestPoint, and to the
fixtures tests/golden/scene_query/*.npz."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import scene_query_ref as ref, scene_query_world as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_ray_cast", "s2amd_world_point_probe", "s2amd_world_query_boxes")
SCENES = (("mixed", 24), ("shapes_zoo", 0), ("tumbler", 60), ("pyramid", 8))


def test_header_declares_the_calls_and_the_structs():
    header = open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(s2amdSolver\*" % call, header), call
    for struct in ("s2amdRay", "s2amdRayHit", "s2amdPointProbe", "s2amdBoxQuery"):
        assert re.search(r"typedef struct %s\b" % struct, header) and re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header)


def test_wire_sizes_and_bindings():
    assert wire.API_VERSION == 5
    assert (wire.ray_dtype.itemsize, wire.ray_hit_dtype.itemsize, wire.point_probe_dtype.itemsize, wire.box_query_dtype.itemsize) == (24, 32, 12, 20)
    assert (wire.RAY_SIZE, wire.RAY_HIT_SIZE, wire.POINT_PROBE_SIZE, wire.BOX_QUERY_SIZE) == (24, 32, 12, 20)
    assert wire.ray_hit_dtype.fields["fraction"][1] == 8 and wire.ray_hit_dtype.fields["normal"][1] == 20
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert lib.s2amd_api_version() == 5
        for call in CALLS:
            assert call in hip.EXPORTS and getattr(lib, call).argtypes is not None, call
    for method in ("world_ray_cast", "world_point_probe", "world_query_boxes"):
        assert callable(getattr(hip.Solver, method))


@needs_reference
def test_the_reference_functions_answer_as_the_statement_expects_them_to():
    """s2RayCastPolygon on a unit box: the ray (-2, 0.1) -> (2, 0.1) enters through the left face at 0.375"""
    box = ref.Polygon()
    for i, (v, n) in enumerate(zip([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)], [(0, -1), (1, 0), (0, 1), (-1, 0)])):
        box.vertices[i], box.normals[i] = ref.Vec2(*v), ref.Vec2(*n)
    box.count = 4
    ray = ref.RayCastInput(ref.Vec2(-2.0, 0.1), ref.Vec2(2.0, 0.1), 1.0)
    out = ref.lib().s2RayCastPolygon(ray, box)
    assert out.hit and out.fraction == 0.375 and (out.normal.x, out.normal.y) == (-1.0, 0.0)


@needs_reference
@pytest.mark.parametrize("scene,p0", SCENES)
def test_box_statement_is_the_reference_world_query(scene, p0):
    """200 boxes per scene after 30 steps: the statement's hits with every mask bit set are exactly the set s2World_QueryAABB calls back for"""
    ref_world, world = sq.reference_world(scene, p0, 30)
    try:
        assert (world["shapes"]["categoryBits"][world["shapes"]["type"] != wire.SHAPE_FREE] != 0).all()
        boxes = sq.random_boxes(world, 200, 11)
        offsets, shapes = ref.query_boxes(world, boxes)
        nonempty = 0
        for i, q in enumerate(boxes):
            want = sorted(s.index for s in ref.ref_query_aabb(ref_world.id, q["box"]))
            assert len(set(want)) == len(want)
            assert shapes[offsets[i]:offsets[i + 1]].tolist() == want, (scene, i, q)
            nonempty += len(want) > 0
        assert nonempty >= 50, nonempty  # (the comparison is of hits, not of empty answers)
    finally:
        ref_world.close()


@needs_reference
@pytest.mark.parametrize("scene,p0", SCENES)
def test_point_statement_is_the_reference_pick(scene, p0):
    """Picking as the reference's samples do it -- s2World_QueryAABB with the box {p, p}, then s2Shape_TestPoint -- gives exactly the
    statement's hit list: at shape centres, on polygon vertices and at random points"""
    ref_world, world = sq.reference_world(scene, p0, 30)
    try:
        _, probes, _ = sq.make_batch(world, (0, 200, 2), 12)
        probes["maskBits"] = ref.ALL_BITS
        offsets, shapes = ref.point_probe(world, probes)
        for i, q in enumerate(probes):
            assert shapes[offsets[i]:offsets[i + 1]].tolist() == ref.ref_pick(ref_world.id, q["p"]), (scene, i, q)
        assert len(shapes) >= 60, len(shapes)
    finally:
        ref_world.close()


@pytest.mark.parametrize("name", sq.FIXTURES)
def test_fixtures_are_what_they_say(name):
    """Shapes, tiles and hits as the GPU tests need them: more than half of the rays hit, so a kernel answering "no hit" cannot pass"""
    fx = sq.load_fixture(name)
    shapes, hits = fx["shapes"], fx["hits"]
    assert (len(fx["rays"]), len(fx["probes"]), len(fx["boxes"])) == sq.BATCH[name]
    assert 2 * int((hits["shape"] >= 0).sum()) >= len(hits)
    assert len(fx["probe_shapes"]) >= len(fx["probes"]) // 4 and len(fx["box_shapes"]) >= len(fx["boxes"])
    assert (np.diff(fx["box_offsets"]) == 0).any() and (np.diff(fx["probe_offsets"]) == 0).any()
    live = shapes["type"] != wire.SHAPE_FREE
    won = hits["shape"][hits["shape"] >= 0]
    assert set(shapes["type"][won].tolist()) >= ({0, 1, 2} if name != "pyramid30" else {2})
    if name == "zoo":
        assert len(shapes) <= 256 and set(shapes["type"][live].tolist()) == {0, 1, 2, 3}
    else:
        assert 256 < len(shapes) <= 512
        assert (won < 256).any() and (won >= 256).any()
        assert (fx["probe_shapes"] >= 256).any() and (fx["box_shapes"] >= 256).any() and (fx["box_shapes"] < 256).any()
    if name == "synthetic":
        assert (~live[:256]).any() and (~live[256:]).any()
        rot = fx["bodies"]["rot"][shapes["body"][live]]
        assert (rot[:, 0] != 0).sum() > 200
        s_rays, s_probes, s_boxes, answers = sq.special_cases()
        assert hits["shape"][:len(answers)].tolist() == answers
        assert fx["rays"][:len(s_rays)].tobytes() == s_rays.tobytes()
        tie = hits[0]
        for key in ("body", "type", "radius", "vertices", "fatAABB", "categoryBits"):
            assert np.array_equal(shapes[sq.TIE_LOW][key], shapes[sq.TIE_HIGH][key]), key
        assert tie["shape"] == sq.TIE_LOW and sq.TIE_LOW < 256 <= sq.TIE_HIGH
        po, ps = fx["probe_offsets"], fx["probe_shapes"]
        assert ps[po[0]:po[1]].tolist() == [sq.BIG_BOX]         # exactly on the box's corner
        assert ps[po[2]:po[3]].tolist() == [sq.MASKED_NEAR] and ps[po[3]:po[4]].tolist() == []
        assert ps[po[5]:po[6]].tolist() == [sq.BIG_CIRCLE]      # on the circle's rim
        bo, bs = fx["box_offsets"], fx["box_shapes"]
        assert bo[3] - bo[2] == 0 and bs[bo[5]:bo[6]].tolist() == [sq.MASKED_NEAR]
        assert hits["fraction"][10] == 0.0 and hits["shape"][10] == -1 and fx["rays"]["maxFraction"][10] == 0.0


@needs_reference
@pytest.mark.parametrize("name", sq.FIXTURES)
def test_fixtures_equal_the_statement_rerun(name):
    fx = sq.load_fixture(name)
    again = sq.expected(sq.fixture_world(fx), fx["rays"], fx["probes"], fx["boxes"])
    for key in sq.RESULT_KEYS:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key


def test_the_synthetic_fixture_is_the_synthetic_world():
    fx = sq.load_fixture("synthetic")
    world = sq.synthetic_world()
    for key in ("bodies", "shapes", "origins"):
        assert np.ascontiguousarray(world[key]).tobytes() == fx[key].tobytes(), key
