"""Proximity queries on the resident world, the part that needs no GPU: the interface as declared and bound, the reference's
s2ShapeDistance as the statement (tests/proximity_ref.py) calls it pinned to three closed forms, the fixtures
tests/golden/proximity/*.npz, and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import hostcheck_util, proximity_ref as ref, proximity_world as pw, scene_query_world as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_closest_shape", "s2amd_world_shapes_in_range")
BOX = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
IDENTITY = (0.0, 1.0)


def test_header_declares_the_calls_and_the_structs():
    header = open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(s2amdSolver\*" % call, header), call
    for struct in ("s2amdProximityQuery", "s2amdProximityHit"):
        assert re.search(r"typedef struct %s\b" % struct, header) and re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header)


def test_wire_sizes_and_bindings():
    assert wire.API_VERSION == 5
    assert (wire.proximity_query_dtype.itemsize, wire.proximity_hit_dtype.itemsize) == (96, 32)
    assert (wire.PROXIMITY_QUERY_SIZE, wire.PROXIMITY_HIT_SIZE) == (96, 32)
    q, h = wire.proximity_query_dtype.fields, wire.proximity_hit_dtype.fields
    assert [q[k][1] for k in ("vertices", "count", "radius", "position", "rot", "maxDistance", "maskBits")] == [0, 64, 68, 72, 80, 88, 92]
    assert [h[k][1] for k in ("shape", "body", "distance", "pointA", "pointB", "iterations")] == [0, 4, 8, 12, 20, 28]
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert lib.s2amd_api_version() == 5
        for call in CALLS:
            assert call in hip.EXPORTS and getattr(lib, call).argtypes is not None, call
    for method in ("world_closest_shape", "world_shapes_in_range"):
        assert callable(getattr(hip.Solver, method))


def _distance(verts_a, radius_a, at_a, verts_b, radius_b, at_b):
    return ref.shape_distance(ref.make_proxy(verts_a, len(verts_a), radius_a), ref.transform(at_a, IDENTITY),
                              ref.make_proxy(verts_b, len(verts_b), radius_b), ref.transform(at_b, IDENTITY))


@needs_reference
def test_the_reference_function_answers_three_closed_forms():
    # a unit box at the origin against a circle of radius 0.25 at (2, 0)
    d = _distance(BOX, 0.0, (0.0, 0.0), [(0.0, 0.0)], 0.25, (2.0, 0.0))
    assert (d.distance, d.pointA.x, d.pointA.y, d.pointB.x, d.pointB.y, d.iterations) == (1.25, 0.5, 0.0, 1.75, 0.0, 3)
    # two circles, radii 0.5 and 0.25, centres 3 apart
    d = _distance([(0.0, 0.0)], 0.5, (1.0, 2.0), [(0.0, 0.0)], 0.25, (4.0, 2.0))
    assert (d.distance, d.pointA.x, d.pointA.y, d.pointB.x, d.pointB.y, d.iterations) == (2.25, 1.5, 2.0, 3.75, 2.0, 1)
    # overlapping boxes: 0, and both witnesses are the one point
    d = _distance(BOX, 0.0, (0.0, 0.0), BOX, 0.0, (0.5, 0.25))
    assert d.distance == 0.0 and (d.pointA.x, d.pointA.y) == (d.pointB.x, d.pointB.y)


@pytest.mark.parametrize("name", pw.FIXTURES)
def test_fixtures_are_what_they_say(name):
    """The batch as the GPU tests need it: every proxy count with and without a radius, three quarters placed relative to a shape, and
    enough answers of every kind that a kernel answering "nothing" or "zero" cannot pass"""
    fx = pw.load_fixture(name)
    queries, hits, offsets, shapes, distances = fx["queries"], fx["hits"], fx["range_offsets"], fx["range_shapes"], fx["range_distances"]
    n = len(queries)
    assert 256 <= n <= 384 and n == pw.QUERIES and len(hits) == n and len(offsets) == n + 1
    assert len(shapes) == len(distances) == offsets[-1]
    assert os.path.getsize(pw.fixture_path(name)) <= max(os.path.getsize(sq.fixture_path(f)) for f in sq.FIXTURES)
    assert 4 * pw.placed_relative_to_a_shape(n) >= 3 * n
    for count in range(1, 9):
        for with_radius in (False, True):
            assert ((queries["count"] == count) & ((queries["radius"] > 0) == with_radius)).any(), (count, with_radius)
    won = hits["shape"] >= 0
    assert 2 * int(won.sum()) >= n
    assert 2 * int((np.diff(offsets) > 0).sum()) >= n
    assert int((won & (hits["distance"] == 0)).sum()) >= 16
    assert pw.zero_ties(fx) >= 8
    assert int((won & (hits["distance"] > 0)).sum()) >= 8
    assert int((queries["maxDistance"] == 0).sum()) >= 8
    assert (~won).any() and (np.diff(offsets) == 0).any()
    # the lists and the records agree with each other
    for i in np.nonzero(won)[0][:64]:
        mine, dist = shapes[offsets[i]:offsets[i + 1]], distances[offsets[i]:offsets[i + 1]]
        assert hits["shape"][i] == mine[np.argmin(dist)] and hits["distance"][i] == dist.min() <= queries["maxDistance"][i]
    world_shapes = fx["shapes"]
    live = world_shapes["type"] != wire.SHAPE_FREE
    assert live[shapes].all()
    types = set(world_shapes["type"][hits["shape"][won]].tolist())
    assert types >= ({0, 1, 2, 3} if name != "pyramid30" else {2}), types  # every shape type the world holds is some query's closest
    if name != "zoo":
        assert (hits["shape"][won] < 256).any() and (hits["shape"][won] >= 256).any() and (shapes >= 256).any() and (shapes < 256).any()
    if name == "synthetic":
        s_queries, answers = pw.special_cases()
        assert queries[:len(s_queries)].tobytes() == s_queries.tobytes()
        for i, want in enumerate(answers):
            if want is not None:
                assert hits["shape"][i] == want, (i, hits[i])
        for key in ("body", "type", "radius", "vertices", "fatAABB", "categoryBits"):
            assert np.array_equal(world_shapes[sq.TIE_LOW][key], world_shapes[sq.TIE_HIGH][key]), key
        assert sq.TIE_LOW < 256 <= sq.TIE_HIGH
        for i in (0, 1):  # both circles are in the list, at the same distance; the record names the lower slot
            mine, dist = shapes[offsets[i]:offsets[i + 1]].tolist(), distances[offsets[i]:offsets[i + 1]]
            assert sq.TIE_LOW in mine and sq.TIE_HIGH in mine and dist[mine.index(sq.TIE_LOW)] == dist[mine.index(sq.TIE_HIGH)] == dist.min()
        assert hits["distance"][0] > 0 and hits["distance"][1] == 0
        assert shapes[offsets[2]:offsets[3]].tolist() == [sq.MASKED_NEAR, sq.MASKED_FAR] and shapes[offsets[3]:offsets[4]].tolist() == [sq.MASKED_FAR]
        assert hits["distance"][5] == 1.5 and hits["distance"][6] == np.nextafter(np.float32(1.5), np.float32(0.0)) and hits["iterations"][6] == 0
        assert (~live).any() and offsets[8] - offsets[7] >= 1  # (free slots' zeroed boxes lie under queries 7 and 8)


@needs_reference
@pytest.mark.parametrize("name", pw.FIXTURES)
def test_fixtures_equal_the_statement_rerun(name):
    fx = pw.load_fixture(name)
    again = pw.expected(sq.fixture_world(fx), fx["queries"])
    for key in pw.RESULT_KEYS:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key
    assert pw.build_fixture(name)["queries"].tobytes() == fx["queries"].tobytes()


def test_the_statement_refuses_what_the_library_refuses():
    q = pw.make_query(BOX, 0.1, (1.0, 2.0), 0.3, 0.5)
    assert ref.valid_query(q)
    for field, value in (("count", 0), ("count", 9), ("radius", -0.5), ("radius", np.nan), ("maxDistance", np.inf), ("maxDistance", -1.0)):
        bad = q.copy()
        bad[field] = value
        assert not ref.valid_query(bad), (field, value)
    bad = q.copy()
    bad["vertices"][3, 1] = np.nan
    assert not ref.valid_query(bad)
    bad["count"] = 3  # (an unused vertex is not looked at)
    assert ref.valid_query(bad)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch():
    """hipcc's own report for proximity_query.hip (`make resources` compiles it with the files tests/test_kernel_resources.py reads),
    through tools/kernel_resources.py: every kernel of the file is there, none has a private frame or a spill."""
    # (the kernels live in an unnamed namespace: told by their mangled names)
    kernels = {"proximityCandidatesKernelILb0E": 1, "proximityCandidatesKernelILb1E": 1, "proximityFinishKernel": 1, "proximityDistancesKernel": 1,
               "listTilePrefixKernel": 1, "listOffsetsKernel": 1, "listWriteKernel": 1}
    hostcheck_util.assert_kernel_resources("resources", None, kernels, floor=3)  # (the candidate pass: 44 KiB of LDS a workgroup, three workgroups a CU)
