"""Contact queries on the resident world, the part that needs no GPU: the interface as declared and bound, the reference's s2Collide*
as the statement (tests/contact_query_ref.py) calls them pinned to three closed forms, the fixtures tests/golden/contact_query/*.npz
with the conditions they must meet, and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import contact_query_ref as ref, contact_query_world as cw, hostcheck_util, proximity_world as pw, scene_query_world as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_collide_shape", "s2amd_world_deepest_contact")
IDENTITY = (0.0, 1.0)
POINT = [(0.0, 0.0)]


def test_header_declares_the_calls_and_the_structs():
    header = open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(s2amdSolver\*" % call, header), call
    for struct in ("s2amdContactQuery", "s2amdContactHit"):
        assert re.search(r"typedef struct %s\b" % struct, header) and re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header)


def test_wire_sizes_and_bindings():
    assert wire.API_VERSION == 5
    assert (wire.contact_query_dtype.itemsize, wire.contact_hit_dtype.itemsize) == (160, 80)
    assert (wire.CONTACT_QUERY_SIZE, wire.CONTACT_HIT_SIZE) == (160, 80)
    q, h, p = wire.contact_query_dtype.fields, wire.contact_hit_dtype.fields, wire.contact_hit_point_dtype.fields
    assert [q[k][1] for k in ("vertices", "normals", "type", "count", "radius", "position", "rot", "maskBits")] == [0, 64, 128, 132, 136, 140, 148, 156]
    assert [h[k][1] for k in ("shape", "body", "pointCount", "queryIsB", "normal", "points", "pad")] == [0, 4, 8, 12, 16, 24, 72]
    assert [p[k][1] for k in ("localAnchorA", "localAnchorB", "separation", "id")] == [0, 8, 16, 20] and wire.contact_hit_point_dtype.itemsize == 24
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert lib.s2amd_api_version() == 5
        for call in CALLS:
            assert call in hip.EXPORTS and getattr(lib, call).argtypes is not None, call
    for method in ("world_collide_shape", "world_deepest_contact"):
        assert callable(getattr(hip.Solver, method))


def _collide(a, at_a, b, at_b):
    return ref.collide(a, ref.transform(at_a, IDENTITY), b, ref.transform(at_b, IDENTITY))


@needs_reference
def test_the_reference_functions_answer_three_closed_forms():
    # two unit circles one unit apart: one point midway, one unit deep, the normal from A to B
    m, name = _collide(cw.make_query(cw.CIRCLE, POINT, 1.0, (0, 0), 0.0), (0.0, 0.0), cw.make_query(cw.CIRCLE, POINT, 1.0, (0, 0), 0.0), (1.0, 0.0))
    p = m.points[0]
    assert name == "s2CollideCircles" and m.pointCount == 1 and (m.normal.x, m.normal.y) == (1.0, 0.0) and p.separation == -1.0
    assert (p.localAnchorA.x, p.localAnchorA.y, p.localAnchorB.x, p.localAnchorB.y) == (0.5, 0.0, -0.5, 0.0)
    # a unit box resting on a unit box, 1/16 deep: two points of that depth, the normal straight up, the ids the clipped corners'
    box = cw.make_query(cw.POLYGON, cw.BOX, 0.0, (0, 0), 0.0)
    made, mine = ref.lib().s2MakeBox(0.5, 0.5), ref.geometry(box)  # (the query's geometry is what s2MakeBox makes, as values)
    assert (made.count, made.radius) == (mine.count, mine.radius) == (4, 0.0)
    for i in range(4):
        assert (made.vertices[i].x, made.vertices[i].y, made.normals[i].x, made.normals[i].y) == (
            mine.vertices[i].x, mine.vertices[i].y, mine.normals[i].x, mine.normals[i].y), i
    m, name = _collide(box, (0.0, 0.0), box, (0.0, 0.9375))
    assert name == "s2CollidePolygons" and m.pointCount == 2 and (m.normal.x, m.normal.y) == (0.0, 1.0)
    assert [m.points[i].separation for i in (0, 1)] == [-0.0625, -0.0625]
    assert sorted((m.points[i].localAnchorA.x, m.points[i].localAnchorA.y) for i in (0, 1)) == [(-0.5, 0.46875), (0.5, 0.46875)]
    assert m.points[0].id != m.points[1].id
    # a segment under a capsule of radius 1/4 whose axis lies 1/4 + 1/64 above it: through s2MakeCapsule, two speculative points 1/64
    # apart; 1/4 + 1/32 above it is beyond the speculative distance: no points
    seg = cw.make_query(cw.SEGMENT, [(-1.0, 0.0), (1.0, 0.0)], 0.0, (0, 0), 0.0)
    cap = cw.make_query(cw.CAPSULE, [(-0.5, 0.0), (0.5, 0.0)], 0.25, (0, 0), 0.0)
    m, name = _collide(seg, (0.0, 0.0), cap, (0.0, 0.265625))
    assert name == "s2CollideSegmentAndCapsule" and m.pointCount == 2 and [m.points[i].separation for i in (0, 1)] == [0.015625, 0.015625]
    assert (m.normal.x, m.normal.y) == (0.0, 1.0)
    assert _collide(seg, (0.0, 0.0), cap, (0.0, 0.28125))[0].pointCount == 0


def test_the_order_rule_is_the_register_table():
    assert len(ref.REGISTERS) == 9 and len(ref.MIXED) == 6 and len(ref.TWO_POINT) == 5
    for a in ref.TYPES:
        for b in ref.TYPES:
            has = (a, b) in ref.REGISTERS or (b, a) in ref.REGISTERS
            assert has == (not (a == b == cw.SEGMENT)), (a, b)
    # the device's table: bit 4 * query type + shape type of 0x7723 (contact_query.hip)
    for a in ref.TYPES:
        for b in ref.TYPES:
            assert bool((0x7723 >> (4 * a + b)) & 1) == ((a, b) in ref.REGISTERS), (a, b)
    source = open(os.path.join(ROOT, "solver2d_amd", "csrc", "contact_query.hip")).read()
    assert "#define S2_CQ_PRIMARY 0x7723u" in source


def coverage(fixtures):
    """What the fixtures hold, from the reference alone: {(function, query is B, point count)}, and per fixture the flags of the
    conditions below"""
    seen, flags = set(), {}
    for name, fx in fixtures.items():
        world, f = sq.fixture_world(fx), {}
        shapes = world["shapes"]
        with_hit = 0
        for q in fx["queries"]:
            found = ref.query_hits(world, q)
            for h, fn in found:
                seen.add((fn, int(h["queryIsB"]), int(h["pointCount"])))
                sep = h["points"]["separation"][:h["pointCount"]]
                f["speculative"] = f.get("speculative", False) or bool((sep > 0).any())
                f["penetrating"] = f.get("penetrating", False) or bool((sep < 0).any())
            slots = [int(h["shape"]) for h, _ in found]
            with_hit += bool(found)
            cands = ref.candidates(world, q)
            f["no candidate"] = f.get("no candidate", False) or not cands
            f["candidates, no hit"] = f.get("candidates, no hit", False) or (bool(cands) and not found)
            f["both tiles"] = f.get("both tiles", False) or (any(s < 256 for s in slots) and any(s >= 256 for s in slots))
            if int(q["type"]) == cw.SEGMENT:
                boxed = ref._candidates(shapes, ref.query_box(q), q["maskBits"])
                f["segment over segment"] = f.get("segment over segment", False) or bool((shapes["type"][boxed] == cw.SEGMENT).any())
            if q["maskBits"] != cw.ALL:
                open_q = q.copy()
                open_q["maskBits"] = cw.ALL
                best = ref.deepest_contact(world, [open_q])[0]["shape"]
                if best >= 0 and (shapes["categoryBits"][best] & q["maskBits"]) == 0:
                    f["nearest masked out"] = True
            if len(found) >= 2:
                keys = sorted((ref.orderable(ref.least_separation(h)), int(h["shape"])) for h, _ in found)
                f["tie"] = f.get("tie", False) or keys[0][0] == keys[1][0]
        f["half hit"] = 2 * with_hit >= len(fx["queries"])
        flags[name] = f
    return seen, flags


@needs_reference
def test_the_fixtures_meet_the_coverage_conditions():
    fixtures = {name: cw.load_fixture(name) for name in cw.FIXTURES}
    seen, flags = coverage(fixtures)
    functions = sorted(set(ref.REGISTERS.values()))
    for fn in functions:  # each of the nine with the query as A
        assert any(s[0] == fn and s[1] == 0 for s in seen), fn
    for fn in ref.MIXED:  # each of the six mixed-type ones with the query as B
        assert any(s[0] == fn and s[1] == 1 for s in seen), fn
    for fn in ref.TWO_POINT:  # each that can return two points, with 1 and with 2
        for points in (1, 2):
            assert any(s[0] == fn and s[2] == points for s in seen), (fn, points)
    assert all(s[2] in (1, 2) for s in seen)
    for flag in ("no candidate", "candidates, no hit", "nearest masked out", "segment over segment", "both tiles", "tie", "speculative",
                 "penetrating"):
        assert any(f.get(flag) for f in flags.values()), flag
    assert flags["synthetic"].get("tie") and flags["pyramid30"].get("both tiles")
    for name in cw.FIXTURES:
        assert flags[name]["half hit"], name


@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_are_what_they_say(name):
    fx = cw.load_fixture(name)
    queries, offsets, hits, deepest = fx["queries"], fx["offsets"], fx["hits"], fx["deepest"]
    n = len(queries)
    assert n == cw.QUERIES == 256 and len(deepest) == n and len(offsets) == n + 1 and len(hits) == offsets[-1]
    assert hits.dtype == deepest.dtype == wire.contact_hit_dtype and queries.dtype == wire.contact_query_dtype
    assert os.path.getsize(cw.fixture_path(name)) <= max(os.path.getsize(pw.fixture_path(f)) for f in pw.FIXTURES)
    counts = np.diff(offsets)
    assert 2 * int((counts > 0).sum()) >= n and (counts == 0).any()
    assert set(hits["pointCount"].tolist()) == {1, 2} and (hits["pad"] == 0).all()
    one = hits["pointCount"] == 1
    assert not hits["points"][one][:, 1].tobytes().strip(b"\0")  # a point >= pointCount is all zero bits
    live = fx["shapes"]["type"] != wire.SHAPE_FREE
    assert live[hits["shape"]].all() and np.array_equal(fx["shapes"]["body"][hits["shape"]], hits["body"])
    for i in range(n):  # ascending by slot; the deepest record is one of the list's, or the no-hit record
        mine = hits[offsets[i]:offsets[i + 1]]
        assert (np.diff(mine["shape"]) > 0).all()
        if len(mine) == 0:
            blank = np.zeros(1, dtype=wire.contact_hit_dtype)[0]
            blank["shape"] = blank["body"] = -1
            assert deepest[i].tobytes() == blank.tobytes()
        else:
            least = [min(float(s) for s in h["points"]["separation"][:h["pointCount"]]) for h in mine]
            k = int(np.argmin(least))  # (the first of equal ones: the lowest slot)
            assert deepest[i].tobytes() == mine[k].tobytes(), i
    if name == "synthetic":
        s_queries, answers = cw.special_cases()
        assert queries[:len(s_queries)].tobytes() == s_queries.tobytes()
        for i, want in enumerate(answers):
            if want is not None:
                assert deepest["shape"][i] == want, (i, deepest[i])
        for i in (0, 1):  # both identical circles are in the list with one manifold; the record names the lower slot
            mine = hits[offsets[i]:offsets[i + 1]]
            low, high = mine[mine["shape"] == sq.TIE_LOW][0], mine[mine["shape"] == sq.TIE_HIGH][0]
            assert low["points"].tobytes() == high["points"].tobytes() and low["normal"].tobytes() == high["normal"].tobytes()
        assert hits[offsets[2]:offsets[3]]["shape"].tolist() == [sq.MASKED_NEAR, sq.MASKED_FAR]
        assert hits[offsets[3]:offsets[4]]["shape"].tolist() == [sq.MASKED_FAR]
        rest = deepest[5]
        assert rest["pointCount"] == 2 and rest["queryIsB"] == 0 and tuple(rest["normal"]) == (0.0, -1.0)
        assert np.allclose(rest["points"]["separation"], -0.005, atol=1e-6)
        assert deepest[7]["pointCount"] == 2 and (deepest[7]["points"]["separation"] > 0).all()
        assert deepest[9]["pointCount"] == 1 and deepest[9]["queryIsB"] == 1 and deepest[9]["points"]["separation"][0] > 0


@needs_reference
@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_equal_the_statement_rerun(name):
    fx = cw.load_fixture(name)
    again = cw.expected(sq.fixture_world(fx), fx["queries"])
    for key in cw.RESULT_KEYS:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key
    assert cw.build_fixture(name)["queries"].tobytes() == fx["queries"].tobytes()


def test_the_statement_refuses_what_the_library_refuses():
    poly = cw.make_query(cw.POLYGON, cw.BOX, 0.1, (1.0, 2.0), 0.3)
    seg = cw.make_query(cw.SEGMENT, [(-1.0, 0.0), (1.0, 0.0)], 0.0, (1.0, 2.0), 0.3)
    circle = cw.make_query(cw.CIRCLE, POINT, 0.5, (1.0, 2.0), 0.3)
    assert ref.valid_query(poly) and ref.valid_query(seg) and ref.valid_query(circle)
    for field, value in (("type", -1), ("type", 4), ("count", 2), ("count", 9), ("radius", -0.5), ("radius", np.nan), ("radius", np.inf)):
        bad = poly.copy()
        bad[field] = value
        assert not ref.valid_query(bad), (field, value)
    for field in ("position", "rot"):
        for k in (0, 1):
            bad = circle.copy()
            bad[field][k] = np.inf
            assert not ref.valid_query(bad), field
    bad = poly.copy()
    bad["normals"][3, 1] = np.nan
    assert not ref.valid_query(bad)
    bad["count"] = 3  # (an unused normal or vertex is not looked at)
    bad["vertices"][3, 0] = np.nan
    assert ref.valid_query(bad)
    ok = seg.copy()
    ok["radius"], ok["count"], ok["vertices"][2], ok["normals"][0] = np.nan, 77, np.nan, np.nan  # (what a segment does not read)
    assert ref.valid_query(ok)
    bad = circle.copy()
    bad["vertices"][0, 1] = np.nan
    assert not ref.valid_query(bad)
    ok = circle.copy()
    ok["vertices"][1] = np.nan
    assert ref.valid_query(ok)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_are_in_the_resource_report():
    """hipcc's own report for contact_query.hip (make resources-contact-query), through tools/kernel_resources.py: every kernel of the
    file is there; the staging and list kernels have no private frame, the manifold kernels at most narrowphase.hip's 144 bytes a lane,
    and 64 KiB of LDS a workgroup leave two workgroups a CU."""
    rows = hostcheck_util.kernel_rows("resources-contact-query", "resources_contact_query.txt")
    for kernel, frame in (("contactCandidatesKernelILb0E", 144), ("contactCandidatesKernelILb1E", 144), ("contactDeepestKernel", 144),
                          ("contactRecordsKernel", 144), ("contactStageKernel", 0), ("listTilePrefixKernel", 0), ("listOffsetsKernel", 0),
                          ("listWriteKernel", 0)):
        found = [r for r in rows if kernel in r["mangled"]]
        assert len(found) == 1, (kernel, [r["mangled"] for r in rows if "Kernel" in r["mangled"]])
        r = found[0]
        assert r["ScratchSize"] <= frame and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["Occupancy"] >= 2, r
