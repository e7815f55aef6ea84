"""Shape casts on the resident world, the part that needs no GPU: the interface as declared and bound, the statement
(tests/shape_cast_ref.py: numpy around the reference's own s2ShapeDistance) pinned to closed forms and checked against sampled
geometry, the fixtures tests/golden/shape_cast/*.npz, and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import hostcheck_util, proximity_ref as pref, scene_query_world as sq, shape_cast_ref as ref, shape_cast_world as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_cast_shape", "s2amd_world_cast_shape_all")
f32 = np.float32
IDENTITY = (0.0, 1.0)


def test_header_declares_the_calls_and_the_structs():
    header = open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(s2amdSolver\*" % call, header), call
    for struct in ("s2amdShapeCast", "s2amdShapeCastHit"):
        assert re.search(r"typedef struct %s\b" % struct, header) and re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header)
    # the three lists of what is not offered no longer name shape casts
    for path in (os.path.join(ROOT, "include", "solver2d_amd.h"), os.path.join(ROOT, "DESIGN.md")):
        for line in open(path):
            assert not (("ot offered" in line or "ut of scope" in line or "left out on purpose" in line) and "shape casts" in line), (path, line)


def test_wire_sizes_and_bindings():
    assert wire.API_VERSION == 5
    assert (wire.shape_cast_dtype.itemsize, wire.shape_cast_hit_dtype.itemsize) == (112, 48)
    assert (wire.SHAPE_CAST_SIZE, wire.SHAPE_CAST_HIT_SIZE) == (112, 48)
    c, h = wire.shape_cast_dtype.fields, wire.shape_cast_hit_dtype.fields
    assert [c[k][1] for k in ("vertices", "count", "radius", "position", "rot", "translation", "maxFraction", "maskBits", "pad")] == [
        0, 64, 68, 72, 80, 88, 96, 100, 104]
    assert [h[k][1] for k in ("shape", "body", "fraction", "distance", "point", "normal", "iterations", "pad")] == [0, 4, 8, 12, 16, 24, 32, 36]
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert lib.s2amd_api_version() == 5
        for call in CALLS:
            assert call in hip.EXPORTS and getattr(lib, call).argtypes is not None, call
    for method in ("world_cast_shape", "world_cast_shape_all"):
        assert callable(getattr(hip.Solver, method))


def test_the_constants_are_the_statement_s():
    assert ref.TARGET == f32(0.005) and ref.TOLERANCE == f32(f32(0.25) * f32(0.005)) and ref.THRESHOLD == f32(ref.TARGET + ref.TOLERANCE)
    assert ref.SPECULATIVE == f32(0.02) >= ref.THRESHOLD and ref.CAP == 20


def _circle_at_the_box(translation, max_fraction=1.0, position=(0.0, 0.0)):
    """A circle of radius 0.25 cast at a unit box centred at (3, 0) -> C(q, s)"""
    c = cw.make_cast(cw.POINT, 0.25, position, 0.0, translation, max_fraction)
    return ref.cast_against(c, pref.make_proxy(c["vertices"], 1, c["radius"]), pref.make_proxy(cw.BOX, 4, 0.0), pref.transform((3.0, 0.0), IDENTITY)), c


@needs_reference
def test_the_statement_answers_its_closed_forms():
    # 2.25 apart at the start: one advance of (2.25 - target) / 4, after which the distance is the target
    (t, d, k), c = _circle_at_the_box((4.0, 0.0))
    h = ref._record(7, 3, t, d, k)
    assert k == 1 and h["iterations"] == 1 and tuple(h["normal"]) == (-1.0, 0.0) and tuple(h["point"]) == (2.5, 0.0)
    assert abs(float(t) - 0.56125) <= 1e-6 and f32(d.distance) < ref.THRESHOLD and h["fraction"] == t and (h["shape"], h["body"]) == (7, 3)
    # the same cast cut short before it gets there; and away from the box: a miss at k = 0
    assert _circle_at_the_box((4.0, 0.0), 0.5)[0] is None
    assert _circle_at_the_box((-4.0, 0.0))[0] is None
    # started inside the box: a hit where it stands, overlapping, so without a normal
    (t, d, k), c = _circle_at_the_box((4.0, 0.0), position=(3.0, 0.1))
    h = ref._record(0, 0, t, d, k)
    assert t == 0 and k == 0 and d.distance == 0 and tuple(h["normal"]) == (0.0, 0.0)
    # no translation: within reach a hit at 0, out of reach a miss
    assert _circle_at_the_box((0.0, 0.0), position=(2.248, 0.0))[0][2] == 0
    assert _circle_at_the_box((0.0, 0.0))[0] is None


@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_are_what_they_say(name):
    """The batch as the GPU tests need it: a kernel answering "nothing", "zero" or "first candidate" cannot pass"""
    fx = cw.load_fixture(name)
    casts, first, offsets, hits = fx["casts"], fx["first"], fx["all_offsets"], fx["all_hits"]
    n = len(casts)
    assert n == cw.CASTS == 256 and len(first) == n and len(offsets) == n + 1 and len(hits) == offsets[-1]
    assert set(fx) == {"casts", "first", "all_offsets", "all_hits", "bodies", "shapes", "origins"}
    assert os.path.getsize(cw.fixture_path(name)) <= max(os.path.getsize(sq.fixture_path(f)) for f in sq.FIXTURES)
    for count in range(1, 9):
        for with_radius in (False, True):
            assert ((casts["count"] == count) & ((casts["radius"] > 0) == with_radius)).any(), (count, with_radius)
    won = first["shape"] >= 0
    lengths = np.diff(offsets)
    assert int((won & (first["fraction"] > 0)).sum()) >= 64
    assert int((won & (first["iterations"] == 0)).sum()) >= 16
    assert int((won & (first["iterations"] >= 2)).sum()) >= 32
    candidates = np.array([len(ref.candidates(fx, c)) for c in casts])
    assert int(((candidates > 0) & ~won).sum()) >= 8 and int((candidates == 0).sum()) >= 1
    assert (candidates >= lengths).all() and (candidates > lengths).any()  # (a kernel that takes every candidate for a hit is told)
    assert (casts["maskBits"] != cw.ALL).sum() >= 4 and (casts["maxFraction"] != 1).sum() >= 8
    assert not (hits["iterations"] == ref.CAP).any() and hits["iterations"].max() >= 3
    assert (hits["distance"] < ref.THRESHOLD).all() and (hits["fraction"] <= casts["maxFraction"][np.repeat(np.arange(n), lengths)]).all()
    assert (hits["pad"] == 0).all() and (first["pad"] == 0).all()
    live = fx["shapes"]["type"] != wire.SHAPE_FREE
    assert live[hits["shape"]].all() and np.array_equal(hits["body"], fx["shapes"]["body"][hits["shape"]])
    # the lists and the first-hit records agree with each other
    assert np.array_equal(won, lengths > 0)
    for i in range(n):
        mine = hits[offsets[i]:offsets[i + 1]]
        assert (np.diff(mine["shape"]) > 0).all()
        if won[i]:
            assert first[i].tobytes() == mine[np.argmin(mine["fraction"])].tobytes(), i  # (argmin: the first of equals, the lowest slot)
        else:
            assert first[i].tobytes() == ref.first_of(casts[i], []).tobytes() and first["fraction"][i] == casts["maxFraction"][i]
    assert int((lengths >= 2).sum()) >= 16 and (first["shape"][won] != hits["shape"][offsets[:-1][won]]).any()
    if name != "zoo":
        assert (first["shape"][won] < 256).any() and (first["shape"][won] >= 256).any()
    if name == "synthetic":
        s_casts, answers = cw.special_cases()
        assert casts[:len(s_casts)].tobytes() == s_casts.tobytes()
        for i, want in enumerate(answers):
            if want is not None:
                assert first["shape"][i] == want, (i, first[i])
        for key in ("body", "type", "radius", "vertices", "fatAABB", "categoryBits"):
            assert np.array_equal(fx["shapes"][sq.TIE_LOW][key], fx["shapes"][sq.TIE_HIGH][key]), key
        assert sq.TIE_LOW < 256 <= sq.TIE_HIGH
        mine = hits[offsets[0]:offsets[1]]  # both circles are in the list, at the same fraction; the record names the lower slot
        assert mine["shape"].tolist() == [sq.TIE_LOW, sq.TIE_HIGH] and mine["fraction"][0] == mine["fraction"][1] > 0
        assert hits["shape"][offsets[1]:offsets[2]].tolist() == [sq.MASKED_NEAR, sq.MASKED_FAR] and hits["shape"][offsets[2]:offsets[3]].tolist() == [sq.MASKED_FAR]
        assert first["fraction"][4] == cw.ONE_ADVANCE == casts["maxFraction"][4] and first["iterations"][4] == 1
        assert casts["maxFraction"][5] == np.nextafter(cw.ONE_ADVANCE, f32(0)) == first["fraction"][5] and candidates[5] >= 1
        assert (~live).any() and candidates[6] >= 1 and candidates[7] >= 1  # (the free slots' zeroed boxes lie under casts 6 and 7)
        assert first["fraction"][8] == 0 and first["iterations"][8] == 0 and first["fraction"][9] == 0
        assert candidates[10] >= 1 and candidates[11] >= 1


@needs_reference
@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_equal_the_statement_rerun(name):
    fx = cw.load_fixture(name)
    world = sq.fixture_world(fx)
    again = cw.expected(world, fx["casts"])
    for key in cw.RESULT_KEYS:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key
    assert cw.build_fixture(name)["casts"].tobytes() == fx["casts"].tobytes()  # (the batch generator is deterministic)
    offsets, hits = ref.cast_shape_all(world, fx["casts"][:16])
    assert offsets.tobytes() == fx["all_offsets"][:17].tobytes() and hits.tobytes() == fx["all_hits"][:offsets[-1]].tobytes()
    assert ref.cast_shape(world, fx["casts"][:16]).tobytes() == fx["first"][:16].tobytes()


@needs_reference
@pytest.mark.parametrize("name", cw.FIXTURES)
def test_the_statement_against_sampled_geometry(name):
    """Independent of the advancement loop: on the way to where the statement says a sweep ends, the reference's distance -- sampled at
    64 fractions, for 64 casts and up to 12 candidates each -- never goes below target - 1e-4 (13 ulp at coordinate 64, a twelfth of
    the tolerance): no sweep has passed through anything or come closer than it says."""
    fx = cw.load_fixture(name)
    least, taken = cw.least_sampled_distance(sq.fixture_world(fx), fx["casts"], fx["first"])
    print("%s: least sampled distance %.6f over %d samples" % (name, least, taken))
    assert taken >= 64 * 64 and least >= float(ref.TARGET) - 1e-4, (least, taken)


def test_the_statement_refuses_what_the_library_refuses():
    c = cw.make_cast(cw.BOX, 0.1, (1.0, 2.0), 0.3, (2.0, -1.0), 0.5)
    assert ref.valid_cast(c)
    for field, value in (("count", 0), ("count", 9), ("radius", -0.5), ("radius", np.nan), ("maxFraction", np.inf), ("maxFraction", -1.0),
                         ("maxFraction", np.nan)):
        bad = c.copy()
        bad[field] = value
        assert not ref.valid_cast(bad), (field, value)
    for field, index, value in (("position", 0, np.inf), ("rot", 1, np.nan), ("translation", 0, np.nan), ("translation", 1, -np.inf)):
        bad = c.copy()
        bad[field][index] = value
        assert not ref.valid_cast(bad), (field, value)
    bad = c.copy()
    bad["vertices"][4, 1] = np.nan  # (an unused vertex is not looked at)
    assert ref.valid_cast(bad)
    bad["count"] = 5
    assert not ref.valid_cast(bad)
    bad = c.copy()
    bad["pad"] = (-1, 0x7FC00000)  # (nor is the padding)
    assert ref.valid_cast(bad)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch():
    """hipcc's own report for shape_cast.hip (make resources-shape-cast), through tools/kernel_resources.py: every kernel of the file is
    there, none has a private frame or a spill, and 48 KiB of LDS a workgroup leave the candidate pass three workgroups a CU."""
    # (the kernels live in an unnamed namespace: told by their mangled names)
    kernels = dict.fromkeys(("castCandidatesKernelILb0E", "castCandidatesKernelILb1E", "castFinishKernel", "castRecordsKernel", "listTilePrefixKernel",
                             "listOffsetsKernel", "listWriteKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-shape-cast", "resources_shape_cast.txt", kernels, floor=3)
