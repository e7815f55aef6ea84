"""Move-and-slide on the resident world, the part that needs no GPU: the interface as declared and bound, the statement
(tests/mover_ref.py: numpy around the reference's own s2ShapeDistance) pinned to closed forms, to its walk over a tiled floor and to
sampled geometry, the fixtures tests/golden/mover/*.npz, and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import hostcheck_util, mover_ref as ref, mover_world as mw, proximity_ref as pref, scene_query_world as sq, shape_cast_ref as cref, shape_cast_world as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
f32 = np.float32
REACHED, BLOCKED, CORNERED, OVERLAPPED, OUT = (wire.MOVER_REACHED, wire.MOVER_BLOCKED, wire.MOVER_CORNERED, wire.MOVER_OVERLAPPED,
                                               wire.MOVER_OUT_OF_ITERATIONS)


def test_header_declares_the_call_and_the_structs():
    header = open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()
    assert re.search(r"\bint s2amd_world_move_shapes\(s2amdSolver\*", header)
    for struct in ("s2amdMover", "s2amdMoverResult", "s2amdMoverPlane"):
        assert re.search(r"typedef struct %s\b" % struct, header) and re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header)
    for name, value in (("MAX_ITERATIONS", 8), ("STATIC_ONLY", 1), ("REACHED", 0), ("BLOCKED", 1), ("CORNERED", 2), ("OVERLAPPED", 3), ("OUT_OF_ITERATIONS", 4)):
        assert re.search(r"#define S2AMD_MOVER_%s %d\b" % (name, value), header), name
        assert getattr(wire, "MOVER_" + name) == value
    assert "GRAZE" in header and "1e-4f" in header and "s2amd_world_deepest_contact" in header
    for missing in ("rotation of the mover", "pushing dynamic bodies", "step-up and step-down", "device memory", "sharded worlds", "device trees"):
        assert missing in header[header.index("Move-and-slide"):header.index("#define S2AMD_MOVER_MAX_ITERATIONS")], missing


def test_wire_sizes_and_bindings():
    assert wire.API_VERSION == 5
    assert (wire.mover_dtype.itemsize, wire.mover_result_dtype.itemsize, wire.mover_plane_dtype.itemsize) == (128, 32, 32)
    assert (wire.MOVER_SIZE, wire.MOVER_RESULT_SIZE, wire.MOVER_PLANE_SIZE) == (128, 32, 32)
    m, r, p = wire.mover_dtype.fields, wire.mover_result_dtype.fields, wire.mover_plane_dtype.fields
    assert [m[k][1] for k in ("vertices", "count", "radius", "position", "rot", "translation", "maxIterations", "maskBits", "ignoreBody", "flags",
                              "reserved")] == [0, 64, 68, 72, 80, 88, 96, 100, 104, 108, 112]
    assert [r[k][1] for k in ("position", "remaining", "status", "planeCount", "iterations", "advances")] == [0, 8, 16, 20, 24, 28]
    assert [p[k][1] for k in ("shape", "body", "fraction", "distance", "point", "normal")] == [0, 4, 8, 12, 16, 24]
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert lib.s2amd_api_version() == 5
        assert "s2amd_world_move_shapes" in hip.EXPORTS and lib.s2amd_world_move_shapes.argtypes is not None
    assert callable(hip.Solver.world_move_shapes)


def test_the_statement_refuses_what_the_library_refuses():
    """The library's list (the header's Validation; tests/test_gpu_mover.py::test_errors and tests/hostcheck/mover_main.cpp put the same
    rules to the library)"""
    m = mw.make_mover(cw.BOX, 0.1, (1.0, 2.0), 0.3, (2.0, -1.0), 4, ignore=6)
    assert ref.valid_mover(m, 7)
    for field, value in (("count", 0), ("count", 9), ("radius", -0.5), ("radius", np.nan), ("radius", np.inf), ("maxIterations", 0), ("maxIterations", 9),
                         ("maxIterations", -1), ("flags", 2), ("flags", 3), ("flags", 0x80000000), ("ignoreBody", 7), ("ignoreBody", 2 ** 31 - 1)):
        bad = m.copy()
        bad[field] = value
        assert not ref.valid_mover(bad, 7), (field, value)
    for field, index, value in (("position", 0, np.inf), ("rot", 1, np.nan), ("translation", 0, np.nan), ("translation", 1, -np.inf), ("reserved", 0, 1),
                                ("reserved", 3, -1)):
        bad = m.copy()
        bad[field][index] = value
        assert not ref.valid_mover(bad, 7), (field, value)
    ok = m.copy()
    ok["vertices"][4, 1] = np.nan  # (an unused vertex is not looked at)
    ok["ignoreBody"], ok["flags"], ok["maxIterations"] = -99, wire.MOVER_STATIC_ONLY, 8
    assert ref.valid_mover(ok, 7)
    ok["count"] = 5
    assert not ref.valid_mover(ok, 7)
    # the library's validator states the same rules
    source = open(os.path.join(ROOT, "solver2d_amd", "csrc", "mover_query.hip")).read()
    for rule in ("m.count < 1 || m.count > S2_NP_MAX_VERTS", "m.radius >= 0.0f", "m.maxIterations >= 1 && m.maxIterations <= S2AMD_MOVER_MAX_ITERATIONS",
                 "(m.flags & ~(uint32_t)S2AMD_MOVER_STATIC_ONLY) == 0u", "m.reserved[3] == 0", "ignoreBody < s->bodyCapacity"):
        assert rule in source, rule


def _box_world(extra=()):
    """A unit box centred at (3, 0) on a static body, and further boxes (x, y, hx, hy)"""
    boxes = [(3.0, 0.0, 0.5, 0.5)] + list(extra)
    bodies, shapes = np.zeros(len(boxes), dtype=wire.body_dtype), np.zeros(len(boxes), dtype=wire.shape_dtype)
    for k, (x, y, hx, hy) in enumerate(boxes):
        mw._static_box(bodies, shapes, k, hx, hy, x, y)
    return sq.empty_world(bodies, shapes, bodies["position"].copy())


@needs_reference
def test_the_statement_answers_its_closed_forms():
    world = _box_world()
    # a circle cast at the unit box lands at the shape casts' 0.56125, slides and is REACHED
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.5)))
    assert abs(float(planes["fraction"][0]) - 0.56125) <= 1e-6 and tuple(planes["normal"][0]) == (-1.0, 0.0) and planes["shape"][0] == 0
    assert (res["status"], res["planeCount"], res["iterations"]) == (REACHED, 1, 2) and res["advances"] == 1
    assert tuple(res["remaining"]) == (0.0, 0.0) and abs(float(res["position"][0]) - 2.245) <= 1e-5 and abs(float(res["position"][1]) - 0.5) <= 1e-6
    assert not planes[1:].tobytes().strip(b"\0")
    # head-on into the face is BLOCKED
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.0)))
    assert (res["status"], res["planeCount"], res["iterations"]) == (BLOCKED, 1, 1) and tuple(res["remaining"]) == (0.0, 0.0)
    assert abs(float(planes["fraction"][0]) - 0.56125) <= 1e-6 and abs(float(res["position"][0]) - 2.245) <= 1e-5
    # started inside the shape is OVERLAPPED with a zero normal, where it stood, everything left
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (3.0, 0.1), 0.0, (4.0, 0.0)))
    assert (res["status"], res["planeCount"], res["iterations"]) == (OVERLAPPED, 1, 1) and tuple(planes["normal"][0]) == (0.0, 0.0)
    assert tuple(res["position"]) == (3.0, f32(0.1)) and tuple(res["remaining"]) == (4.0, 0.0) and planes["fraction"][0] == 0 and planes["distance"][0] == 0
    # a zero translation is REACHED in one iteration with no plane -- also within reach of the box
    for position in ((0.0, 0.0), (2.248, 0.0)):
        res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, position, 0.0, (0.0, 0.0)))
        assert (res["status"], res["planeCount"], res["iterations"], res["advances"]) == (REACHED, 0, 1, 0) and not planes.tobytes().strip(b"\0")
        assert tuple(res["position"]) == tuple(f32(x) for x in position)
    # touching and leaving: the box does not block
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (2.248, 0.0), 0.0, (-1.0, 0.25)))
    assert (res["status"], res["planeCount"]) == (REACHED, 0) and tuple(res["position"]) == (f32(f32(2.248) - f32(1.0)), 0.25)
    # one iteration, something met and something left: OUT_OF_ITERATIONS
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.5), 1))
    assert (res["status"], res["planeCount"], res["iterations"]) == (OUT, 1, 1) and res["remaining"][0] == 0 and res["remaining"][1] > 0
    # into the corner of a floor and the box: two planes, CORNERED or BLOCKED, never through
    world = _box_world([(0.0, -1.0, 10.0, 0.5)])
    res, planes = ref.move(world, mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, -1.0)))
    assert res["status"] in (CORNERED, BLOCKED) and res["planeCount"] == 2 and planes["shape"][:2].tolist() == [1, 0]
    assert res["position"][0] < 2.25 and res["position"][1] > -0.25
    # ignoreBody, STATIC_ONLY and the mask take the box away
    world["bodies"]["type"][0] = wire.BODY_DYNAMIC
    world["shapes"]["categoryBits"][0] = 2
    for m in (mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.0), ignore=0), mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.0), flags=1),
              mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.0), mask=1)):
        res, planes = ref.move(world, m)
        assert (res["status"], res["planeCount"]) == (REACHED, 0) and tuple(res["position"]) == (4.0, 0.0)
    assert ref.move(world, mw.make_mover(cw.POINT, 0.25, (0.0, 0.0), 0.0, (4.0, 0.0), ignore=1))[0]["status"] == BLOCKED


@pytest.mark.parametrize("name", mw.FIXTURES)
def test_fixtures_are_what_they_say(name):
    """The batch as the GPU tests need it: a kernel answering "nothing", "first cast only" or "never slides" cannot pass"""
    fx = mw.load_fixture(name)
    movers, results, planes, first = fx["movers"], fx["results"], fx["planes"], fx["first"]
    n = len(movers)
    assert n == mw.MOVERS == 256 and len(results) == n and planes.shape == (n, 8)
    assert set(fx) == {"movers", "results", "planes", "first", "bodies", "shapes", "origins"}
    assert os.path.getsize(mw.fixture_path(name)) <= max(os.path.getsize(sq.fixture_path(f)) for f in sq.FIXTURES)
    # the batch is the shape-cast batch of the same world
    casts = cw.load_fixture(name)["casts"]
    body = slice(0, n - mw.DIRECTED)
    assert movers[body].tobytes() == mw.from_casts(casts)[body].tobytes() and (movers["maxIterations"][body] == 4).all()
    status, count = results["status"], results["planeCount"]
    assert int((count >= 1).sum()) >= 64
    assert int(((count >= 2) & (planes["fraction"][:, 1] > 0)).sum()) >= 8
    assert int((status == OVERLAPPED).sum()) >= 16
    assert int((status == CORNERED).sum()) >= 1
    assert len(first) >= 64 and (count[first] >= 1).all()
    # ... and the directed movers
    directed = slice(n - mw.DIRECTED, n)
    assert int((status[directed] == BLOCKED).sum()) >= 4 and int((status[directed] == OUT).sum()) >= 4 and int((count[directed] >= 3).sum()) >= 4
    assert int((status[directed] == CORNERED).sum()) >= 4 and int((status[directed] == OVERLAPPED).sum()) >= 2  # (started inside a shape)
    series = movers[directed][:8]
    assert series["maxIterations"].tolist() == list(range(1, 9)) and len(set(series[k].tobytes() for k in ("position", "translation", "vertices"))) == 3
    assert (series["position"] == series["position"][0]).all() and (series["translation"] == series["translation"][0]).all()
    assert (movers["ignoreBody"][directed] >= 0).sum() == 2 and (movers["flags"][directed] == wire.MOVER_STATIC_ONLY).sum() == 1
    assert (movers["maskBits"][directed] != mw.ALL).sum() == 1
    # the records hold together
    live = fx["shapes"]["type"] != wire.SHAPE_FREE
    assert ((status >= 0) & (status <= 4)).all() and (results["iterations"] >= 1).all() and (results["iterations"] <= movers["maxIterations"]).all()
    assert (count <= results["iterations"]).all()
    for i in range(n):
        mine = planes[i, :count[i]]
        assert not planes[i, count[i]:].tobytes().strip(b"\0"), i
        assert live[mine["shape"]].all() and np.array_equal(mine["body"], fx["shapes"]["body"][mine["shape"]]) and len(set(mine["shape"])) == count[i]
        if movers["ignoreBody"][i] >= 0:
            assert not (mine["body"] == movers["ignoreBody"][i]).any()
        if movers["flags"][i] & wire.MOVER_STATIC_ONLY:
            assert (fx["bodies"]["type"][mine["body"]] == wire.BODY_STATIC).all()
        assert ((fx["shapes"]["categoryBits"][mine["shape"]] & movers["maskBits"][i]) != 0).all()
        if status[i] == REACHED:
            assert tuple(results["remaining"][i]) == (0.0, 0.0) and results["iterations"][i] == count[i] + 1
        if status[i] == OVERLAPPED:
            assert tuple(mine["normal"][-1]) == (0.0, 0.0) and mine["distance"][-1] == 0
        if status[i] == BLOCKED:
            assert tuple(results["remaining"][i]) == (0.0, 0.0) and count[i] >= 1
        if status[i] == OUT:
            assert results["iterations"][i] == movers["maxIterations"][i] == count[i] and np.any(results["remaining"][i] != 0)
        if status[i] == CORNERED:
            assert count[i] >= 2
    if name != "zoo":
        shapes_met = np.concatenate([planes["shape"][i, :count[i]] for i in range(n)])
        assert (shapes_met < 256).any() and (shapes_met >= 256).any()
    if name == "synthetic":
        assert planes["shape"][0, 0] == sq.TIE_LOW and sq.TIE_LOW < 256 <= sq.TIE_HIGH  # the tie pair across two tiles: the lower slot
        assert planes["shape"][1, 0] == sq.MASKED_NEAR and planes["shape"][2, 0] == sq.MASKED_FAR and count[3] == 0


@pytest.mark.parametrize("name", mw.FIXTURES)
def test_plane_0_is_the_shape_casts_first_hit(name):
    """At least 64 movers whose plane 0 is the first hit s2amd_world_cast_shape reports: read from the shape-cast fixture, whose casts
    the batch was built from (the movers whose cast had maxFraction 1 make the very same cast)"""
    fx, cfx = mw.load_fixture(name), cw.load_fixture(name)
    same = np.nonzero(cfx["casts"]["maxFraction"][:mw.MOVERS - mw.DIRECTED] == 1)[0]
    hits, planes = cfx["first"][same], fx["planes"][same, 0]
    agree = [i for i in range(len(same)) if hits["shape"][i] >= 0 and
             all(hits[k][i].tobytes() == planes[k][i].tobytes() for k in ("shape", "body", "fraction", "distance", "point", "normal"))]
    assert len(agree) >= 64 and set(same[agree]) <= set(fx["first"].tolist())
    # the others are the statement's exception: touching at the start, and leaving or sliding along
    for i in set(range(len(same))) - set(agree):
        if hits["shape"][i] >= 0:
            assert hits["fraction"][i] == 0 and hits["iterations"][i] == 0 and np.any(hits["normal"][i] != 0), i


@needs_reference
@pytest.mark.parametrize("name", mw.FIXTURES)
def test_fixtures_equal_the_statement_rerun(name):
    fx = mw.load_fixture(name)
    world = sq.fixture_world(fx)
    again = mw.expected(world, fx["movers"])
    for key in mw.RESULT_KEYS:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key
    built = mw.build_fixture(name)  # (the batch generator is deterministic)
    assert built["movers"].tobytes() == fx["movers"].tobytes() and built["first"].tobytes() == fx["first"].tobytes()


@needs_reference
def test_the_prefix_property():
    """With maxIterations = m the planes are the first planes of the maxIterations = 8 answer"""
    fx = mw.load_fixture("synthetic")
    world = sq.fixture_world(fx)
    movers = fx["movers"][np.nonzero(fx["results"]["planeCount"] >= 2)[0][:24]].copy()
    movers["maxIterations"] = 8
    full_results, full_planes = ref.move_shapes(world, movers)
    for m in range(1, 8):
        movers["maxIterations"] = m
        results, planes = ref.move_shapes(world, movers)
        for i in range(len(movers)):
            k = results["planeCount"][i]
            assert k <= full_results["planeCount"][i] and planes[i, :k].tobytes() == full_planes[i, :k].tobytes(), (m, i)
            assert results["iterations"][i] == min(full_results["iterations"][i], m)
            if full_results["iterations"][i] <= m:
                assert results[i].tobytes() == full_results[i].tobytes()
            else:
                assert results["status"][i] == OUT


def _set_down(results):
    """The first frame that ends with the mover set down on something: the first with a plane"""
    return int(np.nonzero(results["planeCount"] >= 1)[0][0])


def test_the_walk():
    """The walk fixture (the statement's 300 frames of (0.05, -0.0027) from (0, 0.52), four iterations, each frame from where the last
    ended) against what a character needs of it.  The mover starts 15 mm above its resting height and 2.7 mm a frame bring it down,
    so "set down" is the first frame that records a plane."""
    fx = mw.load_walk_fixture()
    assert os.path.getsize(mw.fixture_path("walk")) <= max(os.path.getsize(sq.fixture_path(f)) for f in sq.FIXTURES)
    ramp_foot = mw.RAMP_CORNER[0] - 0.5  # (no walker reaches the ramp's face before its centre is here)
    for which in mw.WALKERS:
        floor, wall, ramp = (fx["%s_%s_results" % (kind, which)] for kind in mw.WALKS)
        assert len(floor) == len(wall) == len(ramp) == mw.FRAMES == 300
        for res in (floor, wall, ramp):
            assert (res["iterations"] <= 4).all() and res["position"][0][1] == f32(f32(0.52) + f32(-0.0027))
        # the open floor: 15 m, never CORNERED, never sinking
        assert floor["position"][-1][0] > 14.9 and (floor["status"] == REACHED).all()
        down = _set_down(floor)
        assert down <= 8 and floor["position"][down:, 1].min() >= floor["position"][down][1] - 5e-4
        assert (np.diff(floor["position"][:down + 1, 1]) < 0).all()
        # ... and the same on the ramp world's frames before the ramp: every frame the full 0.05
        before = ramp["position"][:, 0] < ramp_foot
        assert before[:80].all() and ramp[before].tobytes() == floor[before].tobytes()
        # the wall: at rest a skin before it (face 9.5 - half-width 0.25 - s2_linearSlop)
        assert abs(float(wall["position"][-1][0]) - 9.245) <= 1e-3 and (np.abs(wall["position"][200:, 0] - 9.245) <= 1e-3).all()
        assert (wall["status"][:150] == REACHED).all() and (wall["status"][200:] != REACHED).all()
        down = _set_down(wall)
        assert wall["position"][down:, 1].min() >= wall["position"][down][1] - 5e-4
        # the ramp: height gained
        assert ramp["position"][:, 1].max() > 2.0 and ramp["position"][-1][1] > 2.0 and (ramp["status"] != CORNERED).all()
        down = _set_down(ramp)
        assert ramp["position"][down:, 1].min() >= ramp["position"][down][1] - 5e-4
        for kind in mw.WALKS:
            res, planes = fx["%s_%s_results" % (kind, which)], fx["%s_%s_planes" % (kind, which)]
            assert (planes["shape"][np.arange(8)[None, :] < res["planeCount"][:, None]] <= 32).all()


@needs_reference
def test_the_walk_fixture_equals_the_statement_rerun_and_graze_is_why():
    fx = mw.load_walk_fixture()
    again = mw.build_walk_fixture()
    assert set(again) == set(fx)
    for key in fx:
        assert again[key].dtype == fx[key].dtype and again[key].tobytes() == fx[key].tobytes(), key
    # with GRAZE = 0 the box is CORNERED on the open floor before x = 5: this pins why the constant is there
    results, _ = mw.statement_walk("floor", "box", graze=0.0, frames=120)
    cornered = np.nonzero(results["status"] == CORNERED)[0]
    assert len(cornered) >= 1 and results["position"][cornered[0]][0] < 5.0, results["position"][-1]


def _least_sampled_distance(world, movers, samples=16):
    """Along every segment a mover travelled (from p by t * r, one per cast), the reference's distance to the candidates of that cast
    (step 2: without the shapes of recorded planes, the ignored body, the moving bodies under STATIC_ONLY) at `samples` evenly spaced
    fractions of the segment.  Exempt: the shapes within the threshold where the segment starts -- overlapping or touching, the winner
    at t = 0 and the shapes step 3 lets the mover leave or slide along.  -> the least distance seen, and how many were taken"""
    shapes, bodies, origins = world["shapes"], world["bodies"], world["origins"]
    least, taken = np.inf, 0
    for m in movers:
        path = []
        res, planes = ref.move(world, m, path=path)
        proxy_a = pref.make_proxy(m["vertices"], int(m["count"]), m["radius"])
        for b, (p, r, t) in enumerate(path):
            c = ref.cast_of(m, p, r)
            met = set(planes["shape"][:b].tolist())
            for slot in cref.candidates(world, c)[:12]:
                body = int(shapes["body"][slot])
                if int(slot) in met or body == int(m["ignoreBody"]) or (m["flags"] & 1 and bodies["type"][body] != wire.BODY_STATIC):
                    continue
                proxy_b, xf_b = pref.shape_proxy(shapes[slot]), pref.transform(origins[body], bodies["rot"][body])
                if f32(cref.distance_at(c, proxy_a, f32(0.0), proxy_b, xf_b).distance) < cref.THRESHOLD or t == 0:
                    continue
                for j in range(samples + 1):
                    d = cref.distance_at(c, proxy_a, f32(t * f32(j) / f32(samples)), proxy_b, xf_b)
                    least, taken = min(least, float(d.distance)), taken + 1
    return least, taken


@needs_reference
@pytest.mark.parametrize("name", mw.FIXTURES)
def test_the_statement_against_sampled_geometry(name):
    """Independent of the advancement loop and of the clip: no mover has passed through anything or come closer than the skin.  The
    bound is the shape casts' own test's: target - 1e-4."""
    fx = mw.load_fixture(name)
    movers = np.concatenate([fx["movers"][:48], fx["movers"][-mw.DIRECTED:]])
    least, taken = _least_sampled_distance(sq.fixture_world(fx), movers)
    print("%s: least sampled distance %.6f over %d samples" % (name, least, taken))
    assert taken >= 1000 and least >= float(cref.TARGET) - 1e-4, (least, taken)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch():
    """hipcc's own report for mover_query.hip (make resources-mover), through tools/kernel_resources.py: every kernel of the file is
    there, none has a private frame or a spill, and the candidates pass keeps four waves a SIMD beside its 40 KiB of LDS"""
    kernels = dict.fromkeys(("moverInitKernel", "moverCandidatesKernel", "moverAdvanceKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-mover", "resources_mover_query.txt", kernels, floor=4, every_row=True)
    asm = open(os.path.join(hostcheck_util.CSRC, "build", "asm_mover_query.s")).read()
    assert "atomic_umin_x2" in asm and not re.search(r"atomic_f?(add|min|max)_f", asm)  # the 64-bit integer minimum and no float atomic
