"""The grid report without a GPU: the interface as declared and bound with the header's sizes and offsets, the cell-point formula and
the box of the statement (tests/grid_report_ref.py), the statement against the scene queries' point probe, the fixtures
tests/golden/grid_report/*.npz with the condition every scene must meet, the compiler's resource report of the new kernels, and the
host side under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded)."""
import numpy as np
import pytest

from solver2d_amd import wire
from tests import grid_report_ref as ref, grid_report_world as gw, hostcheck_util, scene_query_ref, sensor_report_world as sw, world_chain

needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_set_grid_sensors", "s2amd_world_set_grid_report", "s2amd_world_grid_categories", "s2amd_world_grid_shapes",
         "s2amd_world_grid_occupancy", "s2amd_world_export_grid_occupancy", "s2amd_world_grid_states")
f32 = np.float32


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    fields = {"s2amdGridSensor": wire.grid_sensor_dtype, "s2amdGridState": wire.grid_state_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, fields)
    assert (wire.GRID_SENSOR_SIZE, wire.GRID_STATE_SIZE) == (64, 64)


def test_header_flags_and_bindings():
    defines = {"S2AMD_MAX_GRID_SENSORS": 1024, "S2AMD_MAX_GRID_SIDE": 256, "S2AMD_MAX_GRID_CELLS": 1048576, "S2AMD_GRID_SENSOR_DISABLED": 1,
               "S2AMD_GRID_SENSOR_SKIP_STATIC": 2, "S2AMD_GRID_REPORT_CATEGORIES": 1, "S2AMD_GRID_REPORT_SHAPES": 2, "S2AMD_GRID_REPORT_OCCUPANCY": 4,
               "S2AMD_GRID_REPORT_STATES": 8, "S2AMD_API_VERSION": 5}
    hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_GRID_SENSORS, wire.MAX_GRID_SIDE, wire.MAX_GRID_CELLS) == (1024, 256, 1048576)
    assert (wire.GRID_SENSOR_DISABLED, wire.GRID_SENSOR_SKIP_STATIC) == (1, 2)
    assert (wire.GRID_REPORT_CATEGORIES, wire.GRID_REPORT_SHAPES, wire.GRID_REPORT_OCCUPANCY, wire.GRID_REPORT_STATES, wire.GRID_REPORT_ALL) == (1, 2, 4, 8, 15)
    assert wire.API_VERSION == 5 and wire.RAY_REPORT_ALL == 7 and wire.MAX_RAY_SENSORS == 16384  # the other flag spaces and the API version are untouched


def test_cell_point_formula_by_hand():
    q = gw.make_grid((0.0, 0.0), 0.0, 0.25, 4, 2)
    x, y = ref.local_points(q)
    assert x.shape == (2, 4) and x[0].tolist() == [-0.375, -0.125, 0.125, 0.375] and y[:, 0].tolist() == [-0.125, 0.125]
    x, y = ref.local_points(gw.make_grid((0.0, 0.0), 0.0, 0.5, 7, 5))
    assert x[0].tolist() == [-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5] and y[:, 0].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    # everything in front of the multiply is exact for every width and every i < 256: float32 equals exact rational arithmetic
    for w in range(1, 257):
        i = np.arange(w)
        got = (i.astype(f32) + f32(0.5)) - f32(0.5) * f32(w)
        assert got.dtype == f32 and (got.astype(np.float64) == (2 * i + 1 - w) / 2.0).all(), w
    # a quarter turn: (x, y) -> (-y, x)
    X, Y = ref.transform_points((1.0, 2.0), (1.0, 0.0), f32([0.5]), f32([-0.25]))
    assert (X[0], Y[0]) == (f32(1.25), f32(2.5)) and X.dtype == f32


def test_box_contains_every_cell_point():
    """200 random frames at 256 x 256: the box of the four corner cells contains every cell's P"""
    rng = np.random.RandomState(7)
    world = {"bodies": np.zeros(0, dtype=wire.body_dtype), "origins": np.zeros((0, 2), dtype=f32)}
    for k in range(200):
        angle = rng.rand() * 6.2832 if k % 4 else (k % 16) * np.pi / 8
        scale = 10.0 ** rng.uniform(-3, 3)
        q = gw.make_grid(tuple(rng.uniform(-1, 1, 2) * scale * (1000.0 if k % 3 == 0 else 1.0)), angle, 10.0 ** rng.uniform(-3, 1), 256, 256)
        if k % 5 == 0:
            q["rot"] = f32(q["rot"]) * f32(rng.uniform(0.5, 2.0))  # rot is not checked for normalisation
        active, _, _, X, Y, box = ref.cell_points(world, q)
        assert active
        assert X.min() >= box[0] and Y.min() >= box[1] and X.max() <= box[2] and Y.max() <= box[3], (k, box)


def test_inactive_frames():
    world, grids = gw.scene("ball")
    mounted = grids[1]
    assert not ref.cell_points(world, grids[4])[0]  # DISABLED
    assert ref.cell_points(world, mounted)[0]
    for body in (2, len(world["bodies"])):  # a free body slot; outside the array
        q = mounted.copy()
        q["body"] = body
        assert not ref.cell_points(world, q)[0]
    world["origins"][1] = (np.nan, 0.0)
    assert not ref.cell_points(world, mounted)[0] and ref.cell_points(world, grids[0])[0]
    first, total = ref.first_cells(grids)
    assert first.tolist() == [0, 256, 512, 768, 1024, 1280, 1315, 1316] and total == 1572


@needs_reference
@pytest.mark.parametrize("scene", gw.SCENES)
def test_without_exclusions_the_statement_is_the_point_probe_folded(scene):
    """With exclusions=False the statement equals tests/scene_query_ref.point_probe of its own cell points folded with OR and min, on
    the scene's first, fourth and last state of the chain; the recorded "plain" images are these"""
    fx = gw.load_fixture(scene)
    world, grids, params = gw.fixture_world(fx), fx["grids"], sw.params()
    for k in range(gw.STEPS + 1):
        if k in (0, 4, gw.STEPS):
            cats, low, occ, states = ref.report(world, grids, exclusions=False)
            points, index = ref.probes_of(world, grids)
            offsets, flat = scene_query_ref.point_probe(world, points)
            pc, pl, po = ref.fold_probe(world, len(cats), index, offsets, flat)
            assert cats.tobytes() == pc.tobytes() and low.tobytes() == pl.tobytes() and occ.tobytes() == po.tobytes(), (scene, k)
            assert states["occupied"].sum() == (pl >= 0).sum()
            if k > 0:
                assert fx["plain_%d" % (k - 1)].tobytes() == low.tobytes(), (scene, k)
        if k < gw.STEPS:
            world_chain.oracle_world_step(params, world)


@needs_reference
@pytest.mark.parametrize("scene", gw.SCENES)
def test_recorded_fixtures_equal_the_statement(scene):
    fx = gw.load_fixture(scene)
    built = gw.build_fixture(scene)  # (asserts the condition on the way)
    assert sorted(built) == sorted(fx)
    for key in built:
        assert np.ascontiguousarray(built[key]).tobytes() == fx[key].tobytes(), (scene, key)


@pytest.mark.parametrize("scene", gw.SCENES)
def test_every_scene_meets_the_condition(scene):
    """From the fixture alone: per step at least 95 % of the cells of the active grids are robust, every active grid of more than one
    cell has a robust cell, every name of grid_report_world.COVERAGE occurs among robust cells; the grids are the eight kinds the
    scenes promise and the images have the structure every report has"""
    fx = gw.load_fixture(scene)
    gw.assert_condition(fx, scene)
    share, bare, missing = gw.condition(fx)
    assert share >= 0.95 and bare == [] and missing == []
    grids = fx["grids"]
    first, total = ref.first_cells(grids)
    assert (grids["width"] * grids["height"]).tolist() == [256, 256, 256, 256, 256, 35, 1, 256] and total == 1572
    assert (grids["body"] >= 0).sum() == 2 and ((grids["flags"] & wire.GRID_SENSOR_DISABLED) != 0).tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert ((grids["flags"] & wire.GRID_SENSOR_SKIP_STATIC) != 0).tolist() == [0, 0, 1, 1, 0, 0, 0, 0] and grids["maskBits"][7] == gw.SOME
    assert len(set(fx["shapes"]["categoryBits"][fx["shapes"]["type"] != wire.SHAPE_FREE].tolist())) >= 3
    own, static = int(grids[1]["body"]), fx["bodies"]["type"] == wire.BODY_STATIC
    for k in range(gw.STEPS):
        low, cats = gw.images(grids, fx["shapes_%d" % k]), gw.images(grids, fx["categories_%d" % k])
        assert fx["active_%d" % k].tolist() == [1, 1, 1, 1, 0, 1, 1, 1] and len(fx["robust_%d" % k]) == total
        assert (low[4] == -1).all() and (cats[4] == 0).all()  # DISABLED
        assert all(fx["shapes"]["body"][m] != own for m in low[1][low[1] >= 0])  # never its own body
        for g in (2, 3):
            assert not static[fx["shapes"]["body"][low[g][low[g] >= 0]]].any()  # SKIP_STATIC
        assert ((cats[7] & ~np.uint32(gw.SOME)) == 0).all()  # the mask


def test_displacements_are_what_they_say():
    grids = np.array([gw.make_grid((1.0, 2.0), 0.0, 0.25, 4, 4), gw.make_grid((1.0, 2.0), np.pi / 2, 0.25, 4, 4, body=3)], dtype=wire.grid_sensor_dtype)
    right, left, up, down = gw.variations(grids)
    assert np.allclose(right["position"], [(1.001, 2.0), (1.0, 2.001)], atol=1e-6) and np.allclose(left["position"], [(0.999, 2.0), (1.0, 1.999)], atol=1e-6)
    assert np.allclose(up["position"], [(1.0, 2.001), (0.999, 2.0)], atol=1e-6) and np.allclose(down["position"], [(1.0, 1.999), (1.001, 2.0)], atol=1e-6)
    for v in (right, left, up, down):
        assert v["rot"].tobytes() == grids["rot"].tobytes() and v["body"].tolist() == [-1, 3]


def test_kernels_use_no_scratch():
    """hipcc's own report for grid_report.hip (make resources-grid-report), through tools/kernel_resources.py: every kernel of the file is
    there, none has a private frame or spills"""
    kernels = dict.fromkeys(("gridPoseKernel", "gridCandidatesKernel", "gridRasterKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-grid-report", "resources_grid_report.txt", kernels, floor=4, every_row=True)


@hostcheck_util.needs_sanitizers
def test_grid_report_host_code_under_asan_and_ubsan(tmp_path):
    """The setter with good and bad lists -> every flag combination 0..15 -> every getter (the device export among them) with too-small,
    exact and ample heap buffers of exactly the size passed -> the list replaced and cleared between steps -> uploads with other
    capacities, worlds without shape slots among them -> destroy, for 0, 1, 257 and 1,024 grids, a list at exactly S2AMD_MAX_GRID_CELLS
    and one a cell over, on the sanitizer build of tests/test_hostcheck.py (kernels never run there: what is checked is that the host
    code touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "grid_report_main.cpp", "GRID REPORT MAIN OK", timeout=600)
