"""The grid report of the resident world (s2amd_world_set_grid_sensors / _set_grid_report / _grid_categories / _grid_shapes /
_grid_occupancy / _export_grid_occupancy / _grid_states; solver2d_amd/csrc/grid_report.hip) against its statement
(tests/grid_report_ref.py), byte for byte: the recorded images of tests/golden/grid_report on their robust cells with the world stepped
beside the oracle chain of tests/world_chain.py in the device's orders, the statement itself on every step of every test where the
reference library is built, and always the device's own s2amd_world_point_probe of the statement's cell points, folded with OR and
min, for every grid whose two exclusions remove nothing."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import grid_report_ref as ref, grid_report_world as gw, sensor_report_world as sw, world_chain
from tests.grid_report_world import assert_probe, assert_report, assert_statement, assert_structure, getters
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, downloaded_world, refuses, step_both, upload

pytestmark = pytest.mark.gpu

ALL = wire.GRID_REPORT_ALL
DISABLED, SKIP_STATIC = wire.GRID_SENSOR_DISABLED, wire.GRID_SENSOR_SKIP_STATIC
GETTERS = {wire.GRID_REPORT_CATEGORIES: "world_grid_categories", wire.GRID_REPORT_SHAPES: "world_grid_shapes",
           wire.GRID_REPORT_OCCUPANCY: "world_grid_occupancy", wire.GRID_REPORT_STATES: "world_grid_states"}


@pytest.mark.parametrize("scene,fast", [(scene, fast) for scene in gw.SCENES for fast in (False, True)])
def test_recorded_scenes_every_step(scene, fast):
    """The three scenes of tests/golden/grid_report for STEPS steps in both libraries, the world stepped beside the oracle chain in the
    device's orders: every step the robust cells of SHAPES and CATEGORIES against the fixture -- whatever the state of the reference
    library --, the structure, the device's point probe, and every cell of every array and the states against the live statement on
    the oracle chain's world (libs2amd.so: its resident bytes are the chain's) or on the resident bytes (the tolerance mode)"""
    fx = gw.load_fixture(scene)
    world, grids, params = gw.fixture_world(fx), fx["grids"], sw.params()
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0, fast=fast) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        refuses(s, E_STATE, GETTERS.values())
        for k in range(gw.STEPS):
            step_both(s, params, ref_world)
            what = "%s step %d" % (scene, k)
            resident = downloaded_world(s, world)
            got = getters(s)
            assert_structure(resident, grids, got, what)
            assert_probe(s, resident, grids, got, what)
            assert_statement(resident if fast else ref_world, grids, got, what)
            robust = fx["robust_%d" % k] != 0
            assert got[1][robust].tolist() == fx["shapes_%d" % k][robust].tolist(), what
            assert got[0][robust].tolist() == fx["categories_%d" % k][robust].tolist(), what
            assert got[3]["active"].tolist() == fx["active_%d" % k].tolist(), what
        if not fast:
            for key in world_chain.WORLD_KEYS:
                assert resident[key].tobytes() == ref_world[key].tobytes(), (scene, key)


@pytest.mark.parametrize("flags", [1, 2, 4, 8, 15])
def test_each_flag_alone_and_all(flags):
    world, grids = gw.scene("pyramid")
    params = sw.params()
    with hip.Solver(0) as s, hip.Solver(0) as full:
        for solver, f in ((s, flags), (full, ALL)):
            solver.world_set_grid_sensors(grids)
            solver.world_set_grid_report(f)
            upload(solver, world)
            solver.world_step(params)
        want = dict(zip(GETTERS.values(), getters(full)))
        for flag, name in GETTERS.items():
            if flags & flag:
                assert getattr(s, name)().tobytes() == want[name].tobytes(), name
            else:
                refuses(s, E_STATE, (name,))
        if not flags & wire.GRID_REPORT_OCCUPANCY:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_export_grid_occupancy(0, 0)
        s.world_set_grid_report(0)
        s.world_step(params)
        refuses(s, E_STATE, GETTERS.values())


def test_capacity_protocol_and_export():
    """Through the raw C calls with buffers of exactly the stated sizes: asked one entry short first, which must state the count and
    touch nothing; the export's bytes are the host getter's"""
    world, grids = gw.scene("ball")
    params = sw.params()
    first, cells = ref.first_cells(grids)
    with hip.Solver(0) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        room = cells + 3
        buf = s.device_alloc(4 * room)
        try:
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_export_grid_occupancy(buf, room)  # no step since the upload
            for _ in range(3):
                s.world_step(params)
            L, h = s._L, s._h
            n = ctypes.c_int32(-7)
            for fn, dtype, count, name in ((L.s2amd_world_grid_categories, np.uint32, cells, "world_grid_categories"), (L.s2amd_world_grid_shapes, np.int32, cells, "world_grid_shapes"),
                                           (L.s2amd_world_grid_occupancy, np.float32, cells, "world_grid_occupancy"),
                                           (L.s2amd_world_grid_states, wire.grid_state_dtype, len(grids), "world_grid_states")):
                out = np.zeros(count, dtype=dtype)
                out.view(np.uint8)[:] = 0xAB
                assert (fn(h, wire.as_ptr(out), count - 1, ctypes.byref(n)), n.value) == (E_CAPACITY, count), name
                assert (out.view(np.uint8) == 0xAB).all(), name
                assert fn(h, wire.as_ptr(out), -1, ctypes.byref(n)) == E_INVALID
                assert (fn(h, wire.as_ptr(out), count, ctypes.byref(n)), n.value) == (0, count), name
                assert out.tobytes() == getattr(s, name)().tobytes(), name
            with pytest.raises(hip.S2AmdError, match="error %d" % E_CAPACITY):
                s.world_export_grid_occupancy(buf, cells - 1)
            s.world_export_grid_occupancy(buf, room)
            got = s.device_read(buf, (room,), np.float32)
            occ = s.world_grid_occupancy()
            assert got[:cells].tobytes() == occ.tobytes() and got[cells:].tobytes() == bytes(12) and occ.sum() >= 3
            s.world_set_grid_report(wire.GRID_REPORT_STATES)
            s.world_step(params)
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                s.world_export_grid_occupancy(buf, room)  # its flag was not set before the step
        finally:
            s.device_free(buf)


@pytest.mark.parametrize("slots", [1, 63, 64, 65, 255, 256, 257, 600])
def test_shape_capacities_at_which_a_path_changes(slots):
    """The mask's words and tiles: 1 .. 600 shape slots under the seven distinct grids of grid_report_world.sweep_grids, three steps"""
    world = sw.sweep_world(slots)
    grids = gw.sweep_grids(world, 7)
    params = sw.params()
    with hip.Solver(0) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        for k in range(3):
            s.world_step(params)
            got = assert_report(s, world, grids, "%d slots step %d" % (slots, k))
        assert slots < 63 or got[3]["occupied"].sum() > 0


@pytest.mark.parametrize("count", [1, 64, 65, 256, 257, 1024])
def test_grid_counts_at_which_a_path_changes(count):
    """A tiled list of 1 .. 1,024 grids (the pose pass's workgroups, the candidates pass's chunks of 256) over 300 shape slots,
    compared with the statement on one period of the tiling"""
    world = sw.sweep_world(300)
    grids = gw.sweep_grids(world, count)
    params = sw.params()
    with hip.Solver(0) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        s.world_step(params)
        s.world_step(params)
        got = assert_report(s, world, grids, "%d grids" % count, period=7)
        # every period answers alike
        period = ref.first_cells(grids[:7])[1]
        if count >= 14:
            assert got[1][:period].tobytes() == got[1][period: 2 * period].tobytes()


def test_grid_shapes_at_tile_edges():
    """1 x 1, 1 x 256, 256 x 1, 8 x 8, 17 x 16 (272 cells, across a tile of 256), 65 x 3 and 7 x 5 in one list: extents that end inside an
    8 x 8 block of cells in x, in y and in both"""
    world = sw.sweep_world(300)
    grids = gw.edge_grids()
    params = sw.params()
    with hip.Solver(0) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        for k in range(2):
            s.world_step(params)
            got = assert_report(s, world, grids, "edge grids step %d" % k)
        assert (got[3]["occupied"] > 0).sum() >= 4


def test_one_256_by_256_grid_is_the_point_probe():
    """65,536 cells over sweep_world(600): the device's own point probe of the statement's cell points on the same solver, folded with
    OR and min in numpy, equals the report's arrays"""
    world = sw.sweep_world(600)
    grids = np.array([gw.make_grid((3.75, 9.0), 0.3, 0.0625, 256, 256)], dtype=wire.grid_sensor_dtype)
    params = sw.params()
    with hip.Solver(0) as s:
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        s.world_step(params)
        got = assert_report(s, world, grids, "256 x 256", statement=False)
        assert got[3]["occupied"][0] > 500 and got[3]["candidates"][0] > 300 and len(set(got[1].tolist())) > 200


def test_inactive_grids_leave_the_others_alone():
    """A grid on a free body slot, on a body beyond bodyCapacity after a smaller upload, and on a body whose pose was made NaN:
    inactive, and the other grids' answers are unchanged"""
    world, grids = gw.scene("ball")
    params = sw.params()
    first, _ = ref.first_cells(grids)
    on_free = grids[1].copy()
    on_free["body"] = 2  # the scene's free body slot
    with hip.Solver(0) as s:
        s.world_set_grid_report(ALL)
        s.world_set_grid_sensors(grids)
        upload(s, world)
        s.world_step(params)
        base = getters(s)
        both = np.concatenate([grids, np.array([on_free], dtype=wire.grid_sensor_dtype)])
        upload(s, world)
        s.world_set_grid_sensors(both)
        refuses(s, E_STATE, GETTERS.values())
        s.world_step(params)
        got = assert_report(s, world, both, "free body")
        assert got[3]["active"][-1] == 0 and got[1][: len(base[1])].tobytes() == base[1].tobytes() and got[0][: len(base[0])].tobytes() == base[0].tobytes()
        # a NaN pose switches the mounted grids off
        broken = world_chain.copy_world(world)
        broken["origins"][1] = (np.nan, 0.0)
        broken["bodies"]["position"][1] = (np.nan, 0.0)
        broken["bodies"]["linearVelocity"][1] = 0.0
        fixed_only = np.array([g for g in grids if g["body"] != 1], dtype=wire.grid_sensor_dtype)
        with hip.Solver(0) as t:
            t.world_set_grid_report(ALL)
            t.world_set_grid_sensors(fixed_only)
            upload(t, broken)
            t.world_step(params)
            want = getters(t)
        upload(s, broken)
        s.world_set_grid_sensors(grids)
        s.world_step(params)
        cats, low, occ, states = getters(s)
        mounted = np.flatnonzero(grids["body"] == 1)
        assert len(mounted) >= 1 and (states["active"][mounted] == 0).all()
        keep = np.concatenate([first[g] + np.arange(int(grids[g]["width"]) * int(grids[g]["height"])) for g in range(len(grids)) if grids[g]["body"] != 1])
        assert low[keep].tobytes() == want[1].tobytes() and cats[keep].tobytes() == want[0].tobytes()
        for g in mounted:
            assert (low[first[g]: first[g] + states["cells"][g]] == -1).all()
        # a smaller world: the list holds, a grid whose body is outside the new body array is inactive there
        small = sw.sweep_world(20)
        far = grids[0].copy()
        far["body"] = len(small["bodies"]) + 5
        big = sw.sweep_world(64)
        upload(s, big)
        s.world_set_grid_sensors(np.array([grids[0], far], dtype=wire.grid_sensor_dtype))
        upload(s, small)
        s.world_step(params)
        states = s.world_grid_states()
        assert states["active"].tolist() == [1, 0]


def test_list_replaced_cleared_and_voided():
    world, grids = gw.scene("pyramid")
    params = sw.params()
    with hip.Solver(0) as s:
        refuses(s, E_STATE, GETTERS.values())  # no world
        for bad in (16, -1):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_grid_report(bad)
        s.world_set_grid_sensors(grids)
        s.world_set_grid_report(ALL)
        upload(s, world)
        s.world_step(params)
        first = assert_report(s, world, grids, "first")
        # refusals leave the old list answering
        for field, value in (("width", 0), ("width", 257), ("height", 0), ("height", 257), ("cellSize", 0.0), ("cellSize", -1.0), ("cellSize", np.nan),
                             ("cellSize", np.inf), ("position", (np.nan, 0.0)), ("rot", (0.0, np.inf)), ("flags", 4), ("body", len(world["bodies"]))):
            wrong = grids.copy()
            wrong[1][field] = value
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_grid_sensors(wrong)
        too_many = np.array([gw.make_grid((0.0, 0.0), 0.0, 0.1, 256, 256)] * 17, dtype=wire.grid_sensor_dtype)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
            s.world_set_grid_sensors(too_many)
        assert s.world_grid_shapes().tobytes() == first[1].tobytes()  # not voided by a refusal
        s.world_step(params)
        assert_report(s, world, grids, "after refusals")
        # replaced: void until the next step
        reversed_list = np.ascontiguousarray(grids[::-1])
        s.world_set_grid_sensors(reversed_list)
        refuses(s, E_STATE, GETTERS.values())
        s.world_step(params)
        assert_report(s, world, reversed_list, "reversed")
        # cleared
        s.world_set_grid_sensors(np.zeros(0, dtype=wire.grid_sensor_dtype))
        refuses(s, E_STATE, GETTERS.values())
        s.world_step(params)
        assert [len(x) for x in getters(s)] == [0, 0, 0, 0]
        s.world_set_grid_sensors(grids)
        s.world_step(params)
        assert_report(s, world, grids, "set again")
        # turning on and an upload void
        s.world_set_grid_report(0)
        s.world_set_grid_report(ALL)
        refuses(s, E_STATE, GETTERS.values())
        s.world_step(params)
        upload(s, world)
        refuses(s, E_STATE, GETTERS.values())


def test_the_report_writes_nothing_resident():
    """world_download after STEPS steps with every flag on equals the same chain with the report off, byte for byte"""
    world, grids = gw.scene("pyramid")
    params = sw.params()
    out = []
    for flags in (ALL, 0):
        with hip.Solver(0) as s:
            s.world_set_grid_sensors(grids)
            s.world_set_grid_report(flags)
            upload(s, world)
            for _ in range(gw.STEPS):
                s.world_step(params)
            if flags == 0:
                refuses(s, E_STATE, GETTERS.values())
            out.append(downloaded_world(s, world))
    for key in world_chain.WORLD_KEYS:
        assert out[0][key].tobytes() == out[1][key].tobytes(), key
