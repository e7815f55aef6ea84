"""The shape report without a GPU: the two new structs of include/solver2d_amd.h have the sizes and field offsets of their wire dtypes,
the reference statement the GPU tests compare against (tests/shape_report_ref.py) gives, on a world small enough to work out by hand,
the values written out here, the synthetic world of the GPU test has on the CPU oracle chain the events the GPU test needs, and the host
side of the report runs clean under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing
preloaded)."""
import os

import numpy as np

from solver2d_amd import hip, wire
from tests import common, hostcheck_util, shape_report_ref as ref, shape_report_world, world_chain

f32 = np.float32
INF = float("inf")


def test_shape_report_struct_sizes_and_offsets_match_header(tmp_path):
    fields = {"s2amdShapeDraw": wire.shape_draw_dtype, "s2amdShapeSummary": wire.shape_summary_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, fields)
    assert (wire.shape_draw_dtype.itemsize, wire.shape_summary_dtype.itemsize) == (128, 64)
    assert wire.shape_draw_dtype.fields["vertices"][1] == 32 and wire.shape_draw_dtype.fields["aabb"][1] == 96
    assert wire.shape_summary_dtype.fields["movableBounds"][1] == 32


def test_shape_report_exports_and_flags():
    names = ("s2amd_world_set_shape_report", "s2amd_world_set_shape_view", "s2amd_world_shape_draws", "s2amd_world_shape_view_events",
             "s2amd_world_shape_summary")
    assert (wire.SHAPE_REPORT_DRAW, wire.SHAPE_REPORT_VIEW, wire.SHAPE_REPORT_BOUNDS, wire.SHAPE_REPORT_ALL) == (1, 2, 4, 7)
    assert wire.REPORT_ALL == 7 and wire.JOINT_REPORT_ALL == 7 and wire.API_VERSION == 5  # the other flag spaces and the API version are untouched
    hostcheck_util.assert_header_and_bindings(names, {"S2AMD_SHAPE_REPORT_DRAW": 1, "S2AMD_SHAPE_REPORT_VIEW": 2, "S2AMD_SHAPE_REPORT_BOUNDS": 4})
    if os.path.exists(hip.LIB_PATH):
        # (the built library: every function is there to be called)
        lib = hip.load()
        for name in names:
            assert getattr(lib, name) is not None


VIEW = (-3.4, -5.0, 9.0, 1.75)


def six_slot_world():
    """Bodies 0 static, 1 kinematic, 2 dynamic, 3 dynamic without mass (a bad body), all turned by a quarter (s = 1, c = 0):
    s2TransformPoint gives x = (0 * px - 1 * py) + ox, y = (1 * px + 0 * py) + oy.  Slot 0 a rounded triangle on body 0, slot 1 free,
    slot 2 a circle on body 1, slot 3 a capsule on body 2, slot 4 a segment on body 3, slot 5 a box on body 2 whose aabb holds a NaN.
    Every number is a small dyadic fraction: the float32 results are exact."""
    bodies = np.zeros(4, dtype=wire.body_dtype)
    bodies["type"] = [wire.BODY_STATIC, wire.BODY_KINEMATIC, wire.BODY_DYNAMIC, wire.BODY_DYNAMIC]
    bodies["rot"] = (1.0, 0.0)
    bodies["mass"] = [0.0, 0.0, 2.0, 0.0]
    origins = np.array([(1.0, 2.0), (-3.0, 0.5), (0.0, 0.0), (10.0, -4.0)], dtype=np.float32)
    shapes = np.zeros(6, dtype=wire.shape_dtype)
    shapes["vertices"] = 9.0  # junk beyond every count
    shapes["normals"] = 7.0   # the report never reads them
    shapes["body"] = [0, -1, 1, 2, 3, 2]
    shapes["type"] = [wire.SHAPE_POLYGON, wire.SHAPE_FREE, wire.SHAPE_CIRCLE, wire.SHAPE_CAPSULE, wire.SHAPE_SEGMENT, wire.SHAPE_POLYGON]
    shapes["count"] = [3, 8, 1, 2, 2, 4]
    shapes["radius"] = [0.25, 5.0, 0.5, 0.25, 0.0, 0.0]
    shapes["vertices"][0, :3] = [(0.0, 0.0), (2.0, 0.0), (0.0, 1.0)]
    shapes["vertices"][2, :1] = [(0.5, 1.0)]
    shapes["vertices"][3, :2] = [(-1.0, 0.0), (1.0, 0.0)]
    shapes["vertices"][4, :2] = [(2.0, 1.0), (4.0, -1.0)]
    shapes["vertices"][5, :4] = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
    shapes["aabb"] = [(-0.25, 1.75, 1.25, 4.25), (0.0, 0.0, 0.0, 0.0), (-4.5, 0.5, -3.5, 1.5), (-0.25, -1.25, 0.25, 1.25), (9.0, -2.0, 11.0, 0.0),
                      (np.nan, 0.0, 1.0, 1.0)]
    shapes["fatAABB"] = shapes["aabb"] + np.array([-0.125, -0.125, 0.125, 0.125], dtype=np.float32)
    return {"bodies": bodies, "contacts": np.zeros(0, dtype=wire.contact_dtype), "joints": np.zeros(0, dtype=wire.joint_dtype), "shapes": shapes,
            "pairs": np.zeros(0, dtype=wire.pair_state_dtype), "origins": origins}


def test_reference_statement_on_a_hand_written_world():
    w = six_slot_world()
    # slot 0 touches the view's upper edge (1.75 - 1.75 = 0), slot 4 its right edge (9 - 9 = 0): a difference of 0 is in view;
    # slot 2 ends 0.1 left of it; slot 5's NaN makes no difference > 0
    assert ref.in_view(w, VIEW).tolist() == [True, False, False, True, True, True]
    assert ref.in_view(w, None).tolist() == [True, False, True, True, True, True]
    d = ref.draws(w, VIEW)
    assert d.dtype == wire.shape_draw_dtype and d["shape"].tolist() == [0, 3, 4, 5]
    assert d["body"].tolist() == [0, 2, 3, 2] and d["type"].tolist() == [2, 0, 3, 2]
    assert d["vertexCount"].tolist() == [3, 2, 2, 4]
    assert d["bodyClass"].tolist() == [0, 2, 3, 2]
    assert d["radius"].tolist() == [0.25, 0.25, 0.0, 0.0]
    assert d["axis"].tolist() == [[0.0, 1.0]] * 4  # {c * 1 - s * 0, s * 1 + c * 0}
    zeros = [0.0, 0.0]
    # slot 0 on body 0 at (1, 2): (-0 + 1, 0 + 2), (-0 + 1, 2 + 2), (-1 + 1, 0 + 2)
    assert d["vertices"][0].tolist() == [[1.0, 2.0], [1.0, 4.0], [0.0, 2.0]] + [zeros] * 5
    # slot 3 on body 2 at the origin: (-0 + 0, -1 + 0), (-0 + 0, 1 + 0)
    assert d["vertices"][1].tolist() == [[0.0, -1.0], [0.0, 1.0]] + [zeros] * 6
    # slot 4 on body 3 at (10, -4): (-1 + 10, 2 - 4), (1 + 10, 4 - 4)
    assert d["vertices"][2].tolist() == [[9.0, -2.0], [11.0, 0.0]] + [zeros] * 6
    # slot 5 on body 2: (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5)
    assert d["vertices"][3].tolist() == [[0.5, -0.5], [0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5]] + [zeros] * 4
    for row in range(4):
        used = int(d["vertexCount"][row])
        assert d["vertices"][row, used:].tobytes() == bytes(8 * (8 - used))  # +0, not -0 and not the junk
    assert d["aabb"].tobytes() == w["shapes"]["aabb"][[0, 3, 4, 5]].tobytes()
    assert d["fatAABB"].tobytes() == w["shapes"]["fatAABB"][[0, 3, 4, 5]].tobytes()
    everything = ref.draws(w, None)
    assert everything["shape"].tolist() == [0, 2, 3, 4, 5] and everything["bodyClass"].tolist() == [0, 1, 2, 3, 2]
    # the circle on body 1 at (-3, 0.5): (-1 - 3, 0.5 + 0.5)
    assert everything["vertices"][1].tolist() == [[-4.0, 1.0]] + [zeros] * 7 and int(everything["vertexCount"][1]) == 1

    entered, left = ref.events(np.zeros(6, dtype=bool), w, VIEW)
    assert entered.tolist() == [0, 3, 4, 5] and left.tolist() == [] and entered.dtype == np.int32
    entered, left = ref.events([True, True, True, False, True, True], w, VIEW)
    assert entered.tolist() == [3] and left.tolist() == [1, 2]
    entered, left = ref.events(ref.in_view(w, VIEW), w, VIEW)
    assert entered.tolist() == [] and left.tolist() == []

    m = ref.summary(w, VIEW)
    assert m.dtype == wire.shape_summary_dtype
    assert (int(m["liveShapes"]), int(m["inView"]), int(m["badBodyShapes"]), int(m["pad"])) == (5, 4, 1, 0)
    assert m["byType"].tolist() == [1, 1, 2, 1]  # capsule, circle, polygon, segment
    # over slots 2, 3, 4, 5 (the static body's slot 0 is not movable); the NaN never wins
    assert m["movableBounds"].tolist() == [-4.5, -2.0, 11.0, 1.5]
    # over slots 0, 3, 4, 5
    assert m["viewBounds"].tolist() == [-0.25, -2.0, 11.0, 4.25]
    m = ref.summary(w, None)
    assert int(m["inView"]) == 5 and m["viewBounds"].tolist() == [-4.5, -2.0, 11.0, 4.25]
    # nothing qualifies: the start value is the answer
    w["shapes"]["type"] = wire.SHAPE_FREE
    m = ref.summary(w, VIEW)
    assert m["movableBounds"].tolist() == [INF, INF, -INF, -INF] and m["viewBounds"].tolist() == [INF, INF, -INF, -INF]
    assert int(m["liveShapes"]) == 0 and len(ref.draws(w, VIEW)) == 0


def test_synthetic_world_has_the_events_the_gpu_test_needs():
    """The oracle chain in pool order, stated by the reference alone: what keeps tests/test_gpu_shape_report.py from passing on nothing."""
    world = shape_report_world.synthetic_world()
    shape_report_world.assert_world_is_what_it_says(world)
    view = shape_report_world.VIEW
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, vel, pos, True)
    prev = ref.in_view(world, view)
    assert 0 < int(prev.sum()) < int((world["shapes"]["type"] != wire.SHAPE_FREE).sum())
    assert any(int(prev[t:t + 256].sum()) % 64 != 0 for t in (0, 256))
    entered_all, left_all, both = [], [], 0
    bounds = [ref.summary(world, view)["movableBounds"].tobytes()]
    for _ in range(12):
        world_chain.oracle_world_step(params, world)
        entered, left = ref.events(prev, world, view)
        entered_all += entered.tolist()
        left_all += left.tolist()
        both += 1 if len(entered) and len(left) else 0
        prev = ref.in_view(world, view)
        bounds.append(ref.summary(world, view)["movableBounds"].tobytes())
    assert len(entered_all) >= 8 and len(left_all) >= 8, (len(entered_all), len(left_all))
    events = entered_all + left_all
    assert any(e < 256 for e in events) and any(e >= 256 for e in events)
    assert both >= 1
    assert all(a != b for a, b in zip(bounds, bounds[1:]))
    assert any(int(prev[t:t + 256].sum()) % 64 != 0 for t in (0, 256))
    assert np.isfinite(world["bodies"]["position"]).all()


@hostcheck_util.needs_sanitizers
def test_shape_report_host_code_under_asan_and_ubsan(tmp_path):
    """tests/hostcheck/shape_report_main.cpp, a program of its own: upload -> every flag combination -> a view set, changed and cleared ->
    every getter with too-small, exact and ample buffers -> uploads with other capacities -> destroy, on the sanitizer build of
    tests/test_hostcheck.py (kernels never run there: what is checked is that the host code touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "shape_report_main.cpp", "SHAPE REPORT MAIN OK", timeout=600)
