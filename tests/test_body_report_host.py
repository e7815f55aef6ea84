"""The body report without a GPU: the three new structs of include/solver2d_amd.h have the sizes and field offsets of their wire dtypes,
the reference statement the GPU tests compare against (tests/body_report_ref.py) gives, on a world small enough to work out by hand,
the values written out here, the synthetic world of the GPU test has on the CPU oracle chain the events the GPU test needs, and the host
side of the report runs clean under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing
preloaded)."""
import os

import numpy as np

from solver2d_amd import hip, islands, wire
from tests import body_report_ref as ref, body_report_world, common, hostcheck_util, world_chain

f32 = np.float32
NAN = float("nan")


def test_body_report_struct_sizes_and_offsets_match_header(tmp_path):
    fields = {"s2amdBodyState": wire.body_state_dtype, "s2amdIslandState": wire.island_state_dtype, "s2amdBodySummary": wire.body_summary_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, fields)
    assert (wire.body_state_dtype.itemsize, wire.island_state_dtype.itemsize, wire.body_summary_dtype.itemsize) == (64, 32, 64)
    assert wire.body_state_dtype.fields["origin"][1] == 16 and wire.body_state_dtype.fields["restTime"][1] == 56
    assert wire.island_state_dtype.fields["maxSpeedSquared"][1] == 24 and wire.body_summary_dtype.fields["pad"][1] == 44


def test_body_report_exports_and_flags():
    names = ("s2amd_world_set_body_report", "s2amd_world_set_rest_thresholds", "s2amd_world_body_states", "s2amd_world_body_rest_events",
             "s2amd_world_islands", "s2amd_world_body_summary")
    assert (wire.BODY_REPORT_STATES, wire.BODY_REPORT_REST, wire.BODY_REPORT_ISLANDS, wire.BODY_REPORT_MOVED_ONLY, wire.BODY_REPORT_ALL) == (1, 2, 4, 8, 15)
    # the other three flag spaces and the API version are untouched
    assert wire.REPORT_ALL == 7 and wire.JOINT_REPORT_ALL == 7 and wire.SHAPE_REPORT_ALL == 7 and wire.API_VERSION == 5
    hostcheck_util.assert_header_and_bindings(names, {"S2AMD_BODY_REPORT_STATES": 1, "S2AMD_BODY_REPORT_REST": 2, "S2AMD_BODY_REPORT_ISLANDS": 4,
                                                      "S2AMD_BODY_REPORT_MOVED_ONLY": 8, "S2AMD_API_VERSION": 5})
    if os.path.exists(hip.LIB_PATH):
        # (the built library: every function is there to be called)
        lib = hip.load()
        for name in names:
            assert getattr(lib, name) is not None


THRESHOLDS = (0.5, 1.0, 0.5)  # lin2 = 0.25, ang2 = 1
DT = 0.25


def thirteen_slot_world():
    """Slot 0 static, 1 kinematic, 8 dynamic without mass, 9 free, the rest dynamic with unit mass.  Revolute joints: 0-2, 2-3 and 0-4 (two
    chains from the static body), 1-5, 5-6 and 1-7 (two from the kinematic one), 3-8 and 8-4 (the massless body between two chains);
    mouse joints on 10 and on 2.  Contacts: 2-3 touching; 0-4 touching (counts for 4); 5-99 touching, bodyB outside the array (counts
    for 5, joins nothing); 6-12 without points; 7-12 touching: the only edge that joins two islands; 1-0 touching (counts for nobody).
    Slots 6 and 12 share the top speed; slot 11's velocity is a NaN.  Every number is a small dyadic fraction."""
    D = wire.BODY_DYNAMIC
    bodies = np.zeros(13, dtype=wire.body_dtype)
    bodies["type"] = [wire.BODY_STATIC, wire.BODY_KINEMATIC, D, D, D, D, D, D, D, wire.BODY_FREE, D, D, D]
    bodies["rot"] = (0.0, 1.0)
    bodies["rot"][3] = (1.0, 0.0)   # a quarter turn: atan2f(1, 0) = pi / 2 in float32
    bodies["rot"][5] = (0.0, -1.0)  # a half turn: atan2f(+0, -1) = pi
    bodies["invMass"], bodies["invI"], bodies["mass"], bodies["I"] = 1.0, 2.0, 1.0, 0.5
    for i in (0, 1, 8, 9):
        bodies[i]["invMass"] = bodies[i]["invI"] = bodies[i]["mass"] = bodies[i]["I"] = 0.0
    bodies["position"] = [(i, 0.5 * i) for i in range(13)]
    #                            0       1           2            3          4          5           6         7          8        9 (free)    10          11        12
    bodies["linearVelocity"] = [(0, 0), (0.5, 0.0), (0.25, 0.0), (1.0, 1.0), (0.0, 0.5), (0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 0.0), (9.0, 9.0), (0.25, 0.25), (NAN, 0.0), (0.0, -2.0)]
    bodies["angularVelocity"] = [0.0, 0.0, 1.0, 0.0, 0.0, 1.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    origins = np.array([(i + 0.5, 0.5 * i) for i in range(13)], dtype=np.float32)
    joints = np.zeros(11, dtype=wire.joint_dtype)
    R, M = wire.JOINT_REVOLUTE, wire.JOINT_MOUSE
    joints["type"] = [R, R, R, R, R, R, wire.JOINT_FREE, R, R, M, M]
    joints["bodyA"] = [0, 2, 0, 1, 5, 1, 4, 3, 8, 0, 12]
    joints["bodyB"] = [2, 3, 4, 5, 6, 7, 5, 8, 4, 10, 2]
    contacts = np.zeros(6, dtype=wire.contact_dtype)
    contacts["bodyA"] = [2, 0, 5, 6, 7, 1]
    contacts["bodyB"] = [3, 4, 99, 12, 12, 0]
    contacts["pointCount"] = [1, 2, 1, 0, 2, 1]
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": np.zeros(0, dtype=wire.shape_dtype),
            "pairs": np.zeros(6, dtype=wire.pair_state_dtype), "origins": origins}


def test_reference_statement_on_a_hand_written_world():
    w = thirteen_slot_world()
    state = ref.new_state(w)
    assert state["timer"].tobytes() == bytes(4 * 13)  # +0
    #                 0    1     2     3    4     5    6    7    8    9    10   11   12
    state["timer"][:] = [0.0, 0.25, 0.25, 0.5, 0.75, 0.5, 0.0, 0.0, 0.5, 0.5, 0.0, 1.0, 0.5]
    # bodies 2 and 5 turn, 7 shifts its origin by one ulp-free step, the free slot 9 "moves" too and is nobody's business
    w["bodies"]["rot"][2] = (1.0, 0.0)
    w["origins"][7] = (7.5, 3.75)
    w["origins"][9] = (0.0, 0.0)
    w["bodies"]["position"][4] = (99.0, 99.0)  # the position is not part of the pose that is compared
    step = ref.advance(state, w, THRESHOLDS, DT)
    assert step["reported"].tolist() == [False, True, True, True, True, True, True, True, True, False, True, True, True]
    assert np.flatnonzero(step["moved"]).tolist() == [2, 7]
    # speedSquared: 1: 0.25, 2: 0.0625, 3: 2, 4: 0.25, 5: 0, 6: 4, 7: 0.5, 8: 0, 10: 0.125, 11: NaN, 12: 4; w * w: 2: 1, 5: 1.5625
    assert step["speed2"][[1, 2, 3, 4, 5, 6, 7, 8, 10, 12]].tolist() == [0.25, 0.0625, 2.0, 0.25, 0.0, 4.0, 0.5, 0.0, 0.125, 4.0]
    assert np.isnan(step["speed2"][11])
    # candidates (speedSquared <= 0.25 and w * w <= 1): 1, 2, 4, 8, 10; not 5 (w), not 11 (NaN), not 3, 6, 7, 12
    assert step["timer"].tolist() == [0.0, 0.5, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.75, 0.5, 0.25, 0.0, 0.0]
    assert step["timer"].tobytes() == np.array(step["timer"].tolist(), dtype=f32).tobytes() and not np.signbit(step["timer"]).any()
    # at rest (timer >= 0.5; 1 and 2 reach it exactly); the free slot 9 keeps its timer and is never at rest
    assert np.flatnonzero(step["now"]).tolist() == [1, 2, 4, 8]
    assert np.flatnonzero(step["before"]).tolist() == [3, 4, 5, 8, 11, 12]
    rested, woke = ref.events(step)
    assert rested.tolist() == [1, 2] and woke.tolist() == [3, 5, 11, 12] and rested.dtype == np.int32
    assert state["timer"].tobytes() == step["timer"].tobytes() and state["pose"].tobytes() == ref.pose_of(w).tobytes()

    island, isl = ref.islands(w, step)
    #                          0  1  2  3  4  5  6  7   8   9  10 11 12
    assert island.tolist() == [-1, 0, 1, 1, 2, 3, 3, 4, 5, -1, 6, 7, 4]
    assert isl.dtype == wire.island_state_dtype and isl["firstBody"].tolist() == [1, 2, 4, 5, 7, 8, 10, 11]
    assert isl["bodyCount"].tolist() == [1, 2, 1, 2, 2, 1, 1, 1]
    # contacts: 2-3 -> island 1; 0-4 -> 2; 5-99 -> 3; 7-12 -> 4; 1-0 -> nobody; 6-12 has no points
    assert isl["contactCount"].tolist() == [0, 1, 1, 1, 1, 0, 0, 0]
    # joints by bodyA when movable, else bodyB: 0-2 -> 1, 2-3 -> 1, 0-4 -> 2, 1-5 -> 3, 5-6 -> 3, 1-7 -> 4, 3-8 -> 1, 8-4 -> 2;
    # the mouse joints by bodyB alone: 10 -> 6, 2 -> 1 (bodyA 12 is not looked at)
    assert isl["jointCount"].tolist() == [0, 4, 2, 2, 1, 0, 1, 0]
    assert isl["restingBodies"].tolist() == [1, 1, 1, 0, 0, 1, 0, 0]
    assert isl["minRestTime"].tolist() == [0.5, 0.0, 1.0, 0.0, 0.0, 0.75, 0.25, 0.0]
    # of 7 (0.5) and 12 (4), 12; of 5 (0) and 6 (4), 6; island 7 holds the NaN alone
    assert isl["fastestBody"].tolist() == [1, 3, 4, 6, 12, 8, 10, -1]
    assert isl["maxSpeedSquared"].tolist() == [0.25, 2.0, 0.25, 4.0, 4.0, 0.0, 0.125, -1.0]
    # the same islands as the host's finder on a world it accepts (without the edge that leaves the array)
    ok = w["contacts"][w["contacts"]["bodyB"] < 13]
    host, n = islands.find_islands(w["bodies"], ok, w["joints"])
    assert n == 8 and host.tolist() == island.tolist()

    s = ref.states(w, step, island=island, island_states=isl)
    assert s.dtype == wire.body_state_dtype and s["slot"].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]
    assert s["island"].tolist() == [0, 1, 1, 2, 3, 3, 4, 5, 6, 7, 4]
    # bit 0 moved (2, 7), bit 1 at rest (1, 2, 4, 8), bit 2 the island is at rest (islands 0, 2, 5: slots 1, 4, 8)
    assert s["flags"].tolist() == [2 | 4, 1 | 2, 0, 2 | 4, 0, 0, 1, 2 | 4, 0, 0, 0]
    assert s["type"].tolist() == [1] + [2] * 10
    assert s["origin"].tolist() == [[1.5, 0.5], [2.5, 1.0], [3.5, 1.5], [4.5, 2.0], [5.5, 2.5], [6.5, 3.0], [7.5, 3.75], [8.5, 4.0], [10.5, 5.0], [11.5, 5.5],
                                    [12.5, 6.0]]
    assert s["position"][3].tolist() == [99.0, 99.0] and s["position"][0].tolist() == [1.0, 0.5]
    assert s["rot"][1].tolist() == [1.0, 0.0] and s["rot"][4].tolist() == [0.0, -1.0]
    half_pi, pi = f32(1.5707963705062866), f32(3.1415927410125732)
    assert s["angle"].tolist() == [0.0, half_pi, half_pi, 0.0, pi, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert s["angularVelocity"].tolist() == [0.0, 1.0, 0.0, 0.0, 1.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert s["linearVelocity"][2].tolist() == [1.0, 1.0] and np.isnan(s["linearVelocity"][9][0])
    assert s["restTime"].tolist() == [0.5, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.75, 0.25, 0.0, 0.0]
    assert s["speedSquared"][[0, 1, 2, 5, 10]].tolist() == [0.25, 0.0625, 2.0, 4.0, 4.0] and np.isnan(s["speedSquared"][9])
    only = ref.states(w, step, moved_only=True)
    assert only["slot"].tolist() == [2, 7] and only["island"].tolist() == [-1, -1] and only["flags"].tolist() == [1 | 2, 1]

    m = ref.summary(w, step, isl)
    assert m.dtype == wire.body_summary_dtype
    assert [int(m[k]) for k in ("bodies", "dynamicBodies", "kinematicBodies", "movedBodies", "restingBodies")] == [11, 10, 1, 2, 4]
    # islands 1, 3 and 4 have two bodies: the lowest index; 6 and 12 share the top speed: the lower slot
    assert [int(m[k]) for k in ("islands", "restingIslands", "largestIsland", "largestIslandBodies", "fastestBody")] == [8, 3, 1, 2, 6]
    assert float(m["maxSpeedSquared"]) == 4.0 and m["pad"].tolist() == [0] * 5
    m = ref.summary(w, step)
    assert [int(m[k]) for k in ("islands", "restingIslands", "largestIsland", "largestIslandBodies", "fastestBody")] == [0, 0, -1, 0, 6]

    # the next step: nobody moved; 1 and 2 stay at rest, 10 reaches 0.5 exactly
    step = ref.advance(state, w, THRESHOLDS, DT)
    assert not step["moved"].any()
    rested, woke = ref.events(step)
    assert rested.tolist() == [10] and woke.tolist() == [] and np.flatnonzero(step["now"]).tolist() == [1, 2, 4, 8, 10]
    # thresholds changed by the caller: "before" is the kept timers under the new `seconds`, so only what the step changes is an event
    step = ref.advance(state, w, (0.5, 1.0, 1.0), DT)
    # timers now 1: 1.0, 2: 1.0, 4: 1.5, 8: 1.25, 10: 0.75; before (>= 1 on the old timers 0.75, 0.75, 1.25, 1.0, 0.5): 4, 8
    rested, woke = ref.events(step)
    assert rested.tolist() == [1, 2] and woke.tolist() == []
    # nothing reported: the fields of "nobody"
    w["bodies"]["type"] = wire.BODY_STATIC
    step = ref.advance(ref.new_state(w), w, THRESHOLDS, DT)
    island, isl = ref.islands(w, step)
    m = ref.summary(w, step, isl)
    assert len(isl) == 0 and (island == -1).all() and len(ref.states(w, step)) == 0
    assert [int(m[k]) for k in ("bodies", "islands", "largestIsland", "largestIslandBodies", "fastestBody")] == [0, 0, -1, 0, -1]
    assert float(m["maxSpeedSquared"]) == -1.0


def test_synthetic_world_has_the_events_the_gpu_test_needs():
    """The oracle chain in pool order, stated by the reference alone: what keeps tests/test_gpu_body_report.py from passing on nothing."""
    world = body_report_world.synthetic_world()
    body_report_world.assert_world_is_what_it_says(world)
    vel, pos = common.DEFAULT_ITERS["TGS_Soft"]
    params = wire.StepParams.make("TGS_Soft", float(body_report_world.DT), vel, pos, True)
    state = ref.new_state(world)
    rested_all, woke_all = [], []
    dropped = np.array(body_report_world.DROPPED)
    for n in range(1, 13):
        world_chain.oracle_world_step(params, world)
        step = ref.advance(state, world, body_report_world.THRESHOLDS, params.dt)
        rested, woke = ref.events(step)
        rested_all += rested.tolist()
        woke_all += woke.tolist()
        # the bodies that start at rest under gravity: at rest after step 3, awake after step 4
        assert step["now"][dropped].all() == (n == 3) and step["now"][dropped].any() == (n == 3), n
        for t in (0, 256, 512):
            tile = slice(t, t + 256)
            unmoved = step["reported"][tile] & ~step["moved"][tile]
            assert int(unmoved.sum()) >= 10 and int(step["moved"][tile].sum()) >= 10, (n, t)
            assert int(step["reported"][tile].sum()) % 64 != 0
        island, isl = ref.islands(world, step)
        groups = sorted(sorted(np.flatnonzero(island == k).tolist()) for k in range(len(isl)) if isl[k]["bodyCount"] > 1)
        assert groups == sorted(sorted(g) for g in body_report_world.expected_islands()), n
        assert int(isl["jointCount"].sum()) == int((world["joints"]["type"] != wire.JOINT_FREE).sum())
    assert len(rested_all) >= 8 and len(woke_all) >= 8, (len(rested_all), len(woke_all))
    for events in (rested_all, woke_all):
        assert any(e < 256 for e in events) and any(e >= 256 for e in events)
    damped = set(body_report_world.DAMPED)
    assert len(damped & set(rested_all)) >= 8  # slowed down through the threshold
    assert np.isfinite(world["bodies"]["position"]).all()


@hostcheck_util.needs_sanitizers
def test_body_report_host_code_under_asan_and_ubsan(tmp_path):
    """tests/hostcheck/body_report_main.cpp, a program of its own: upload -> every flag combination -> thresholds set and changed ->
    every getter with too-small, exact and ample buffers -> uploads with other capacities -> destroy, on the sanitizer build of
    tests/test_hostcheck.py (kernels never run there: what is checked is that the host code touches only memory it owns)."""
    hostcheck_util.run_sanitized(tmp_path, "body_report_main.cpp", "BODY REPORT MAIN OK", timeout=600)
