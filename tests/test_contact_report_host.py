"""The contact report without a GPU: the two new structs of include/solver2d_amd.h have the sizes of their wire dtypes, and the
reference statement the GPU tests compare against (tests/contact_report_ref.py) gives, on a world small enough to work out by hand,
the values written out here."""
import numpy as np

from solver2d_amd import wire
from tests import contact_report_ref as ref, hostcheck_util


def test_report_struct_sizes_match_header(tmp_path):
    hostcheck_util.assert_struct_layout(tmp_path, {"s2amdTouchingContact": wire.touching_contact_dtype, "s2amdBodyContactSum": wire.body_contact_sum_dtype})
    assert [wire.touching_contact_dtype.itemsize, wire.body_contact_sum_dtype.itemsize] == [64, 16]


def test_report_exports_and_flags():
    hostcheck_util.assert_header_and_bindings(("s2amd_world_set_report", "s2amd_world_touch_events", "s2amd_world_touching", "s2amd_world_body_sums"))
    assert (wire.REPORT_TOUCH, wire.REPORT_CONTACTS, wire.REPORT_BODY_SUMS, wire.REPORT_ALL) == (1, 2, 4, 7)


def three_contact_world():
    """Bodies 0, 1, 2; contact 0 (0 -> 1) with two points, contact 1 (1 -> 2) with one, contact 2 (0 -> 2) without points: body 1 is
    bodyB of one contact and bodyA of another.  Every number is a small dyadic fraction: the float32 results are exact."""
    bodies = np.zeros(3, dtype=wire.body_dtype)
    bodies["rot"] = [(0.0, 1.0), (1.0, 0.0), (0.0, 1.0)]  # {s, c}: body 1 is turned by 90 degrees
    origins = np.array([(1.0, 2.0), (0.5, -1.0), (7.0, 7.0)], dtype=np.float32)
    contacts = np.zeros(3, dtype=wire.contact_dtype)
    pairs = np.zeros(3, dtype=wire.pair_state_dtype)
    pairs["shapeA"], pairs["shapeB"] = [0, 1, 0], [1, 2, 2]
    contacts["bodyA"], contacts["bodyB"] = [0, 1, 0], [1, 2, 2]
    contacts["pointCount"] = [2, 1, 0]
    contacts["normal"] = [(0.0, 1.0), (1.0, 0.0), (0.0, 1.0)]
    c0 = contacts[0]["points"]
    c0[0]["localAnchorA"], c0[0]["separation"], c0[0]["normalImpulse"], c0[0]["tangentImpulse"] = (0.5, 0.25), -0.125, 2.0, 0.5
    c0[1]["localAnchorA"], c0[1]["separation"], c0[1]["normalImpulse"], c0[1]["tangentImpulse"] = (-0.5, 0.25), 0.0, 4.0, -1.0
    c1 = contacts[1]["points"]
    c1[0]["localAnchorA"], c1[0]["separation"], c1[0]["normalImpulse"], c1[0]["tangentImpulse"] = (2.0, 1.0), 0.0625, 8.0, 0.25
    # what a one-point manifold leaves in its second point, and a manifold without points in both, is not reported
    c1[1]["localAnchorA"], c1[1]["normalImpulse"], c1[1]["tangentImpulse"], c1[1]["separation"] = (9.0, 9.0), 99.0, 99.0, 9.0
    contacts[2]["points"][0]["normalImpulse"] = 55.0
    pairs["persisted"] = [(1, 0), (1, 1), (1, 1)]
    return {"bodies": bodies, "contacts": contacts, "joints": np.zeros(0, dtype=wire.joint_dtype), "shapes": np.zeros(3, dtype=wire.shape_dtype),
            "pairs": pairs, "origins": origins}


def test_reference_statement_on_a_hand_written_world():
    w = three_contact_world()
    assert ref.touching_mask(w).tolist() == [True, True, False]
    began, ended = ref.events([False, False, True], w)
    assert began.tolist() == [0, 1] and ended.tolist() == [2] and began.dtype == np.int32
    began, ended = ref.events(ref.before_of(w["contacts"]), w)
    assert began.tolist() == [] and ended.tolist() == []

    t = ref.touching(w)
    assert t.dtype == wire.touching_contact_dtype and len(t) == 2
    assert t["slot"].tolist() == [0, 1] and t["bodyA"].tolist() == [0, 1] and t["bodyB"].tolist() == [1, 2]
    assert t["pointCount"].tolist() == [2, 1] and t["persisted"].tolist() == [[1, 0], [1, 0]] and t["pad"].tolist() == [0, 0]
    assert t["normal"].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    # body 0: identity rotation, origin (1, 2); body 1: x = (c * 2 - s * 1) + 0.5 = -0.5, y = (s * 2 + c * 1) - 1 = 1
    assert t["point"].tolist() == [[[1.5, 2.25], [0.5, 2.25]], [[-0.5, 1.0], [0.0, 0.0]]]
    assert t["separation"].tolist() == [[-0.125, 0.0], [0.0625, 0.0]]
    assert t["normalImpulse"].tolist() == [[2.0, 4.0], [8.0, 0.0]]
    assert t["tangentImpulse"].tolist() == [[0.5, -1.0], [0.25, 0.0]]

    # contact 0: tangent (1, -0): P0 = (0.5, 2), P1 = (-1, 4); contact 1: tangent (0, -1): P = (8, -0.25)
    s = ref.body_sums(w)
    assert s.dtype == wire.body_contact_sum_dtype
    assert s["impulse"].tolist() == [[0.5, -6.0], [-8.5, 6.25], [8.0, -0.25]]
    assert s["normalImpulse"].tolist() == [6.0, 14.0, 8.0]
    assert s["touching"].tolist() == [1, 2, 1]


def test_a_dead_pair_slot_does_not_touch():
    w = three_contact_world()
    w["pairs"]["shapeA"][0] = -1
    assert ref.touching_mask(w).tolist() == [False, True, False]
    assert ref.touching(w)["slot"].tolist() == [1]
    assert ref.body_sums(w)["touching"].tolist() == [0, 1, 1]
