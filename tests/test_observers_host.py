"""The observers without a GPU: the interface as declared and bound with the header's sizes and offsets, the statement
(tests/observer_ref.py) on hand-made cases with exactly representable numbers -- a 3-4-5 frame rotation, the clamp's edges, a NaN passing
through, every status in the stated priority order --, the history rule over a re-base, the setter's validation cases as data, the
compiler's resource report of the new kernel, and the host side under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a
stand-alone program, nothing preloaded)."""
import re

import numpy as np

from solver2d_amd import wire
from tests import hostcheck_util, observer_ref as ref

CALLS = ("s2amd_world_set_observers", "s2amd_world_set_observation_report", "s2amd_world_observations", "s2amd_world_export_observations",
         "s2amd_world_export_observations_async", "s2amd_world_observer_states", "s2amd_world_observer_counts")
F = np.float32
INF = F(np.inf)


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    records = {"s2amdObserver": wire.observer_dtype, "s2amdObserverState": wire.observer_state_dtype}
    hostcheck_util.assert_struct_layout(tmp_path, records)
    assert (wire.OBSERVER_SIZE, wire.OBSERVER_STATE_SIZE) == (64, 32)


def test_header_defines_and_bindings():
    defines = {"S2AMD_MAX_OBSERVERS": wire.MAX_OBSERVERS, "S2AMD_MAX_OBSERVATION_CHANNELS": wire.MAX_OBSERVATION_CHANNELS,
               "S2AMD_MAX_OBSERVATION_FRAMES": wire.MAX_OBSERVATION_FRAMES, "S2AMD_OBSERVER_BODY_POINT": ref.POINT,
               "S2AMD_OBSERVER_BODY_ROTATION": ref.ROTATION, "S2AMD_OBSERVER_BODY_ANGLE": ref.ANGLE, "S2AMD_OBSERVER_BODY_LINEAR_VELOCITY": ref.LINEAR,
               "S2AMD_OBSERVER_BODY_ANGULAR_VELOCITY": ref.ANGULAR, "S2AMD_OBSERVER_REVOLUTE_ANGLE": ref.REV_ANGLE,
               "S2AMD_OBSERVER_REVOLUTE_SPEED": ref.REV_SPEED, "S2AMD_OBSERVER_REVOLUTE_MOTOR_IMPULSE": ref.REV_IMPULSE,
               "S2AMD_OBSERVER_BODY_CONTACT": ref.CONTACT, "S2AMD_OBSERVER_RAY_RANGE": ref.RAY, "S2AMD_OBSERVER_ACTION": ref.ACTION,
               "S2AMD_OBSERVER_DISABLED": wire.OBSERVER_DISABLED, "S2AMD_OBSERVER_RELATIVE": wire.OBSERVER_RELATIVE,
               "S2AMD_OBSERVER_STATUS_OBSERVED": ref.OBSERVED, "S2AMD_OBSERVER_STATUS_DISABLED": ref.DISABLED,
               "S2AMD_OBSERVER_STATUS_SKIPPED": ref.SKIPPED, "S2AMD_OBSERVER_STATUS_SOURCE_OFF": ref.SOURCE_OFF,
               "S2AMD_OBSERVATION_REPORT_VECTOR": wire.OBSERVATION_REPORT_VECTOR, "S2AMD_OBSERVATION_REPORT_STATES": wire.OBSERVATION_REPORT_STATES,
               "S2AMD_API_VERSION": 5}
    header = hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_OBSERVERS, wire.MAX_OBSERVATION_CHANNELS, wire.MAX_OBSERVATION_FRAMES, wire.API_VERSION) == (16384, 65536, 16, 5)
    assert wire.OBSERVER_WIDTH == {1: 2, 2: 2, 3: 1, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1, 9: 2, 10: 1, 11: 1}
    assert (wire.OBSERVER_BODY_POINT, wire.OBSERVER_ACTION, wire.OBSERVER_STATUS_SOURCE_OFF) == (ref.POINT, ref.ACTION, ref.SOURCE_OFF)
    # the actuators' note on how observations leave names the new export
    assert re.search(r"observations leave device to device \(s2amd_world_export_observations,", header)


# ---- the statement on hand-made cases ----
def tiny_world():
    """bodies: 0 static at the origin, 1 dynamic at (1, 2) rotated by the 3-4-5 angle {s, c} = {0.6, 0.8}, 2 free, 3 dynamic at (5, -1)
    rotated by a quarter turn; joints: 0 revolute between 1 and 3, 1 mouse on 3, 2 free"""
    bodies = np.zeros(4, dtype=wire.body_dtype)
    bodies["rot"] = (0.0, 1.0)
    bodies["type"] = (wire.BODY_STATIC, wire.BODY_DYNAMIC, wire.BODY_FREE, wire.BODY_DYNAMIC)
    bodies["rot"][1], bodies["rot"][3] = (0.6, 0.8), (1.0, 0.0)
    bodies["linearVelocity"][1], bodies["linearVelocity"][3] = (2.0, 1.0), (7.0, -4.0)
    bodies["angularVelocity"][1], bodies["angularVelocity"][3] = 0.5, 2.0
    joints = np.zeros(3, dtype=wire.joint_dtype)
    joints["type"] = (wire.JOINT_REVOLUTE, wire.JOINT_MOUSE, wire.JOINT_FREE)
    joints["bodyA"], joints["bodyB"] = (1, 3, 0), (3, 3, 0)
    joints["referenceAngle"][0], joints["motorImpulse"][0] = 0.25, -1.5
    origins = np.array([(0.0, 0.0), (1.0, 2.0), (9.0, 9.0), (5.0, -1.0)], dtype=F)
    return {"bodies": bodies, "joints": joints, "origins": origins}


def sources():
    sums = np.zeros(4, dtype=wire.body_contact_sum_dtype)
    sums["touching"], sums["normalImpulse"] = (3, 0, 0, 1), (4.5, 0.0, 0.0, 0.75)
    return sums, np.array([0.5, 1.0, 0.25], dtype=F), np.array([-0.75, 2.0], dtype=F)


def one(kind, target, src=None, lengths=None, **kw):
    observers = wire.observer_list([wire.observer(kind, target, 1, **kw)])
    assert ref.valid(observers, 4, 1) == -1
    vector, states, counts = ref.observe(tiny_world(), observers, sources() if src is None else src, channels=4, lengths=lengths)
    assert vector[0] == 0 and vector[3] == 0 and counts.sum() == 1 and counts[states[0]["status"]] == 1
    width = wire.OBSERVER_WIDTH[kind]
    assert vector[1:1 + width].tobytes() == states[0]["value"][:width].tobytes() and not states[0]["value"][width:].any() and not states[0]["raw"][width:].any()
    return states[0]


def bits(x):
    return np.array(x, dtype=F).view(np.uint32).tolist()


def test_frames_with_a_three_four_five_rotation():
    # the point (5, 10) of body 1's frame: rotated {0.8 * 5 - 0.6 * 10, 0.6 * 5 + 0.8 * 10} = {-2, 11}, plus the origin (1, 2)
    assert one(ref.POINT, 1, local=(5.0, 10.0))["raw"].tolist() == [-1.0, 13.0]
    # body 3's origin (5, -1) seen from body 1: d = (4, -3); {0.8 * 4 + 0.6 * -3, -0.6 * 4 + 0.8 * -3} = {1.4, -4.8} as float32 sums
    got = one(ref.POINT, 3, frame=1)["raw"]
    assert bits(got) == bits([F(F(F(0.8) * F(4.0)) + F(F(0.6) * F(-3.0))), F(F(F(-0.6) * F(4.0)) + F(F(0.8) * F(-3.0)))])
    assert np.allclose(got, [1.4, -4.8], atol=1e-6)
    # from the static body at the origin, unrotated: the world point itself
    assert one(ref.POINT, 1, frame=0, local=(5.0, 10.0))["raw"].tolist() == [-1.0, 13.0]
    # rotations: body 3 (a quarter turn) in body 1's frame {c1 * s3 - s1 * c3, c1 * c3 + s1 * s3} = {0.8, 0.6}; the other way {-0.8, 0.6}
    assert one(ref.ROTATION, 3, frame=1)["raw"].tolist() == [F(0.8), F(0.6)]
    assert one(ref.ROTATION, 1, frame=3)["raw"].tolist() == [F(-0.8), F(0.6)]
    assert one(ref.ROTATION, 1)["raw"].tolist() == [F(0.6), F(0.8)]
    assert one(ref.ANGLE, 3)["raw"][0] == F(np.pi / 2) and one(ref.ANGLE, 3, frame=3)["raw"][0] == 0
    assert one(ref.ANGLE, 1, frame=3)["raw"][0] == -one(ref.ANGLE, 3, frame=1)["raw"][0] != 0
    # velocities: body 3's (7, -4) in the quarter-turned frame of itself {c * x + s * y, -s * x + c * y} = {-4, -7}
    assert one(ref.LINEAR, 3)["raw"].tolist() == [7.0, -4.0] and one(ref.LINEAR, 3, frame=3)["raw"].tolist() == [-4.0, -7.0]
    # ... relative to body 1's (2, 1): (5, -5), rotated into body 1's frame {0.8 * 5 + 0.6 * -5, -0.6 * 5 + 0.8 * -5} = {1, -7}
    assert one(ref.LINEAR, 3, frame=1, flags=wire.OBSERVER_RELATIVE)["raw"].tolist() == [1.0, -7.0]
    # RELATIVE without a frame subtracts nothing
    assert one(ref.LINEAR, 3, flags=wire.OBSERVER_RELATIVE)["raw"].tolist() == [7.0, -4.0]
    assert one(ref.ANGULAR, 3)["raw"][0] == 2.0 and one(ref.ANGULAR, 3, frame=1)["raw"][0] == 2.0
    assert one(ref.ANGULAR, 3, frame=1, flags=wire.OBSERVER_RELATIVE)["raw"][0] == 1.5
    assert one(ref.ANGULAR, 3, flags=wire.OBSERVER_RELATIVE)["raw"][0] == 2.0


def test_joint_and_source_kinds():
    # joint 0: bodyA = 1 (the 3-4-5 angle), bodyB = 3 (a quarter turn): s = 1 * 0.8 - 0 * 0.6, c = 0 * 0.8 + 1 * 0.6, minus the reference 0.25
    from tests import joint_report_ref
    assert one(ref.REV_ANGLE, 0)["raw"][0] == F(joint_report_ref.atan2f(F(0.8), F(0.6)) - F(0.25))
    assert one(ref.REV_SPEED, 0)["raw"][0] == 1.5 and one(ref.REV_IMPULSE, 0)["raw"][0] == -1.5
    assert one(ref.CONTACT, 0)["raw"].tolist() == [1.0, 4.5] and one(ref.CONTACT, 3)["raw"].tolist() == [1.0, 0.75]
    assert bits(one(ref.CONTACT, 1)["raw"]) == [0, 0]
    assert one(ref.RAY, 2)["raw"][0] == 0.25 and one(ref.ACTION, 0)["raw"][0] == -0.75
    # the value: gain and bias on every component of a width-2 kind
    st = one(ref.CONTACT, 0, gain=2.0, bias=-1.0, lower=0.0, upper=6.0)
    assert st["value"].tolist() == [1.0, 6.0] and st["raw"].tolist() == [1.0, 4.5]


def test_clamp_edges_and_a_nan_passing_through():
    # t exactly at a bound is not replaced by it: -0.0 at lower = +0.0 keeps its sign, as the two comparisons say
    world = tiny_world()
    world["bodies"]["angularVelocity"][3] = -0.0

    def value(w, **kw):
        world["bodies"]["angularVelocity"][3] = w
        return ref.observe(world, wire.observer_list([wire.observer(ref.ANGULAR, 3, 0, **kw)]), (None, None, None))[1][0]

    assert bits(value(-0.0, bias=-0.0, lower=0.0, upper=1.0)["value"][0]) == bits(F(-0.0))
    assert value(2.0, gain=0.5, lower=1.0, upper=3.0)["value"][0] == 1.0 and value(2.0, gain=0.5, bias=2.0, lower=1.0, upper=3.0)["value"][0] == 3.0
    assert value(2.0, gain=0.5, bias=2.5, lower=1.0, upper=3.0)["value"][0] == 3.0 and value(-9.0, gain=0.5, lower=1.0, upper=3.0)["value"][0] == 1.0
    # one rounding per operation: 2^24 + 1 is 2^24
    assert value(1.0, gain=F(2.0 ** 24), bias=1.0)["value"][0] == F(2.0 ** 24)
    # infinite bounds let an overflowing product through, finite bounds catch it
    assert value(3.0e38, gain=2.0)["value"][0] == INF and value(3.0e38, gain=2.0, lower=-5.0, upper=7.0)["value"][0] == 7.0
    # a NaN fails both comparisons: it is OBSERVED and passes through unclamped, in raw and in value
    st = value(np.nan, lower=-1.0, upper=1.0)
    assert st["status"] == ref.OBSERVED and np.isnan(st["raw"][0]) and np.isnan(st["value"][0])
    # ... and an infinity is clamped
    assert value(np.inf, lower=-1.0, upper=1.0)["value"][0] == 1.0


def test_every_status_in_the_stated_order():
    off = (None, None, None)
    # DISABLED before everything: a free target, a source that is off
    for kind, target in ((ref.POINT, 2), (ref.REV_ANGLE, 1), (ref.CONTACT, 2), (ref.RAY, 99), (ref.ACTION, 0)):
        st = one(kind, target, src=off, flags=wire.OBSERVER_DISABLED)
        assert st["status"] == ref.DISABLED and not st["raw"].any() and not st["value"].any()
    # SKIPPED: a free body, a body beyond the array, a frame on a free slot and beyond the array; a mouse joint, a free joint, a joint beyond
    for kind, target, frame in ((ref.POINT, 2, -1), (ref.ANGLE, 4, -1), (ref.LINEAR, 1, 2), (ref.ROTATION, 1, 4), (ref.ANGULAR, 2, 1),
                                (ref.REV_ANGLE, 1, -1), (ref.REV_SPEED, 2, -1), (ref.REV_IMPULSE, 3, -1), (ref.CONTACT, 2, -1), (ref.CONTACT, 4, -1)):
        st = one(kind, target, frame=frame, bias=5.0)
        assert st["status"] == ref.SKIPPED and bits(st["raw"]) == [0, 0] and bits(st["value"]) == [0, 0], (kind, target, frame)
    # SKIPPED before SOURCE_OFF: a free body under kind 9 with the sums off; a ray beyond a list whose ranges did not report
    assert one(ref.CONTACT, 2, src=off)["status"] == ref.SKIPPED
    assert one(ref.RAY, 3)["status"] == ref.SKIPPED and one(ref.ACTION, 2)["status"] == ref.SKIPPED
    assert one(ref.RAY, 3, src=off, lengths=(3, 2))["status"] == ref.SKIPPED and one(ref.RAY, 2, src=off, lengths=(3, 2))["status"] == ref.SOURCE_OFF
    # SOURCE_OFF: each source; with no list at all there is no count to be beyond
    sums, ranges, actions = sources()
    assert one(ref.CONTACT, 0, src=(None, ranges, actions))["status"] == ref.SOURCE_OFF
    assert one(ref.RAY, 0, src=(sums, None, actions))["status"] == ref.SOURCE_OFF and one(ref.RAY, 99, src=(sums, None, actions))["status"] == ref.SOURCE_OFF
    assert one(ref.ACTION, 1, src=(sums, ranges, None))["status"] == ref.SOURCE_OFF and one(ref.ACTION, 99, src=(sums, ranges, None))["status"] == ref.SOURCE_OFF
    st = one(ref.CONTACT, 0, src=off, bias=5.0)
    assert bits(st["raw"]) == [0, 0] and bits(st["value"]) == [0, 0]
    # OBSERVED: everything else, the bias alone makes a value
    assert one(ref.CONTACT, 1, bias=5.0)["value"].tolist() == [5.0, 5.0]


def test_history_rule_over_a_rebase():
    h = ref.History(3, 2)
    v = [np.array([k, -k], dtype=F) for k in range(1, 8)]
    assert h.push(v[0]).tolist() == [[1, -1]] * 3  # the first reporting step fills every frame
    assert h.push(v[1]).tolist() == [[2, -2], [1, -1], [1, -1]]
    assert h.push(v[2]).tolist() == [[3, -3], [2, -2], [1, -1]]
    assert h.push(v[3]).tolist() == [[4, -4], [3, -3], [2, -2]]
    h.rebase()
    assert h.push(v[4]).tolist() == [[5, -5]] * 3
    assert h.push(v[5]).tolist() == [[6, -6], [5, -5], [5, -5]]
    one_frame = ref.History(1, 2)
    assert one_frame.push(v[0]).tolist() == [[1, -1]] and one_frame.push(v[1]).tolist() == [[2, -2]]


GOOD = [wire.observer(ref.POINT, 1, 2, frame=0, local=(0.5, 0.25), lower=-1.0, upper=1.0), wire.observer(ref.REV_ANGLE, 0, 0, lower=-1.0, upper=1.0),
        wire.observer(ref.CONTACT, 3, 5), wire.observer(ref.ACTION, 7, 1, flags=wire.OBSERVER_DISABLED | wire.OBSERVER_RELATIVE)]
# (field, index into the field or None, value) on record 0 unless `record` is given: every validation rule of the header
BAD = [("kind", None, 0), ("kind", None, 12), ("target", None, -1), ("frame", None, -2), ("channel", None, -1), ("channel", None, 6), ("flags", None, 4),
       ("flags", None, -1), ("gain", None, np.nan), ("gain", None, np.inf), ("bias", None, np.nan), ("bias", None, -np.inf), ("local", 0, np.nan),
       ("local", 1, np.inf), ("reserved", 0, 1), ("reserved", 4, -1), ("lower", None, np.nan), ("upper", None, np.nan), ("lower", None, 2.0), ("upper", None, -2.0),
       ("channel", None, 0), ("channel", None, 1), ("channel", None, 4)]


def test_validation_rules_of_the_statement():
    good = wire.observer_list(GOOD)
    assert ref.valid(good, 7, 1) == -1 and ref.valid(good, 7, 16) == -1
    assert ref.valid(good, 6, 1) == 2 and ref.valid(good, 0, 1) == 0 and ref.valid(good, wire.MAX_OBSERVATION_CHANNELS + 1, 1) == 0
    assert ref.valid(good, 7, 0) == 0 and ref.valid(good, 7, 17) == 0 and ref.valid(good[:0], 0, 0) == -1
    for name, index, value in BAD:
        wrong = good.copy()
        if index is None:
            wrong[name][0] = value
        else:
            wrong[name][0][index] = value
        assert ref.valid(wrong, 7, 2) >= 0, (name, index, value)
    for record in (1, 2, 3):  # kinds 6-11 take no frame
        wrong = good.copy()
        wrong["frame"][record] = 0
        assert ref.valid(wrong, 7, 2) == record
    allowed = good.copy()
    allowed["lower"], allowed["upper"] = (np.inf, -np.inf, 0.0, -np.inf), (np.inf, -np.inf, 0.0, np.inf)  # lower == upper, infinities
    allowed["target"][0], allowed["frame"][0] = 2 ** 31 - 1, 2 ** 31 - 1  # capacities are the device's to judge
    assert ref.valid(allowed, 7, 2) == -1
    # adjacent ranges do not overlap; one channel of overlap does
    touching = wire.observer_list([wire.observer(ref.POINT, 0, 0), wire.observer(ref.ANGLE, 0, 2), wire.observer(ref.LINEAR, 0, 3)])
    assert ref.valid(touching, 5, 1) == -1
    touching["channel"][1] = 1
    assert ref.valid(touching, 5, 1) == 1


def test_kernels_use_no_scratch():
    """hipcc's own report for observers.hip (make resources-observers), through tools/kernel_resources.py: the kernel of the file is
    there, it has no private frame, spills nothing and uses no LDS."""
    kernels = dict.fromkeys(("observeKernel", "reportBodyRangesKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-observers", "resources_observers.txt", kernels, floor=4, total=2)


@hostcheck_util.needs_sanitizers
def test_observer_host_code_under_asan_and_ubsan(tmp_path):
    """Every validation rule, the overlap check included, with and without a world and a list, each leaving the old list, its sizes, its
    ring's head and its answers standing -> the list held across uploads -> the ring's head over more steps than frames -> the host
    getter, the waiting export and the enqueued export against the stated history at every head position, for frames = 1, 2, 3 (5 and
    16 once), across re-bases by upload, replacement and flags and across steps with the flags at 0 -> the getters with too-small and
    exact heap buffers -> destroy, for 0, 1, 65, 257, 1,000 and 16,384 observers, on the sanitizer build of tests/test_hostcheck.py
    (kernels never run there: the program plays the kernel's one write into the row the host chose)."""
    hostcheck_util.run_sanitized(tmp_path, "observers_main.cpp", "OBSERVERS MAIN OK", timeout=600)
