"""What the GPU tests of the resident world (tests/test_gpu_*.py) share: the error codes, upload / download / one step beside the oracle
chain, the refusal loop, the byte-for-byte comparisons with their "first differing rows" messages, and the world builders and pickers
that more than one feature's tests use.  A helper that belongs to one feature lives in that feature's tests/*_world.py or
tests/*_ref.py; raw s2Solve_* parity helpers live in tests/parity.py.  Test infrastructure only."""
import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import contact_report_ref, ray_report_world as rw, step_metrics_ref, world_chain
from tests.world_chain import golden, oracle_world_step

E_INVALID, E_STATE, E_CAPACITY = -1, -4, -5
OTHER_KEYS = ("contacts", "shapes", "pairs", "origins")
# the observers' kinds (S2AMD_OBSERVER_*), in the header's order
POINT, ROTATION, ANGLE, LINEAR, ANGULAR, REV_ANGLE, REV_SPEED, REV_IMPULSE, CONTACT, RAY, ACTION = range(1, 12)


def upload(s, world):
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])


def download(s, world):
    """-> (the resident world in copies of `world`'s arrays, the stage-3 status of the last step)"""
    out = world_chain.copy_world(world)
    res = s.world_download(*[out[k] for k in world_chain.WORLD_KEYS])
    return dict(zip(world_chain.WORLD_KEYS, res[:6])), res[6]


def downloaded_world(s, world):
    """download() without the status"""
    return download(s, world)[0]


def step_both(s, params, ref_world):
    """One s2amd_world_step and the same step of the oracle chain in the device's orders; returns the step's info."""
    info = s.world_step(params)
    order, _ = s.contact_order()
    jorder, _ = s.joint_order()
    oracle_world_step(params, ref_world, contact_order=order, joint_order=jorder)
    return info


def refuses(s, code, getters):
    """Every getter of `getters` (names of hip.Solver methods) raises with S2AMD error `code`"""
    for name in getters:
        with pytest.raises(hip.S2AmdError, match="error %d" % code):
            getattr(s, name)()


def assert_same_bytes(got, want, what):
    """Two arrays: the same dtype, shape and bytes; the failure names the first differing rows"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %r %r / %r %r" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = np.atleast_1d(got), np.atleast_1d(want)
        rows = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(g, w)])
        raise AssertionError("%s differs, first rows %s: got %r, want %r" % (what, rows[:8].tolist(), g[rows[:2]], w[rows[:2]]))


def assert_equal_bytes(got, want, what, keys=None):
    """assert_same_bytes for every key of `keys` (of `got` where none are given) of two dicts of arrays"""
    for key in (got if keys is None else keys):
        assert_same_bytes(got[key], want[key], "%s: %s" % (what, key))


def assert_record(got, want, what):
    assert got.dtype == wire.step_metrics_dtype
    if not step_metrics_ref.same_record(got, want):
        bad = [n for n in got.dtype.names if np.asarray(got[n]).tobytes() != np.asarray(want[n]).tobytes()]
        raise AssertionError("%s: the record differs in %s: %s / reference %s" % (what, bad, got, want))


def assert_metrics_equal_reference(s, ref_world, params, flags, step, what):
    """s2amd_world_metrics against the statement on `ref_world` (the oracle chain after the step); returns the reference record"""
    want = step_metrics_ref.record(ref_world, params, flags, step)
    assert_record(s.world_metrics(), want, what)
    return want


def assert_same_world(got, want, what, keys=world_chain.WORLD_KEYS):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.tobytes() != b.tobytes():
            bad = [n for n in a.dtype.names if a[n].tobytes() != b[n].tobytes()] if a.dtype.names else []
            rows = np.flatnonzero([a[i].tobytes() != b[i].tobytes() for i in range(len(a))])
            raise AssertionError("%s: %s differ in fields %s, first rows %s" % (what, k, bad, rows[:5].tolist()))


def slots_of(world):
    b, j = world["bodies"], world["joints"]
    return {"free": np.flatnonzero(b["type"] == wire.BODY_FREE), "static": np.flatnonzero(b["type"] == wire.BODY_STATIC),
            "kinematic": np.flatnonzero(b["type"] == wire.BODY_KINEMATIC), "dynamic": np.flatnonzero(b["type"] == wire.BODY_DYNAMIC),
            "free_joint": np.flatnonzero(j["type"] == wire.JOINT_FREE), "revolute": np.flatnonzero(j["type"] == wire.JOINT_REVOLUTE),
            "mouse": np.flatnonzero(j["type"] == wire.JOINT_MOUSE)}


def motorised(world, torque=40.0):
    """A copy whose revolute joints have their motors on"""
    out = world_chain.copy_world(world)
    rev = out["joints"]["type"] == wire.JOINT_REVOLUTE
    out["joints"]["enableMotor"][rev] = 1
    out["joints"]["maxMotorTorque"][rev] = torque
    return out


def packed(records):
    """(kind, target, keyword arguments) triples -> the list with channels packed in order, and the channel count"""
    out, channel = [], 0
    for kind, target, kw in records:
        out.append(wire.observer(kind, target, channel, **kw))
        channel += wire.OBSERVER_WIDTH[kind]
    return wire.observer_list(out), channel


def down_ray(world, body):
    x = float(world["bodies"]["position"][body][0])
    return rw.make_ray((x, 60.0), (x, -60.0))


def every_kind(world):
    """The eleven kinds on mixed24; the contact observer sits on the body the plain oracle step presses hardest"""
    at = slots_of(world)
    d, rev = at["dynamic"], at["revolute"]
    probe = world_chain.copy_world(world)
    world_chain.oracle_world_step(golden("mixed24_PGS")[0], probe)
    sums = contact_report_ref.body_sums(probe)
    pressed = int(d[np.argmax(sums["normalImpulse"][d])])
    return packed([(POINT, d[0], dict(frame=d[1], local=(0.25, -0.5), gain=0.5)), (ROTATION, d[2], dict(frame=d[3])), (ANGLE, d[4], dict(frame=d[5], gain=2.0)),
                   (LINEAR, d[6], dict(frame=d[7], flags=wire.OBSERVER_RELATIVE, gain=0.25, lower=-1.0, upper=1.0)), (ANGULAR, d[8], dict(frame=d[9], flags=wire.OBSERVER_RELATIVE, bias=0.125)),
                   (REV_ANGLE, rev[0], dict(gain=-1.0)), (REV_SPEED, rev[1], dict(gain=0.5)), (REV_IMPULSE, rev[0], dict(gain=10.0)),
                   (CONTACT, pressed, dict(gain=0.5, bias=0.25)), (RAY, 0, dict(gain=0.01)), (ACTION, 1, dict(bias=1.0))])
