"""The reference side of the world-edit tests (tests/test_world_edit_host.py) and the generator of their fixtures
tests/golden/world_edit/*.npz (python -m tests.world_edit_world, with oracle/_ref/libs2ref.so built).  Test infrastructure only.

A case is a scene of the reference stepped a while, packed into wire arrays, a seeded list of edits on the targets the reference's own
functions accept (live body slots, joints of the right type) with repeated targets, the reference's eight functions called with that list
through ctypes, and the world packed again.  A fixture holds exactly that: the arrays before, the list, the reference's arrays after --
data only."""
import ctypes
import os

import numpy as np

from solver2d_amd import wire
from tests import refbind, world_edit_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_edit")
# name -> (scene, p0, p1, steps before the edits, edits, seed)
CASES = {"mixed24": ("mixed", 24, 0, 30, 400, 11), "far_ragdoll_pile0": ("far_ragdoll_pile", 0, 0, 20, 600, 12),
         "joint_grid6": ("joint_grid", 6, 6, 10, 400, 13), "tumbler60": ("tumbler", 60, 0, 40, 400, 14)}
FIXTURE_KEYS = ("bodies_before", "joints_before", "edits", "bodies_after", "joints_after")


class Vec2(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float)]


class ObjectId(ctypes.Structure):  # s2BodyId, s2JointId (include/solver2d/id.h:19-40)
    _fields_ = [("index", ctypes.c_int32), ("world", ctypes.c_int16), ("revision", ctypes.c_uint16)]


def setters():
    L = refbind.lib()
    table = {"s2Body_SetLinearVelocity": [ObjectId, Vec2], "s2Body_SetAngularVelocity": [ObjectId, ctypes.c_float],
             "s2Body_ApplyForceToCenter": [ObjectId, Vec2], "s2Body_ApplyLinearImpulse": [ObjectId, Vec2, Vec2],
             "s2MouseJoint_SetTarget": [ObjectId, Vec2], "s2RevoluteJoint_EnableLimit": [ObjectId, ctypes.c_bool],
             "s2RevoluteJoint_EnableMotor": [ObjectId, ctypes.c_bool], "s2RevoluteJoint_SetMotorSpeed": [ObjectId, ctypes.c_float]}
    for name, args in table.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, None
    return L


def reference_apply(world, edits):
    """The reference's own eight functions on a refbind.RefWorld, one call per edit in list order.  Ids are {index, world, revision 0}:
    the recipe compiles with NDEBUG (tests/test_world_edit_host.py checks that it says so), so no function reads the revision."""
    L = setters()
    for e in edits:
        oid = ObjectId(int(e["target"]), world.id.index, 0)
        v = [float(x) for x in e["v"]]
        kind = int(e["kind"])
        if kind == wire.EDIT_BODY_SET_LINEAR_VELOCITY:
            L.s2Body_SetLinearVelocity(oid, Vec2(v[0], v[1]))
        elif kind == wire.EDIT_BODY_SET_ANGULAR_VELOCITY:
            L.s2Body_SetAngularVelocity(oid, v[0])
        elif kind == wire.EDIT_BODY_APPLY_FORCE_TO_CENTER:
            L.s2Body_ApplyForceToCenter(oid, Vec2(v[0], v[1]))
        elif kind == wire.EDIT_BODY_APPLY_LINEAR_IMPULSE:
            L.s2Body_ApplyLinearImpulse(oid, Vec2(v[0], v[1]), Vec2(v[2], v[3]))
        elif kind == wire.EDIT_MOUSE_SET_TARGET:
            L.s2MouseJoint_SetTarget(oid, Vec2(v[0], v[1]))
        elif kind == wire.EDIT_REVOLUTE_ENABLE_LIMIT:
            L.s2RevoluteJoint_EnableLimit(oid, bool(e["flag"] != 0))
        elif kind == wire.EDIT_REVOLUTE_ENABLE_MOTOR:
            L.s2RevoluteJoint_EnableMotor(oid, bool(e["flag"] != 0))
        else:
            assert kind == wire.EDIT_REVOLUTE_SET_MOTOR_SPEED
            L.s2RevoluteJoint_SetMotorSpeed(oid, v[0])


def reference_case(name):
    """-> dict of FIXTURE_KEYS, from the compiled reference"""
    scene, p0, p1, steps, count, seed = CASES[name]
    with refbind.RefWorld(scene, "TGS_Soft", p0, p1) as world:
        for _ in range(steps):
            world.step()
        bodies, contacts, joints = world.pack()
        edits = ref.random_edits(np.random.RandomState(seed), bodies, joints, count)
        reference_apply(world, edits)
        after_b, after_c, after_j = world.pack()
        assert after_c.tobytes() == contacts.tobytes()
    return dict(zip(FIXTURE_KEYS, (bodies, joints, edits, after_b, after_j)))


def fixture_path(name):
    return os.path.join(GOLDEN, "%s.npz" % name)


def load_fixture(name):
    with np.load(fixture_path(name)) as d:
        return {k: d[k] for k in FIXTURE_KEYS}


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for case in CASES:
        data = reference_case(case)
        np.savez_compressed(fixture_path(case), **data)
        print(case, {k: len(v) for k, v in data.items()}, os.path.getsize(fixture_path(case)), "bytes")
