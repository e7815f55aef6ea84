"""The joint report of include/solver2d_amd.h (s2amd_world_set_joint_report and its getters) stated in numpy on a wire world dict as
tests/world_chain.py keeps it: what the device's compaction (solver2d_amd/csrc/joint_report.hip) must return, byte for byte.
Everything is float32 with one rounding per operation; the angle goes through glibc's atan2f by ctypes, element by element (numpy's
float32 arctan2 need not be glibc's, and the device's s2_atan2f is pinned to glibc).  Test infrastructure only."""
import ctypes
import ctypes.util

import numpy as np

from solver2d_amd import wire

f32 = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def atan2f(y, x):
    return f32(_libm.atan2f(float(f32(y)), float(f32(x))))


def live_slots(joints):
    return np.flatnonzero(joints["type"] != wire.JOINT_FREE)


def _transform_point(origin, rot, p):
    """s2TransformPoint (include/solver2d/math.h:350-356), rot = {s, c}"""
    ox, oy, qs, qc, px, py = f32(origin[0]), f32(origin[1]), f32(rot[0]), f32(rot[1]), f32(p[0]), f32(p[1])
    x = f32(f32(f32(qc * px) - f32(qs * py)) + ox)
    y = f32(f32(f32(qs * px) + f32(qc * py)) + oy)
    return x, y


def _relative_angle(rb, ra):
    """s2RelativeAngle(b, a) (math.h:320-327), rot = {s, c}"""
    bs, bc, as_, ac = f32(rb[0]), f32(rb[1]), f32(ra[0]), f32(ra[1])
    s = f32(f32(bs * ac) - f32(bc * as_))
    c = f32(f32(bc * ac) + f32(bs * as_))
    return atan2f(s, c)


def _axial(j):
    if int(j["type"]) == wire.JOINT_REVOLUTE:
        return f32(f32(f32(j["motorImpulse"]) + f32(j["lowerImpulse"])) - f32(j["upperImpulse"]))  # src/revolute_joint.c:137
    return f32(j["motorImpulse"])  # src/mouse_joint.c:102-103


def states(world):
    """s2amdJointState of every live joint slot, ascending."""
    joints, bodies = world["joints"], world["bodies"]
    origins = np.asarray(world["origins"], dtype=f32)
    slots = live_slots(joints)
    out = np.zeros(len(slots), dtype=wire.joint_state_dtype)
    for k, slot in enumerate(slots.tolist()):
        j, r = joints[slot], out[k]
        a, b = int(j["bodyA"]), int(j["bodyB"])
        r["slot"], r["type"], r["bodyA"], r["bodyB"] = slot, j["type"], a, b
        r["anchorB"] = _transform_point(origins[b], bodies["rot"][b], j["localOriginAnchorB"])
        r["impulse"] = j["impulse"]
        r["motorImpulse"] = j["motorImpulse"]
        r["axialImpulse"] = _axial(j)
        if int(j["type"]) == wire.JOINT_REVOLUTE:
            r["anchorA"] = _transform_point(origins[a], bodies["rot"][a], j["localOriginAnchorA"])
            r["angle"] = f32(_relative_angle(bodies["rot"][b], bodies["rot"][a]) - f32(j["referenceAngle"]))
            r["angularSpeed"] = f32(f32(bodies["angularVelocity"][b]) - f32(bodies["angularVelocity"][a]))
            r["lowerImpulse"], r["upperImpulse"] = j["lowerImpulse"], j["upperImpulse"]
        else:  # mouse: what src/joint.c:485-492 draws; angle and limit impulses are +0 whatever the record holds
            r["anchorA"] = j["targetA"]
            r["angularSpeed"] = bodies["angularVelocity"][b]
    return out


def limit_mask(joints):
    """bool[2 * slots]: entry 2 * slot + side (0 lower, 1 upper) -- a revolute joint with enableLimit whose stored impulse is > 0."""
    limited = (joints["type"] == wire.JOINT_REVOLUTE) & (joints["enableLimit"] != 0)
    mask = np.zeros(2 * len(joints), dtype=bool)
    mask[0::2] = limited & (joints["lowerImpulse"] > 0)
    mask[1::2] = limited & (joints["upperImpulse"] > 0)
    return mask


def events(prev_mask, world):
    """(began, ended) code lists, ascending, of a step that took the limits from `prev_mask` to the state of `world`."""
    now = limit_mask(world["joints"])
    prev = np.asarray(prev_mask, dtype=bool)
    return np.flatnonzero(now & ~prev).astype(np.int32), np.flatnonzero(prev & ~now).astype(np.int32)


def body_sums(world):
    """s2amdBodyJointSum per body slot: a plain loop of float32 adds from +0 over the live joints in slot order, the bodyA term of a
    joint before its bodyB term; revolute: -impulse, -axial for bodyA and +impulse, +axial for bodyB (src/revolute_joint.c:140-144);
    mouse: +impulse, +motorImpulse for bodyB only."""
    nb = len(world["bodies"])
    ix, iy, ax = [f32(0)] * nb, [f32(0)] * nb, [f32(0)] * nb
    count = [0] * nb
    joints = world["joints"]
    for slot in live_slots(joints).tolist():
        j = joints[slot]
        a, b = int(j["bodyA"]), int(j["bodyB"])
        px, py, axial = f32(j["impulse"][0]), f32(j["impulse"][1]), _axial(j)
        if int(j["type"]) == wire.JOINT_REVOLUTE:
            ix[a], iy[a], ax[a] = f32(ix[a] + (-px)), f32(iy[a] + (-py)), f32(ax[a] + (-axial))
            count[a] += 1
        ix[b], iy[b], ax[b] = f32(ix[b] + px), f32(iy[b] + py), f32(ax[b] + axial)
        count[b] += 1
    out = np.zeros(nb, dtype=wire.body_joint_sum_dtype)
    out["impulse"][:, 0], out["impulse"][:, 1] = np.array(ix, dtype=f32), np.array(iy, dtype=f32)
    out["axialImpulse"] = np.array(ax, dtype=f32)
    out["joints"] = count
    return out


def summary(world):
    """One s2amdJointSummary record: counts, and the largest squared anchor gap over the live revolute joints (the lowest slot on a tie,
    never a NaN; -1.0 / -1 without one)."""
    joints = world["joints"]
    out = np.zeros(1, dtype=wire.joint_summary_dtype)[0]
    mask = limit_mask(joints)
    out["liveJoints"] = len(live_slots(joints))
    out["revoluteJoints"] = int((joints["type"] == wire.JOINT_REVOLUTE).sum())
    out["atLower"], out["atUpper"] = int(mask[0::2].sum()), int(mask[1::2].sum())
    best, best_slot = f32(-1.0), -1
    for r in states(world):
        if int(r["type"]) != wire.JOINT_REVOLUTE:
            continue
        dx, dy = f32(r["anchorB"][0] - r["anchorA"][0]), f32(r["anchorB"][1] - r["anchorA"][1])
        g = f32(f32(dx * dx) + f32(dy * dy))
        if g > best:  # (ascending slots: a tie keeps the lower one; a NaN compares false)
            best, best_slot = g, int(r["slot"])
    out["maxGapSquared"], out["maxGapSlot"] = best, best_slot
    return out
