"""The statement of the observers (include/solver2d_amd.h: s2amd_world_set_observers, s2amd_world_set_observation_report,
s2amd_world_observations, s2amd_world_export_observations, s2amd_world_observer_states, s2amd_world_observer_counts), restated in numpy
for the tests.  Test infrastructure only.

An observer reads its target after the step, forms its raw value x -- float32 scalar by scalar, every product, sum and difference rounded
on its own, the five functions of include/solver2d/math.h restated operation for operation, atan2f through glibc as
tests/joint_report_ref.py takes it -- and its value y = clamp(gain * x + bias), the actuators' command rule.  A world is a dict with
"bodies", "joints" and "origins" (the keys of tests/world_chain.py); observers are wire.observer_dtype records; `sources` is
(body sums: wire.body_contact_sum_dtype per body slot, ranges: float32 per ray, actions: float32 per action channel), each None when its
source is off, and `lengths` = (rays of the ray list, channels of the actuator list), 0 with no such list."""
import numpy as np

from solver2d_amd import wire
from tests import actuator_ref, joint_report_ref

F = np.float32
OBSERVED, DISABLED, SKIPPED, SOURCE_OFF = 0, 1, 2, 3
POINT, ROTATION, ANGLE, LINEAR, ANGULAR, REV_ANGLE, REV_SPEED, REV_IMPULSE, CONTACT, RAY, ACTION = range(1, 12)


def transform_point(origin, rot, p):
    """s2TransformPoint (math.h:350-356), rot = {s, c}"""
    ox, oy, s, c, px, py = F(origin[0]), F(origin[1]), F(rot[0]), F(rot[1]), F(p[0]), F(p[1])
    return F(F(F(c * px) - F(s * py)) + ox), F(F(F(s * px) + F(c * py)) + oy)


def inv_rotate_vector(rot, v):
    """s2InvRotateVector (math.h:344-347): {c * v.x + s * v.y, -s * v.x + c * v.y}"""
    s, c, vx, vy = F(rot[0]), F(rot[1]), F(v[0]), F(v[1])
    return F(F(c * vx) + F(s * vy)), F(F(F(-s) * vx) + F(c * vy))


def sub(a, b):
    """s2Sub (math.h:91-94)"""
    return F(F(a[0]) - F(b[0])), F(F(a[1]) - F(b[1]))


def inv_transform_point(origin, rot, p):
    """s2InvTransformPoint (math.h:359-364)"""
    return inv_rotate_vector(rot, sub(p, origin))


def inv_mul_rot(b, a):
    """s2InvMulRot(b, a) (math.h:307-317) -> {s, c}"""
    bs, bc, as_, ac = F(b[0]), F(b[1]), F(a[0]), F(a[1])
    return F(F(bc * as_) - F(bs * ac)), F(F(bc * ac) + F(bs * as_))


def valid(observers, channels, frames):
    """What the host checks before anything is replaced: -1, or the index of the first invalid record (for an overlap: the later one in
    channel order)."""
    if len(observers) > wire.MAX_OBSERVERS:
        return 0
    if len(observers) and not (1 <= channels <= wire.MAX_OBSERVATION_CHANNELS and 1 <= frames <= wire.MAX_OBSERVATION_FRAMES):
        return 0
    for i, o in enumerate(observers):
        kind = int(o["kind"])
        if not 1 <= kind <= 11 or o["target"] < 0 or o["frame"] < -1 or (kind >= REV_ANGLE and o["frame"] != -1):
            return i
        if o["channel"] < 0 or int(o["channel"]) + wire.OBSERVER_WIDTH[kind] > channels:
            return i
        if int(o["flags"]) & ~(wire.OBSERVER_DISABLED | wire.OBSERVER_RELATIVE) or o["reserved"].any():
            return i
        if not all(np.isfinite(x) for x in (o["gain"], o["bias"], o["local"][0], o["local"][1])) or not o["lower"] <= o["upper"]:
            return i
    order = sorted(range(len(observers)), key=lambda i: int(observers["channel"][i]))
    for before, after in zip(order, order[1:]):
        if int(observers["channel"][before]) + wire.OBSERVER_WIDTH[int(observers["kind"][before])] > int(observers["channel"][after]):
            return after
    return -1


def raw(world, o, sources, lengths):
    """-> (status, [x_0 .. x_width-1]) of one observer"""
    bodies, joints, origins = world["bodies"], world["joints"], np.asarray(world["origins"], dtype=F).reshape(-1, 2)
    sums, ranges, actions = sources
    kind, target, frame, flags = int(o["kind"]), int(o["target"]), int(o["frame"]), int(o["flags"])

    def live(body):
        return 0 <= body < len(bodies) and bodies["type"][body] != wire.BODY_FREE

    if flags & wire.OBSERVER_DISABLED:
        return DISABLED, []
    if kind <= ANGULAR:
        framed = frame >= 0
        if not live(target) or (framed and not live(frame)):
            return SKIPPED, []
        b, f = bodies[target], bodies[frame] if framed else None
        relative = framed and flags & wire.OBSERVER_RELATIVE
        if kind == POINT:
            p = transform_point(origins[target], b["rot"], o["local"])
            return OBSERVED, list(inv_transform_point(origins[frame], f["rot"], p) if framed else p)
        if kind in (ROTATION, ANGLE):
            q = inv_mul_rot(f["rot"], b["rot"]) if framed else (F(b["rot"][0]), F(b["rot"][1]))
            return OBSERVED, list(q) if kind == ROTATION else [joint_report_ref.atan2f(q[0], q[1])]
        if kind == LINEAR:
            v = sub(b["linearVelocity"], f["linearVelocity"]) if relative else (F(b["linearVelocity"][0]), F(b["linearVelocity"][1]))
            return OBSERVED, list(inv_rotate_vector(f["rot"], v) if framed else v)
        w = F(b["angularVelocity"])
        return OBSERVED, [F(w - F(f["angularVelocity"])) if relative else w]
    if kind <= REV_IMPULSE:
        if target >= len(joints) or joints["type"][target] != wire.JOINT_REVOLUTE:
            return SKIPPED, []
        j = joints[target]
        if kind == REV_ANGLE:
            return OBSERVED, [actuator_ref.servo_angle(world, target)]  # the joint report's angle: a body outside the array is unrotated
        if kind == REV_SPEED:
            w = [F(bodies["angularVelocity"][k]) if 0 <= k < len(bodies) else F(0.0) for k in (int(j["bodyA"]), int(j["bodyB"]))]
            return OBSERVED, [F(w[1] - w[0])]
        return OBSERVED, [F(j["motorImpulse"])]
    if kind == CONTACT:
        if not live(target):
            return SKIPPED, []
        if sums is None:
            return SOURCE_OFF, []
        return OBSERVED, [F(1.0) if sums["touching"][target] > 0 else F(0.0), F(sums["normalImpulse"][target])]
    length = lengths[0] if kind == RAY else lengths[1]
    source = ranges if kind == RAY else actions
    if length > 0 and target >= length:
        return SKIPPED, []
    if source is None or length == 0:
        return SOURCE_OFF, []
    return OBSERVED, [F(source[target])]


def observe(world, observers, sources, channels=None, lengths=None):
    """-> (vector: float32[channels] of this step, states: wire.observer_state_dtype per observer, counts: int32[4] per status).
    `lengths` defaults to the lengths of the sources given."""
    sums, ranges, actions = sources
    if lengths is None:
        lengths = (0 if ranges is None else len(ranges), 0 if actions is None else len(actions))
    if channels is None:
        channels = max([int(o["channel"]) + wire.OBSERVER_WIDTH[int(o["kind"])] for o in observers] + [1])
    vector = np.zeros(channels, dtype=F)
    states = np.zeros(len(observers), dtype=wire.observer_state_dtype)
    counts = np.zeros(4, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i, o in enumerate(observers):
            status, x = raw(world, o, sources, lengths)
            st = states[i]
            st["observer"], st["status"] = i, status
            counts[status] += 1
            width = wire.OBSERVER_WIDTH[int(o["kind"])]
            y = [actuator_ref.command(v, o["gain"], o["bias"], o["lower"], o["upper"]) for v in x] if status == OBSERVED else [F(0.0)] * width
            st["raw"][:len(x)], st["value"][:len(y)] = x, y
            vector[int(o["channel"]):int(o["channel"]) + width] = y
    return vector, states, counts


class History:
    """The ring, restated: frame 0 is the last reporting step, frame k the k-th before it; the first reporting step after a re-base
    (an upload, a new list, the flags from 0 to non-zero) fills every frame; a step with the flags at 0 is none."""

    def __init__(self, frames, channels):
        self.rows = np.zeros((frames, channels), dtype=F)
        self.fresh = True

    def rebase(self):
        self.fresh = True

    def push(self, vector):
        """One reporting step -> float32[frames][channels], newest first"""
        if self.fresh:
            self.rows[:] = vector
        else:
            self.rows[1:] = self.rows[:-1].copy()
            self.rows[0] = vector
        self.fresh = False
        return self.rows.copy()
