"""The step metrics of include/solver2d_amd.h (s2amd_world_set_metrics, s2amd_world_metrics, s2amd_world_metrics_history) stated in numpy on
a wire world dict as tests/world_chain.py keeps it: what the device's reduction (solver2d_amd/csrc/step_metrics.hip) must return, byte for
byte.  Everything is float32 with one rounding per operation in the order the header states; every float sum has the one shape `psum`.
`record(world, params, flags, step)` is the s2amdStepMetrics of a step that left `world`.  Test infrastructure only."""
import numpy as np

from solver2d_amd import wire

f32 = np.float32
TILE = 256
LINEAR_SLOP = f32(0.005)  # s2_linearSlop


def psum(terms):
    """PSUM: tiles of 256 consecutive slots, the last padded with +0; inside a tile eight rounds of x[0::2] + x[1::2]; the tile sums added
    left to right from +0."""
    terms = np.asarray(terms, dtype=f32)
    tiles = (len(terms) + TILE - 1) // TILE
    x = np.zeros(tiles * TILE, dtype=f32)
    x[: len(terms)] = terms
    x = x.reshape(tiles, TILE)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(8):
            x = x[:, 0::2] + x[:, 1::2]
            assert x.dtype == f32
        acc = f32(0)
        for t in x[:, 0] if tiles else []:
            acc = f32(acc + t)
    return acc


def _transform(origins, rot, idx, p):
    """s2TransformPoint of the points p[k] by body idx[k] (include/solver2d/math.h:350-356), rot = {s, c}"""
    s, c = rot[idx, 0], rot[idx, 1]
    x = (c * p[:, 0] - s * p[:, 1]) + origins[idx, 0]
    y = (s * p[:, 0] + c * p[:, 1]) + origins[idx, 1]
    assert x.dtype == f32 and y.dtype == f32
    return x, y


def _point_velocity(bodies, idx, anchor):
    b = bodies[idx]
    a = anchor - b["localCenter"]
    s, c = b["rot"][:, 0], b["rot"][:, 1]
    rx, ry = c * a[:, 0] - s * a[:, 1], s * a[:, 0] + c * a[:, 1]
    w, v = b["angularVelocity"], b["linearVelocity"]
    ux, uy = v[:, 0] - w * ry, v[:, 1] + w * rx
    assert ux.dtype == f32 and uy.dtype == f32
    return ux, uy


def touching_slots(world):
    """pair slot live, pointCount > 0, both bodies inside the body array"""
    contacts, nb = world["contacts"], len(world["bodies"])
    a, b = contacts["bodyA"], contacts["bodyB"]
    ok = (world["pairs"]["shapeA"] >= 0) & (contacts["pointCount"] > 0) & (a >= 0) & (a < nb) & (b >= 0) & (b < nb)
    return np.flatnonzero(ok)


def contact_points(world):
    """(slot, point index, gap, vn, normalImpulse) of every point of every touching slot, ascending by slot then point"""
    contacts, bodies = world["contacts"], world["bodies"]
    origins = np.ascontiguousarray(np.asarray(world["origins"], dtype=f32).reshape(-1, 2))
    rot = np.ascontiguousarray(bodies["rot"])
    slots = touching_slots(world)
    count = np.minimum(contacts["pointCount"][slots], 2)
    slot = np.concatenate([slots, slots[count == 2]])
    point = np.concatenate([np.zeros(len(slots), dtype=np.int64), np.ones(int((count == 2).sum()), dtype=np.int64)])
    order = np.lexsort((point, slot))
    slot, point = slot[order], point[order]
    c = contacts[slot]
    p = c["points"][np.arange(len(slot)), point] if len(slot) else c["points"][:, 0]
    a, b, n = c["bodyA"], c["bodyB"], c["normal"]
    with np.errstate(invalid="ignore", over="ignore"):
        ax, ay = _transform(origins, rot, a, p["localAnchorA"])
        bx, by = _transform(origins, rot, b, p["localAnchorB"])
        dx, dy = bx - ax, by - ay
        gap = (dx * n[:, 0] + dy * n[:, 1]) + p["separation"]
        uax, uay = _point_velocity(bodies, a, p["localAnchorA"])
        ubx, uby = _point_velocity(bodies, b, p["localAnchorB"])
        ex, ey = ubx - uax, uby - uay
        vn = ex * n[:, 0] + ey * n[:, 1]
    assert gap.dtype == f32 and vn.dtype == f32
    return slot, point, gap, vn, p["normalImpulse"].astype(f32)


def _first_best(values, slots, larger):
    """(value, slot) of the smallest (larger: largest) value that is a number; the first of equal ones, so the lowest slot and inside a slot
    the lower point (argmin / argmax return the first occurrence); (+0, -1) with none"""
    values, slots = np.asarray(values, dtype=f32), np.asarray(slots)
    number = ~np.isnan(values)
    values, slots = values[number], slots[number]
    if len(values) == 0:
        return f32(0), -1
    k = int(np.argmax(values) if larger else np.argmin(values))
    return values[k], int(slots[k])


def contact_section(world, out):
    contacts = world["contacts"]
    slot, point, gap, vn, impulse = contact_points(world)
    out["touchingContacts"], out["touchingPoints"] = len(touching_slots(world)), len(slot)
    with np.errstate(invalid="ignore"):
        out["penetratingPoints"] = int((gap < -LINEAR_SLOP).sum())
        approaching = vn < 0
        pen = np.where(gap < 0, -gap, f32(0)).astype(f32)
    out["approachingPoints"] = int(approaching.sum())
    out["minGap"], out["minGapSlot"] = _first_best(gap, slot, larger=False)
    out["maxApproachSpeed"], out["maxApproachSlot"] = _first_best(-vn[approaching], slot[approaching], larger=True)
    # a slot's term: p0, or p0 + p1 (one add)
    pen_terms, imp_terms = np.zeros(len(contacts), dtype=f32), np.zeros(len(contacts), dtype=f32)
    first, second = point == 0, point == 1
    pen_terms[slot[first]], imp_terms[slot[first]] = pen[first], impulse[first]
    with np.errstate(invalid="ignore", over="ignore"):
        pen_terms[slot[second]] = pen_terms[slot[second]] + pen[second]
        imp_terms[slot[second]] = imp_terms[slot[second]] + impulse[second]
    out["sumPenetration"], out["sumNormalImpulse"] = psum(pen_terms), psum(imp_terms)


def body_terms(world, gravity):
    """(counted, kinetic, potential, px, py, spin) per body slot; +0 for a slot that is free or static"""
    b = world["bodies"]
    counted = (b["type"] != wire.BODY_FREE) & (b["type"] != wire.BODY_STATIC)
    gx, gy = f32(gravity[0]), f32(gravity[1])
    v, w, pos = b["linearVelocity"], b["angularVelocity"], b["position"]
    half = f32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        kinetic = ((half * b["mass"]) * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])) + ((half * b["I"]) * (w * w))
        potential = -((b["mass"] * b["gravityScale"]) * (gx * pos[:, 0] + gy * pos[:, 1]))
        px, py = b["mass"] * v[:, 0], b["mass"] * v[:, 1]
        spin = b["I"] * w
    terms = [np.where(counted, t, f32(0)).astype(f32) for t in (kinetic, potential, px, py, spin)]
    for t, raw in zip(terms, (kinetic, potential, px, py, spin)):
        assert raw.dtype == f32
    return [counted] + terms


def body_section(world, gravity, out):
    counted, kinetic, potential, px, py, spin = body_terms(world, gravity)
    out["energyBodies"] = int(counted.sum())
    out["kineticEnergy"], out["potentialEnergy"] = psum(kinetic), psum(potential)
    out["momentum"] = (psum(px), psum(py))
    out["spin"] = psum(spin)


def joint_gaps(world):
    """(revolute mask, g per joint slot): the squared anchor gap; a body outside the array stands at the origin, unrotated"""
    joints, bodies = world["joints"], world["bodies"]
    nb = len(bodies)
    origins = np.concatenate([np.asarray(world["origins"], dtype=f32).reshape(-1, 2), np.zeros((1, 2), dtype=f32)])
    rot = np.concatenate([bodies["rot"].astype(f32).reshape(-1, 2), np.array([[0.0, 1.0]], dtype=f32)])
    revolute = joints["type"] == wire.JOINT_REVOLUTE
    a = np.where((joints["bodyA"] >= 0) & (joints["bodyA"] < nb), joints["bodyA"], nb)
    b = np.where((joints["bodyB"] >= 0) & (joints["bodyB"] < nb), joints["bodyB"], nb)
    with np.errstate(invalid="ignore", over="ignore"):
        ax, ay = _transform(origins, rot, a, joints["localOriginAnchorA"])
        bx, by = _transform(origins, rot, b, joints["localOriginAnchorB"])
        dx, dy = bx - ax, by - ay
        g = dx * dx + dy * dy
    assert g.dtype == f32
    return revolute, g


def joint_section(world, out):
    revolute, g = joint_gaps(world)
    out["revoluteJoints"] = int(revolute.sum())
    # the rule of tests/joint_report_ref.py: summary -- from (-1, -1), ascending slots, `g > best`: a tie keeps the lower slot, a NaN never wins
    with np.errstate(invalid="ignore"):
        slots = np.flatnonzero(revolute & (g > f32(-1.0)))
    best, best_slot = f32(-1.0), -1
    if len(slots):
        best_slot = int(slots[np.argmax(g[slots])])
        best = g[best_slot]
    out["maxJointGapSquared"], out["maxJointGapSlot"] = best, best_slot
    out["sumJointGapSquared"] = psum(np.where(revolute, g, f32(0)).astype(f32))


def record(world, params, flags, step):
    """One s2amdStepMetrics: `world` as the step left it, `params` the step's wire.StepParams, `step` the records written before it."""
    out = np.zeros(1, dtype=wire.step_metrics_dtype)[0]
    out["step"], out["flags"], out["solverType"], out["dt"] = step, flags, int(params.solverType), f32(params.dt)
    if flags & wire.METRICS_CONTACTS:
        contact_section(world, out)
    if flags & wire.METRICS_BODIES:
        body_section(world, (params.gravity[0], params.gravity[1]), out)
    if flags & wire.METRICS_JOINTS:
        joint_section(world, out)
    return out


def same_record(got, want):
    """byte for byte, except that of a float sum that is a NaN only "is a NaN" is stated"""
    got, want = np.array([got], dtype=wire.step_metrics_dtype), np.array([want], dtype=wire.step_metrics_dtype)
    for name in ("sumPenetration", "sumNormalImpulse", "kineticEnergy", "potentialEnergy", "momentum", "spin", "sumJointGapSquared"):
        both = np.isnan(got[name]) & np.isnan(want[name])
        got[name][both], want[name][both] = 0, 0
    return got.tobytes() == want.tobytes()
