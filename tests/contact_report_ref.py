"""The contact report of include/solver2d_amd.h (s2amd_world_set_report and its getters) stated in numpy on a wire world dict as
tests/world_chain.py keeps it: what the device's compaction (solver2d_amd/csrc/contact_report.hip) must return, byte for byte.
Test infrastructure only."""
import numpy as np

from solver2d_amd import wire

f32 = np.float32


def touching_mask(world):
    """A slot touches when its pair slot is live and its manifold has points."""
    return (world["pairs"]["shapeA"] >= 0) & (world["contacts"]["pointCount"] > 0)


def before_of(contacts):
    """The "before" state of slots as uploaded or written by the caller: pointCount > 0 of the records."""
    return np.asarray(contacts["pointCount"]) > 0


def events(prev_touching, world):
    """(began, ended) slot lists, ascending, of a step that took the slots from `prev_touching` to the state of `world`."""
    now = touching_mask(world)
    prev = np.asarray(prev_touching, dtype=bool)
    return np.flatnonzero(now & ~prev).astype(np.int32), np.flatnonzero(prev & ~now).astype(np.int32)


def touching(world):
    """s2amdTouchingContact of every touching slot, ascending: point[j] = s2TransformPoint({origin, rot} of bodyA, localAnchorA) in
    float32, one rounding per operation, in the order of include/solver2d/math.h:350-356."""
    slots = np.flatnonzero(touching_mask(world))
    c, p = world["contacts"][slots], world["pairs"][slots]
    out = np.zeros(len(slots), dtype=wire.touching_contact_dtype)
    out["slot"], out["bodyA"], out["bodyB"] = slots, c["bodyA"], c["bodyB"]
    out["pointCount"] = c["pointCount"]
    out["normal"] = c["normal"]
    origins = np.asarray(world["origins"], dtype=f32)
    ox, oy = origins[c["bodyA"], 0], origins[c["bodyA"], 1]
    rot = world["bodies"]["rot"][c["bodyA"]]
    qs, qc = rot[:, 0].astype(f32), rot[:, 1].astype(f32)
    for j in range(2):
        used = c["pointCount"] > j
        pt = c["points"][:, j]
        px, py = pt["localAnchorA"][:, 0], pt["localAnchorA"][:, 1]
        x = (qc * px - qs * py) + ox
        y = (qs * px + qc * py) + oy
        assert x.dtype == f32 and y.dtype == f32
        out["point"][:, j, 0] = np.where(used, x, f32(0))
        out["point"][:, j, 1] = np.where(used, y, f32(0))
        out["persisted"][:, j] = np.where(used, p["persisted"][:, j], 0)
        for name in ("separation", "normalImpulse", "tangentImpulse"):
            out[name][:, j] = np.where(used, pt[name], f32(0))
    return out


def body_sums(world):
    """s2amdBodyContactSum per body slot: a plain loop of float32 adds from +0 over the touching contacts in slot order, points in
    index order; P = s2Add(s2MulSV(normalImpulse, normal), s2MulSV(tangentImpulse, s2RightPerp(normal))) (src/solve_common.c:304-314),
    -P for bodyA, +P for bodyB."""
    nb = len(world["bodies"])
    ix, iy, nn = [f32(0)] * nb, [f32(0)] * nb, [f32(0)] * nb
    count = [0] * nb
    contacts = world["contacts"]
    for k in np.flatnonzero(touching_mask(world)).tolist():
        c = contacts[k]
        a, b = int(c["bodyA"]), int(c["bodyB"])
        nx, ny = f32(c["normal"][0]), f32(c["normal"][1])
        tx, ty = ny, -nx  # s2RightPerp
        count[a] += 1
        count[b] += 1
        for j in range(int(c["pointCount"])):
            ni, ti = f32(c["points"][j]["normalImpulse"]), f32(c["points"][j]["tangentImpulse"])
            px = f32(f32(ni * nx) + f32(ti * tx))
            py = f32(f32(ni * ny) + f32(ti * ty))
            ix[a], iy[a], nn[a] = f32(ix[a] + (-px)), f32(iy[a] + (-py)), f32(nn[a] + ni)
            ix[b], iy[b], nn[b] = f32(ix[b] + px), f32(iy[b] + py), f32(nn[b] + ni)
    out = np.zeros(nb, dtype=wire.body_contact_sum_dtype)
    out["impulse"][:, 0], out["impulse"][:, 1] = np.array(ix, dtype=f32), np.array(iy, dtype=f32)
    out["normalImpulse"] = np.array(nn, dtype=f32)
    out["touching"] = count
    return out
