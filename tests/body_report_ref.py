"""The body report of include/solver2d_amd.h (s2amd_world_set_body_report, s2amd_world_set_rest_thresholds and their getters) stated in
numpy on a wire world dict as tests/world_chain.py keeps it: what the device's passes (solver2d_amd/csrc/body_report.hip) must return,
byte for byte.  Everything is float32 with one rounding per operation; the angle goes through glibc's atan2f (tests/joint_report_ref.py).

The report has a state of its own -- the pose copy and the timers -- so the statement has one: `new_state(world)` is the state after an
upload or after the flags went from 0 to non-zero, `advance(state, world, thresholds, dt)` is one reporting step on the world as it stands
after the step and returns what that step saw.  Test infrastructure only."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from solver2d_amd import wire
from tests.joint_report_ref import atan2f

f32 = np.float32
DEFAULT_THRESHOLDS = (f32(0.01), f32(0.0349065850), f32(0.5))
MOVED, AT_REST, ISLAND_AT_REST = 1, 2, 4


def reported(bodies):
    return (bodies["type"] != wire.BODY_FREE) & (bodies["type"] != wire.BODY_STATIC)


def movable(bodies):
    return reported(bodies) & ((bodies["invMass"] != 0) | (bodies["invI"] != 0))


def pose_of(world):
    """{origin.x, origin.y, rot.s, rot.c} of every slot as four uint32"""
    origins = np.asarray(world["origins"], dtype=f32).reshape(-1, 2)
    both = np.concatenate([origins, world["bodies"]["rot"].astype(f32)], axis=1)
    return np.ascontiguousarray(both).view(np.uint32).copy()


def new_state(world):
    return {"pose": pose_of(world), "timer": np.zeros(len(world["bodies"]), dtype=f32)}


def advance(state, world, thresholds, dt):
    """One reporting step: per slot `moved`, `before`, `now` (at rest), `timer`, `speed2`; the state moves on."""
    bodies = world["bodies"]
    lin, ang, seconds = (f32(t) for t in thresholds)
    lin2, ang2 = f32(lin * lin), f32(ang * ang)
    rep = reported(bodies)
    pose = pose_of(world)
    moved = rep & (pose != state["pose"]).any(axis=1)
    v, w = bodies["linearVelocity"].astype(f32), bodies["angularVelocity"].astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        speed2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
        ww = w * w
        assert speed2.dtype == f32 and ww.dtype == f32
        candidate = (speed2 <= lin2) & (ww <= ang2)  # a NaN fails
        old = state["timer"]
        before = rep & (old >= seconds)
        timer = np.where(rep, np.where(candidate, old + f32(dt), f32(0)), old).astype(f32)
    now = rep & (timer >= seconds)
    state["pose"], state["timer"] = pose, timer
    return {"moved": moved, "before": before, "now": now, "timer": timer, "speed2": speed2.astype(f32), "reported": rep}


def events(step):
    """(rested, woke) slot lists, ascending"""
    return (np.flatnonzero(step["now"] & ~step["before"]).astype(np.int32), np.flatnonzero(step["before"] & ~step["now"]).astype(np.int32))


def fastest(slots, speed2):
    """(slot, speed) of the largest speed2 among `slots` (ascending): of equal ones the lowest slot, a NaN never wins; (-1, -1.0) for none"""
    best, best_v = -1, f32(-1.0)
    for i in slots:
        if speed2[i] > best_v:
            best, best_v = int(i), speed2[i]
    return best, best_v


def island_labels(world):
    """island index per body slot (-1: not reported) and the island count: the rule of solver2d_amd/islands.py: find_islands, with edges
    that name a body outside the array joining nothing."""
    bodies, contacts, joints = world["bodies"], world["contacts"], world["joints"]
    nb = len(bodies)
    mov, rep = movable(bodies), reported(bodies)
    ea, eb = [], []
    for a, b in ((contacts["bodyA"][contacts["pointCount"] > 0], contacts["bodyB"][contacts["pointCount"] > 0]),
                 (joints["bodyA"][joints["type"] == wire.JOINT_REVOLUTE], joints["bodyB"][joints["type"] == wire.JOINT_REVOLUTE])):
        a, b = a.astype(np.int64), b.astype(np.int64)
        ok = (a >= 0) & (a < nb) & (b >= 0) & (b < nb)
        a, b = a[ok], b[ok]
        both = mov[a] & mov[b]
        ea.append(a[both])
        eb.append(b[both])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    _n, label = connected_components(coo_matrix((np.ones(len(ea), dtype=np.int8), (ea, eb)), shape=(nb, nb)), directed=False)
    island = np.full(nb, -1, dtype=np.int32)
    seen = {}
    for i in np.flatnonzero(rep):  # ascending: an island's number is the rank of its lowest slot
        island[i] = seen.setdefault(int(label[i]), len(seen))
    return island, len(seen)


def _owner(mov, nb, a, b):
    """the body an edge counts for: a when it is movable, else b when it is, else -1 (a slot outside the array is not movable)"""
    def ok(x):
        return 0 <= x < nb and bool(mov[x])
    return a if ok(a) else b if ok(b) else -1


def islands(world, step):
    """(island per slot, s2amdIslandState records)"""
    bodies, contacts, joints = world["bodies"], world["contacts"], world["joints"]
    nb = len(bodies)
    island, count = island_labels(world)
    mov = movable(bodies)
    out = np.zeros(count, dtype=wire.island_state_dtype)
    for k in range(count):
        slots = np.flatnonzero(island == k)
        out[k]["firstBody"], out[k]["bodyCount"] = slots[0], len(slots)
        out[k]["restingBodies"] = int(step["now"][slots].sum())
        out[k]["minRestTime"] = step["timer"][slots].min()
        out[k]["fastestBody"], out[k]["maxSpeedSquared"] = fastest(slots, step["speed2"])
    for c in contacts[contacts["pointCount"] > 0]:
        o = _owner(mov, nb, int(c["bodyA"]), int(c["bodyB"]))
        if o >= 0:
            out[island[o]]["contactCount"] += 1
    for j in joints[joints["type"] != wire.JOINT_FREE]:
        o = _owner(mov, nb, int(j["bodyA"]) if j["type"] == wire.JOINT_REVOLUTE else -1, int(j["bodyB"]))
        if o >= 0:
            out[island[o]]["jointCount"] += 1
    return island, out


def states(world, step, moved_only=False, island=None, island_states=None):
    """s2amdBodyState of every reported body (moved_only: that moved), ascending; island / island_states: of `islands`, None without ISLANDS"""
    bodies = world["bodies"]
    listed = step["reported"] & (step["moved"] if moved_only else True)
    slots = np.flatnonzero(listed)
    b = bodies[slots]
    out = np.zeros(len(slots), dtype=wire.body_state_dtype)
    out["slot"], out["type"] = slots, b["type"]
    out["origin"] = np.asarray(world["origins"], dtype=f32).reshape(-1, 2)[slots]
    out["position"], out["rot"] = b["position"], b["rot"]
    out["angle"] = [atan2f(r[0], r[1]) for r in b["rot"]]
    out["angularVelocity"], out["linearVelocity"] = b["angularVelocity"], b["linearVelocity"]
    out["restTime"], out["speedSquared"] = step["timer"][slots], step["speed2"][slots]
    flags = np.where(step["moved"][slots], MOVED, 0) | np.where(step["now"][slots], AT_REST, 0)
    if island is None:
        out["island"] = -1
    else:
        out["island"] = island[slots]
        resting = island_states["restingBodies"] == island_states["bodyCount"]
        flags = flags | np.where(resting[island[slots]], ISLAND_AT_REST, 0)
    out["flags"] = flags
    return out


def summary(world, step, island_states=None):
    """s2amdBodySummary; island_states None: without ISLANDS"""
    bodies = world["bodies"]
    rep = step["reported"]
    out = np.zeros(1, dtype=wire.body_summary_dtype)[0]
    out["bodies"] = int(rep.sum())
    out["dynamicBodies"], out["kinematicBodies"] = int((bodies["type"] == wire.BODY_DYNAMIC).sum()), int((bodies["type"] == wire.BODY_KINEMATIC).sum())
    out["movedBodies"], out["restingBodies"] = int(step["moved"].sum()), int(step["now"].sum())
    out["largestIsland"] = -1
    if island_states is not None and len(island_states):
        out["islands"] = len(island_states)
        out["restingIslands"] = int((island_states["restingBodies"] == island_states["bodyCount"]).sum())
        out["largestIsland"] = int(np.argmax(island_states["bodyCount"]))  # (argmax: the lowest index among equals)
        out["largestIslandBodies"] = int(island_states["bodyCount"].max())
    out["fastestBody"], out["maxSpeedSquared"] = fastest(np.flatnonzero(rep), step["speed2"])
    return out
