"""The worlds and grid lists of the grid report's tests.  Test infrastructure only.

The three scenes are tests/sensor_report_world.py's (a falling ball, a base-3 pyramid with a flyer, a six-link chain) with distinct
category bits per shape slot, each under eight grids: a fixed 16 x 16 grid of 0.25 m cells turned by 0.3 rad, the same grid mounted on
the moving body (ball, flyer, last link) and centred on it -- the cells inside its own shape read what lies behind, or nothing --, one
on a static body with SKIP_STATIC, a copy of the first with SKIP_STATIC, a DISABLED copy of the first, a 7 x 5 grid, a 1 x 1 grid, and a copy of the
first whose mask passes only some categories.

tests/golden/grid_report/<scene>.npz (python -m tests.grid_report_world writes them; data only) hold the world, the grids and, per step
of the oracle chain, the SHAPES and CATEGORIES images, the SHAPES image without the exclusions, the active grids and the robust mask: a
cell is robust when its values are unchanged with the grid's position displaced by 1 mm along +-x and +-y of its own frame, and with
the chain stepped in other sweep orders (run_statement says why).
build_fixture refuses a scene that fails the condition: at least 95 % of the cells of the active grids robust per step, at least one
robust cell in every active grid of more than one cell, every name of COVERAGE among robust cells."""
import os

import numpy as np

from solver2d_amd import wire
from tests import grid_report_ref, sensor_report_world as sw
from tests.resident import downloaded_world

f32 = np.float32
ALL = 0xFFFFFFFF
STEPS = sw.STEPS
SCENES = sw.SCENES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_report")
WORLD_KEYS = sw.WORLD_KEYS
CLEARANCE = 1e-3   # a robust cell keeps its values with the grid displaced by this much along +-x and +-y of its own frame
ORDER_CHAINS = 6    # further chains in other sweep orders that a robust cell must agree with (run_statement)
ROBUST_SHARE = 0.95  # ... and at least this share of the cells of the active grids is robust, per scene and step
SOME = 0b01010  # the masked grid passes categories 2 and 8
COVERAGE = ("occupied", "empty", "two shapes in one grid", "own shape hidden", "skip-static changes", "mask changes")


def make_grid(position, angle, cell_size, width, height, body=-1, flags=0, mask=ALL):
    q = np.zeros(1, dtype=wire.grid_sensor_dtype)[0]
    q["position"], q["rot"] = position, (np.sin(angle), np.cos(angle))
    q["cellSize"], q["width"], q["height"] = cell_size, width, height
    q["maskBits"], q["body"], q["flags"] = mask, body, flags
    return q


# per scene: the centre of the fixed grids, the moving body, the static body and where the grid on it is centred (in its frame), the 1 x 1
# cell, and where the grid on the moving body is centred (the chain's: half a cell off, so that a row of cell centres lies on the axis of
# the link's capsule, which is thinner than a cell)
_PLACES = {
    "ball": ((0.3, 1.9), 1, 0, (0.4, 1.6), (0.0, 0.1), (0.0, 0.0)),
    "pyramid": ((0.2, 1.4), None, 0, (0.0, 1.5), (0.0, 0.5), (0.0, 0.0)),
    "chain": ((1.646, 4.3316), 6, 0, (1.5, -1.5), (0.0, 5.0), (0.125, 0.125)),
}


def scene(name):
    """-> (world, grids)"""
    world, _ = sw.BUILDERS[name]()
    shapes = world["shapes"]
    live = np.flatnonzero(shapes["type"] != wire.SHAPE_FREE)
    shapes["categoryBits"][live] = (1 << (live % 5)).astype(np.uint32)  # (no pair is made in the chain: the filter is not read again)
    centre, mover, static, on_static, single, on_mover = _PLACES[name]
    if mover is None:
        mover = len(world["bodies"]) - 2  # the pyramid's flyer
    assert world["bodies"]["type"][mover] == wire.BODY_DYNAMIC and world["bodies"]["type"][static] == wire.BODY_STATIC
    fixed = make_grid(centre, 0.3, 0.25, 16, 16)
    off, masked, skipping = fixed.copy(), fixed.copy(), fixed.copy()
    skipping["flags"] = wire.GRID_SENSOR_SKIP_STATIC
    off["flags"] = wire.GRID_SENSOR_DISABLED
    masked["maskBits"] = SOME
    grids = np.array([
        fixed,
        make_grid(on_mover, 0.0, 0.25, 16, 16, body=mover),
        make_grid(on_static, 0.1, 0.25, 16, 16, body=static, flags=wire.GRID_SENSOR_SKIP_STATIC),
        skipping,
        off,
        make_grid(centre, 0.0, 0.5, 7, 5),
        make_grid(single, 0.0, 0.25, 1, 1),
        masked,
    ], dtype=wire.grid_sensor_dtype)
    return world, grids


def images(grids, array):
    first = np.cumsum(grids["width"] * grids["height"]) - grids["width"] * grids["height"]
    return [array[first[g]: first[g] + int(q["width"]) * int(q["height"])].reshape(int(q["height"]), int(q["width"])) for g, q in enumerate(grids)]


def displaced(grids, dx, dy):
    """Every grid's position moved by (dx, dy) of its own frame (the frame the position is given in, turned by the grid's rot)"""
    out = grids.copy()
    s, c = grids["rot"][:, 0].astype(np.float64), grids["rot"][:, 1].astype(np.float64)
    out["position"][:, 0] = (grids["position"][:, 0] + (c * dx - s * dy)).astype(np.float32)
    out["position"][:, 1] = (grids["position"][:, 1] + (s * dx + c * dy)).astype(np.float32)
    return out


def variations(grids):
    c = float(CLEARANCE)
    return [displaced(grids, c, 0.0), displaced(grids, -c, 0.0), displaced(grids, 0.0, c), displaced(grids, 0.0, -c)]


def robust_report(world, grids, exclusions=True):
    """The statement's (categories, shapes, occupancy, states) and the robust mask: the cells whose SHAPES and CATEGORIES values are
    those of the four variations as well"""
    from tests import grid_report_ref as ref
    got = ref.report(world, grids, exclusions)
    robust = np.ones(len(got[1]), dtype=bool)
    for other in variations(grids):
        cats, low, _, _ = ref.report(world, other, exclusions)
        robust &= (cats == got[0]) & (low == got[1])
    return got, robust


def _step_in_order(params, w, rng):
    """One step of the oracle chain with the active contacts and the joints swept in another order: reversed (rng None) or shuffled"""
    from tests import world_chain
    active = np.flatnonzero(w["contacts"]["pointCount"] > 0).astype(np.int32)
    joints = np.arange(len(w["joints"]), dtype=np.int32)
    if rng is None:
        active, joints = active[::-1], joints[::-1]
    else:
        active, joints = rng.permutation(active), rng.permutation(joints)
    world_chain.oracle_world_step(params, w, contact_order=np.ascontiguousarray(active, dtype=np.int32), joint_order=np.ascontiguousarray(joints, dtype=np.int32))


def run_statement(world, grids, steps=STEPS):
    """The chain in pool order -> fixture entries per step k: shapes_k (the SHAPES image over all cells), categories_k, robust_k,
    active_k (per grid) and plain_k (the SHAPES image without the two exclusions).

    The world a device steps is the chain in the DEVICE's sweep orders, not in pool order, and the solvers are order sensitive: the
    six-link chain lies up to 4 mm elsewhere after a few steps.  A recorded cell can be compared with any stepped world only where the
    orders agree, so robust_k also asks that the values are those of ORDER_CHAINS further chains (reversed order, and seeded shuffles
    of the active contacts and of the joints, each chain keeping its own rule from the first step on).  This only ever takes cells out
    of the mask: the condition of 95 % robust cells is asked of what remains."""
    from tests import grid_report_ref as ref, world_chain
    w = world_chain.copy_world(world)
    others = [(world_chain.copy_world(world), None if i == 0 else np.random.RandomState(100 + i)) for i in range(ORDER_CHAINS)]
    out = {}
    p = sw.params()
    for k in range(steps):
        world_chain.oracle_world_step(p, w)
        (cats, low, _, states), robust = robust_report(w, grids)
        (_, plain, _, _), plain_robust = robust_report(w, grids, exclusions=False)
        robust &= plain_robust
        for other, rng in others:
            _step_in_order(p, other, rng)
            oc, ol, _, _ = ref.report(other, grids)
            robust &= (oc == cats) & (ol == low) & (ref.report(other, grids, exclusions=False)[1] == plain)
        out["shapes_%d" % k], out["categories_%d" % k] = low, cats
        out["robust_%d" % k] = robust.astype(np.uint8)
        out["active_%d" % k] = states["active"].astype(np.uint8)
        out["plain_%d" % k] = plain
    return out


def fixture_path(name):
    return os.path.join(GOLDEN, "%s.npz" % name)


def load_fixture(name):
    d = np.load(fixture_path(name))
    return {k: np.ascontiguousarray(d[k]) for k in d.files}


def fixture_world(fx):
    return {k: fx[k].copy() for k in WORLD_KEYS}


def coverage(fx, k):
    """The names of COVERAGE that step k of a fixture shows among its robust cells"""
    grids = fx["grids"]
    low, plain = images(grids, fx["shapes_%d" % k]), images(grids, fx["plain_%d" % k])
    ok = [m != 0 for m in images(grids, fx["robust_%d" % k])]
    seen = set()
    if (low[0][ok[0]] >= 0).any():
        seen.add("occupied")
    if (low[0][ok[0]] < 0).any():
        seen.add("empty")
    if len(set(low[0][ok[0] & (low[0] >= 0)].tolist())) >= 2:
        seen.add("two shapes in one grid")
    # a cell inside the own body's shape (without the exclusions it reads that shape) that reads another shape or nothing
    own = int(grids[1]["body"])
    inside = ok[1] & (plain[1] >= 0)
    inside[inside] = fx["shapes"]["body"][plain[1][inside]] == own
    if inside.any() and (low[1][inside] != plain[1][inside]).all():
        seen.add("own shape hidden")
    if (ok[3] & ok[0] & (low[3] != low[0])).any():
        seen.add("skip-static changes")
    if (ok[7] & ok[0] & (low[7] != low[0])).any() and (low[7][ok[7]] >= 0).any():
        seen.add("mask changes")
    return seen


def condition(fx):
    """(the least share of robust cells among the cells of active grids over the steps, the active grids of more than one cell without
    a robust cell as (step, grid) pairs, the names of COVERAGE no step shows among robust cells): from the fixture alone"""
    grids = fx["grids"]
    cells = (grids["width"] * grids["height"]).astype(np.int64)
    share, bare, seen = 1.0, [], set()
    for k in range(STEPS):
        robust, active = images(grids, fx["robust_%d" % k]), fx["active_%d" % k] != 0
        total = int(cells[active].sum())
        share = min(share, sum(int((robust[g] != 0).sum()) for g in np.flatnonzero(active)) / max(total, 1))
        bare += [(k, int(g)) for g in np.flatnonzero(active) if cells[g] > 1 and not (robust[g] != 0).any()]
        seen |= coverage(fx, k)
    return share, bare, sorted(set(COVERAGE) - seen)


def assert_condition(fx, what):
    share, bare, missing = condition(fx)
    assert share >= ROBUST_SHARE and not bare and not missing, "%s: %.4f of the cells robust, grids without a robust cell %s, not covered %s: move the grid" % (
        what, share, bare, missing)


def build_fixture(name):
    world, grids = scene(name)
    fx = {k: world[k] for k in WORLD_KEYS}
    fx["grids"] = grids
    fx.update(run_statement(world, grids))
    assert_condition(fx, name)  # (a fixture that fails the condition is not written)
    return fx


def sweep_grids(world, count):
    """`count` grids that repeat seven distinct ones over tests/sensor_report_world.sweep_world: a tall fixed grid over the first lattice
    columns (shapes of every wave of every tile), a fixed turned one, one carried by a falling body (its own shape lies under it), one on
    the ground with SKIP_STATIC, a DISABLED copy of the first, one on the free body slot, and one that passes category 2 only (nothing)."""
    bodies, shapes = world["bodies"], world["shapes"]
    at = min(70, len(shapes) - 1)
    carrier = int(shapes["body"][at]) if shapes["type"][at] != wire.SHAPE_FREE and at > 0 else -1
    tall = make_grid((1.0, 6.0), 0.0, 0.25, 8, 44)
    off = tall.copy()
    off["flags"] = wire.GRID_SENSOR_DISABLED
    distinct = [
        tall,
        make_grid((3.6, 2.5), 0.4, 0.2, 9, 11),
        make_grid((0.1, 0.0), 0.3, 0.125, 8, 8, body=carrier),
        make_grid((-2.0, 1.6), 0.0, 0.25, 12, 6, body=0, flags=wire.GRID_SENSOR_SKIP_STATIC),
        off,
        make_grid((0.0, 0.0), 0.0, 1.0, 5, 5, body=len(bodies) - 1),
        make_grid((5.0, 2.0), 0.2, 0.25, 6, 6, mask=2),
    ]
    assert bodies["type"][len(bodies) - 1] == wire.BODY_FREE
    return np.array([distinct[i % len(distinct)] for i in range(count)], dtype=wire.grid_sensor_dtype)


def edge_grids():
    """The extents at which a tile of 64 cells, an 8 x 8 block or a row ends, over the lattice of sweep_world"""
    return np.array([
        make_grid((1.0, 1.0), 0.0, 0.25, 1, 1),
        make_grid((2.0, 6.4), 0.05, 0.05, 1, 256),
        make_grid((4.0, 3.0), -0.05, 0.05, 256, 1),
        make_grid((3.0, 2.0), 0.3, 0.25, 8, 8),
        make_grid((3.0, 4.0), 0.0, 0.2, 17, 16),
        make_grid((3.5, 5.0), 0.7, 0.1, 65, 3),
        make_grid((1.5, 3.0), 0.0, 0.3, 7, 5),
    ], dtype=wire.grid_sensor_dtype)


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for name in SCENES:
        built = build_fixture(name)
        print("%s: %d grids, robust share %.4f" % (name, len(built["grids"]), condition(built)[0]))
        np.savez_compressed(fixture_path(name), **built)
        print("  %d bytes" % os.path.getsize(fixture_path(name)))


def getters(s):
    return s.world_grid_categories(), s.world_grid_shapes(), s.world_grid_occupancy(), s.world_grid_states()


def plain(world, grids):
    """Which grids the two exclusions cannot change: fixed in the world or on a body without a live shape, and no SKIP_STATIC"""
    shapes = world["shapes"]
    live_bodies = set(shapes["body"][shapes["type"] != wire.SHAPE_FREE].tolist())
    return np.array([(int(q["body"]) < 0 or int(q["body"]) not in live_bodies) and not (int(q["flags"]) & wire.GRID_SENSOR_SKIP_STATIC) for q in grids], dtype=bool)


def assert_structure(world, grids, got, what):
    """What every report satisfies whatever the geometry: sizes, the fixed fields, the states' figures from the arrays"""
    cats, low, occ, states = got
    first, total = grid_report_ref.first_cells(grids)
    assert len(cats) == len(low) == len(occ) == total and len(states) == len(grids), what
    assert states["grid"].tolist() == list(range(len(grids))) and states["body"].tobytes() == grids["body"].tobytes(), what
    assert states["firstCell"].tolist() == first.tolist() and states["cells"].tolist() == (grids["width"] * grids["height"]).tolist(), what
    assert occ.tobytes() == (low >= 0).astype(np.float32).tobytes() and ((cats != 0) == (low >= 0)).all(), what
    shapes = world["shapes"]
    hit = low >= 0
    assert (shapes["type"][low[hit]] != wire.SHAPE_FREE).all() and ((cats[hit] & shapes["categoryBits"][low[hit]]) != 0).all(), what
    for g, q in enumerate(grids):
        mine = low[first[g]: first[g] + int(q["width"]) * int(q["height"])]
        st = states[g]
        assert st["occupied"] == (mine >= 0).sum() and st["lowestShape"] == (mine[mine >= 0].min() if (mine >= 0).any() else -1), (what, g)
        if not st["active"]:
            assert (mine == -1).all() and st["candidates"] == 0 and st["position"].tobytes() + st["rot"].tobytes() + st["box"].tobytes() == bytes(32), (what, g)
        else:
            own = int(q["body"])
            assert own < 0 or (shapes["body"][mine[mine >= 0]] != own).all(), (what, g)  # a mounted grid never sees its own body
            if int(q["flags"]) & wire.GRID_SENSOR_SKIP_STATIC:
                assert (world["bodies"]["type"][shapes["body"][mine[mine >= 0]]] != wire.BODY_STATIC).all(), (what, g)


def assert_probe(s, world, grids, got, what):
    """The device's own s2amd_world_point_probe of the statement's cell points, folded: the arrays of every plain grid"""
    cats, low, occ, states = got
    first, total = grid_report_ref.first_cells(grids)
    active = np.array([grid_report_ref.cell_points(world, q)[0] for q in grids], dtype=bool)
    assert states["active"].tolist() == active.astype(int).tolist(), what
    points, index = grid_report_ref.probes_of(world, grids)
    if len(points) == 0:
        return
    offsets, flat = s.world_point_probe(points, expected=4 * len(points) + 64)
    pc, pl, po = grid_report_ref.fold_probe(world, total, index, offsets, flat)
    keep = np.zeros(total, dtype=bool)
    ok = plain(world, grids)
    for g, q in enumerate(grids):
        if ok[g] or not active[g]:
            keep[first[g]: first[g] + int(q["width"]) * int(q["height"])] = True
    assert cats[keep].tobytes() == pc[keep].tobytes(), what
    assert low[keep].tobytes() == pl[keep].tobytes(), what
    assert occ[keep].tobytes() == po[keep].tobytes(), what
    # ... and an exclusion only ever removes hits
    assert ((cats & ~pc) == 0).all() and ((low >= pl) | (low < 0)).all(), what


def assert_statement(world, grids, got, what, period=None):
    """The statement's bytes where the reference is built; a list that repeats its first `period` grids is compared on one period"""
    if not grid_report_ref.available():
        return
    cats, low, occ, states = got
    n = len(grids) if period is None or period >= len(grids) else period
    if n < len(grids):
        assert all(grids[i].tobytes() == grids[i % n].tobytes() for i in range(len(grids)))
    wc, wl, wo, ws = grid_report_ref.report(world, grids[:n])
    cells = len(wc)
    for k in range(0, len(grids), n):
        m = min(n, len(grids) - k)
        c = int(ws["firstCell"][m - 1] + ws["cells"][m - 1])
        at = (k // n) * cells
        assert cats[at: at + c].tobytes() == wc[:c].tobytes() and low[at: at + c].tobytes() == wl[:c].tobytes() and occ[at: at + c].tobytes() == wo[:c].tobytes(), (what, k)
        want = ws[:m].copy()
        want["grid"] += k
        want["firstCell"] += at
        if states[k: k + m].tobytes() != want.tobytes():
            bad = [f for f in want.dtype.names if states[k: k + m][f].tobytes() != want[f].tobytes()]
            raise AssertionError("%s: states of period %d differ in %s: %s / %s" % (what, k, bad, states[k: k + m][:2], want[:2]))


def assert_report(s, world, grids, what, period=None, statement=True):
    resident = downloaded_world(s, world)
    got = getters(s)
    assert_structure(resident, grids, got, what)
    assert_probe(s, resident, grids, got, what)
    if statement:
        assert_statement(resident, grids, got, what, period)
    return got
