"""The group patience of the structure builds (solver_internal.h: noteGraphChanged, SolverRest::groupPatienceNow; "group_patience", on by
default) on worlds big enough for it -- at least S2_GROUP_PATIENCE_MIN_POSITIONS = 16,384 sweep positions, which no other world of the
suite has.  When a contact touches a body that an LDS group or a resident island holds while the structure is younger than 8 steps, the
next structures are built WITHOUT groups: the small islands go into the colour batches of the global part, beside the strips where the
world has a big island too, until the graph has been quiet for 4, 8, ... steps; then a rebuild that no change of the graph asked for
brings the groups back.

The worlds (tests/world_chain.py: debris_world, pile_and_debris_world; counted by tests/test_churn_worlds.py) are base-10 pyramids, alone
or beside one base-100 pile, with five small heavy balls that come down on the top boxes of five small pyramids in steps 6, 9, 12, 15
and 20.  Every run is the whole loop of test_wrecking_ball_world_loop -- pair query against the oracle's, contact creation,
s2amd_world_step, the oracle chain swept in the order the device reports -- and every byte of every array must agree, at every step in
which the structure was built again or the number of groups changed and at every 4th step otherwise."""
import functools

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import common, world_chain
from tests.world_chain import _create_contacts

pytestmark = pytest.mark.gpu

MAX_GROUP_BODIES = 1024  # SolverRest::optMaxGroupBodies: islands up to this size go into LDS groups / resident islands
# the steps of a run: the last ball touches in step 20, the groups are due back 4 (at most 8) quiet steps later.  s2Solve_XPBD lets
# untouched base-10 pyramids lose and regain manifold points from step 35 on (oracle chain in pool order), so its run ends before that.
STEPS = {"TGS_Soft": 40, "SoftStep": 40, "PGS_Soft": 40, "PGS_NGS_Block": 40, "XPBD": 32}


@functools.lru_cache(maxsize=None)
def _world(shape, count=None):
    if shape == "debris":
        return world_chain.debris_world(*(() if count is None else (count,)))[0]
    return world_chain.pile_and_debris_world()[0]


def _small_islands(world):
    return int((world_chain.island_census(world)["bodies"] <= MAX_GROUP_BODIES).sum())


def _chain(s, world, params, steps, what):
    """Uploads `world` and runs the whole loop for `steps` steps against the oracle chain.  Returns one row per step: the stats the
    structure path shows through, what changed the graph in that step, and (where the device ran without groups) how many small islands
    the oracle's side of the chain holds."""
    ref = world_chain.copy_world(world)
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
    rows = []
    for step in range(steps):
        created = 0
        if world_chain.moved_any(ref):
            got = s.world_find_pairs()
            want = world_chain.oracle_find_pairs(ref)
            assert np.array_equal(got, want), "%s step %d: new pairs" % (what, step)
            if len(got):
                created = len(got)
                slots, contacts, pairs = _create_contacts(ref, got)
                s.world_set_contacts(slots, contacts, pairs)
        info = s.world_step(params)
        order, _ = s.contact_order()
        status = world_chain.oracle_world_step(params, ref, contact_order=order)
        assert info["separatedCount"] == int((status == wire.PAIR_SEPARATED).sum()), "%s step %d" % (what, step)
        st = s.stats()
        row = {"step": step, "created": created, "graphChanged": int(info["graphChanged"]), "small": None}
        row.update({k: int(st[k]) for k in ("groupCount", "stripCount", "structureBuilds", "placedContacts")})
        if row["groupCount"] == 0:
            row["small"] = _small_islands(ref)
        turned = not rows or row["structureBuilds"] != rows[-1]["structureBuilds"] or row["groupCount"] != rows[-1]["groupCount"]
        if turned or step % 4 == 3:
            out = world_chain.copy_world(world)
            res = s.world_download(*[out[k] for k in world_chain.WORLD_KEYS])
            world_chain.assert_device_equals_oracle(dict(zip(world_chain.WORLD_KEYS, res[:6])), ref,
                                                    "%s step %d (%d groups, %d strips, build %d)" % (what, step, row["groupCount"], row["stripCount"], row["structureBuilds"]))
        rows.append(row)
    return rows


def _story(rows):
    """The steps at which the groups went and came back, and the builds: what a run exercised, for the log."""
    gone = [r["step"] for i, r in enumerate(rows) if i > 0 and r["groupCount"] == 0 and rows[i - 1]["groupCount"] > 0]
    back = [r["step"] for i, r in enumerate(rows) if i > 0 and r["groupCount"] > 0 and rows[i - 1]["groupCount"] == 0]
    built = [r["step"] for i, r in enumerate(rows) if i == 0 or r["structureBuilds"] != rows[i - 1]["structureBuilds"]]
    return "groups gone in steps %s, back in steps %s; %d structure builds (in steps %s), %d contacts placed, groups/strips at the end %d/%d" % (
        gone, back, rows[-1]["structureBuilds"], built, rows[-1]["placedContacts"], rows[-1]["groupCount"], rows[-1]["stripCount"])


def _params(solver_name):
    vel, pos = common.DEFAULT_ITERS[solver_name]
    return wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)


# the resident-island kernels (soft solvers) on both worlds, the op interpreter on the debris
RUNS = [("debris", "TGS_Soft"), ("debris", "SoftStep"), ("debris", "PGS_Soft"), ("pile", "TGS_Soft"), ("pile", "SoftStep"), ("pile", "PGS_Soft"),
        ("debris", "PGS_NGS_Block"), ("debris", "XPBD")]


@pytest.mark.parametrize("shape,solver_name", RUNS)
def test_groups_go_and_come_back_under_the_default_options(shape, solver_name):
    """Default options.  The run must have taken the path, all three stages of it:
    (a) groups in the first step;
    (b) a later step without groups while the oracle's side still holds small islands (they are in the global part's colour batches);
    (c) after the last created contact, a step that has groups again although the step before had none -- at least 4 steps after the
        last change of the graph (a created contact or a manifold that gained or lost its points), with no such change in it, and
        with a structure build in it that nothing but the patience running out asked for.
    Each of these steps is among those compared byte for byte (_chain).  Then the same world is uploaded again on the same solver: a new
    world clears the patience, so its first step has groups, and it is bit-exact as well."""
    world = _world(shape)
    what = "%s %s" % (shape, solver_name)
    with hip.Solver(0) as s:
        rows = _chain(s, world, _params(solver_name), STEPS[solver_name], what)
        print("%s: %s" % (what, _story(rows)))
        assert rows[0]["groupCount"] > 0, (what, rows[0])  # (a)
        without = [r for r in rows[1:] if r["groupCount"] == 0]
        assert without and all(r["small"] > 0 for r in without), (what, _story(rows))  # (b)
        if shape == "pile":
            # ... next to strips: the big pile is on them in at least one of those steps
            assert any(r["stripCount"] > 1 for r in without), (what, [(r["step"], r["stripCount"]) for r in without])
        last_created = max(r["step"] for r in rows if r["created"])
        returns = []
        for i in range(last_created + 1, len(rows)):
            if rows[i]["groupCount"] > 0 and rows[i - 1]["groupCount"] == 0:
                last_change = max(r["step"] for r in rows[:i + 1] if r["created"] or r["graphChanged"])
                returns.append((i, last_change))
                assert i - last_change >= 4 and rows[i]["graphChanged"] == 0 and rows[i]["created"] == 0, (what, i, last_change, _story(rows))
                assert rows[i]["structureBuilds"] == rows[i - 1]["structureBuilds"] + 1, (what, rows[i - 1], rows[i])
        assert returns, (what, _story(rows))  # (c)
        # reset: the same world again on the same solver
        again = _chain(s, world, _params(solver_name), 1, what + ", uploaded again")
        assert again[0]["groupCount"] > 0, (what, again[0])


@pytest.mark.parametrize("shape,solver_name", RUNS)
def test_groups_stay_with_the_patience_switched_off(shape, solver_name):
    """Control: the same worlds and steps with option "group_patience" 0.  Groups in every step, bit-exact against this run's own oracle
    chain (the two runs report different sweep orders, so neither is held against the other)."""
    what = "%s %s, group_patience 0" % (shape, solver_name)
    with hip.Solver(0) as s:
        s.set_option("group_patience", 0)
        rows = _chain(s, _world(shape), _params(solver_name), STEPS[solver_name], what)
    print("%s: %s" % (what, _story(rows)))
    assert all(r["groupCount"] > 0 for r in rows), (what, _story(rows))


@pytest.mark.parametrize("solver_name", ["TGS_Soft", "PGS_NGS_Block"])
def test_groups_stay_in_a_world_below_the_threshold(solver_name):
    """The debris shape with 60 pyramids (8,700 positions, below S2_GROUP_PATIENCE_MIN_POSITIONS) and the same balls under the default
    options: building again is the cheap way there, the groups are in every structure."""
    what = "debris of 60 %s" % solver_name
    with hip.Solver(0) as s:
        rows = _chain(s, _world("debris", 60), _params(solver_name), STEPS[solver_name], what)
    print("%s: %s" % (what, _story(rows)))
    assert all(r["groupCount"] > 0 for r in rows), (what, _story(rows))
    assert rows[-1]["structureBuilds"] > 1, (what, _story(rows))  # (the balls did force rebuilds)
