"""The worlds of tests/test_gpu_group_patience.py (tests/world_chain.py: churn_world, debris_world, pile_and_debris_world), counted on the
host with solver2d_amd/islands.py: the group patience applies from S2_GROUP_PATIENCE_MIN_POSITIONS = 16,384 sweep positions on
(solver2d_amd/csrc/solver_internal.h), and whether a world has them is a count here, not a guess there."""
import numpy as np

from solver2d_amd import synthetic, wire
from tests import world_chain

MIN_POSITIONS = 16384    # S2_GROUP_PATIENCE_MIN_POSITIONS
MAX_GROUP_BODIES = 1024  # SolverRest::optMaxGroupBodies


def _check_indices(world, balls):
    b, c, sh, p = world["bodies"], world["contacts"], world["shapes"], world["pairs"]
    live = p["shapeA"] >= 0
    assert np.array_equal(live, c["pointCount"] > 0) and len(c) == len(p)
    assert (c["constraintIndex"][~live] == -1).all() and (p["shapeB"][~live] == -1).all()
    assert (~live).sum() >= 4 * live.sum() // 3 + 256  # wreck_world's spare slots
    # one shape per body, same index; every pair names the shapes of its manifold's bodies; no pair twice
    assert np.array_equal(sh["body"], np.arange(len(b)))
    assert np.array_equal(p["shapeA"][live], c["bodyA"][live]) and np.array_equal(p["shapeB"][live], c["bodyB"][live])
    keys = c["bodyA"][live].astype(np.int64) * len(b) + c["bodyB"][live]
    assert len(np.unique(keys)) == len(keys)
    assert np.array_equal(sh["proxyKey"], (np.arange(len(b)) << 4) | b["type"])
    assert np.array_equal(world["origins"], b["position"])
    # every manifold joins bodies that touch: centres one box apart (a ground: the box stands on it)
    d = np.abs(b["position"][c["bodyA"][live]] - b["position"][c["bodyB"][live]])
    on_ground = b["type"][c["bodyA"][live]] == wire.BODY_STATIC
    assert (d[~on_ground].max(axis=1) <= 1.0 + 1e-6).all() and (d[on_ground][:, 1] == 1.5).all()
    assert list(balls) == list(range(len(b) - len(balls), len(b)))
    assert (sh["type"][balls] == wire.SHAPE_CIRCLE).all() and (sh["enlarged"][balls] == 1).all() and (sh["enlarged"][:balls[0]] == 0).all()


def _ball_targets(world, balls):
    """Per ball: (bodies of the island below it, metres between the ball and the top of the box below it)."""
    b = world["bodies"]
    from solver2d_amd import islands
    island, _ = islands.find_islands(b, world["contacts"], world["joints"])
    out = []
    for i in balls:
        x, y = b["position"][i]
        under = np.flatnonzero((np.abs(b["position"][:, 0] - x) < 0.5) & (b["position"][:, 1] < y) & (b["type"] == wire.BODY_DYNAMIC) &
                               (np.arange(len(b)) < balls[0]))
        top = under[np.argmax(b["position"][under, 1])]
        out.append((int((island == island[top]).sum()), float(y - world["shapes"]["radius"][i] - (b["position"][top, 1] + 0.5))))
    return out


def test_churn_worlds_have_the_positions_and_islands_the_group_patience_needs():
    for count, enough in ((120, True), (60, False)):
        world, balls = world_chain.debris_world(count)
        _check_indices(world, balls)
        census = world_chain.island_census(world)
        assert census["positions"] == 145 * count and (census["positions"] >= MIN_POSITIONS) == enough
        assert len(census["bodies"]) == count and (census["bodies"] == 55).all() and (census["constraints"] == 145).all()
        for size, gap in _ball_targets(world, balls):
            assert size == 55 and gap > 2.0 * float(synthetic.AABB_MARGIN)  # a small pyramid; no pair before the first structure is built
    world, balls = world_chain.pile_and_debris_world()
    _check_indices(world, balls)
    census = world_chain.island_census(world)
    assert census["positions"] == 14950 + 14 * 145 and census["positions"] >= MIN_POSITIONS
    small = census["bodies"] <= MAX_GROUP_BODIES
    assert small.sum() >= 12 and (census["bodies"][small] == 55).all()
    assert (~small).sum() == 1 and census["bodies"][~small][0] == 5050
    for size, gap in _ball_targets(world, balls):
        assert size == 55 and gap > 2.0 * float(synthetic.AABB_MARGIN)  # no ball over the big pile
