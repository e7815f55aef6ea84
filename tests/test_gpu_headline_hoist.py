"""The persistent strip step kernel (wide_kernel.hip: wideStepKernel) prepares round 0 of a solve sweep inside the plain warm start in
front of it, in the half of the workgroup that idles there; relax sweeps, cold starts and the body-centric warm start prepare it where
the sweep begins.  And a step that is only enqueued (option "async") records no timing events.  Neither may change a bit: the C-ABI
result equals the oracle BIT FOR BIT when the oracle sweeps in the order the library reports, on every path into a solve sweep, on the
roomier layouts (parked rounds, <3, 3>, <4, 2>), on the POINTS == 0 variant and under the two other soft solvers, which share the
step loop.  Every case asserts that it ran the persistent wide kernel: one that falls to another path fails."""
import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import common, oraclebind
from tests.parity import resident_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pile():
    return synthetic.pyramid(100)


def on_the_wide_kernel(s):
    st = s.stats()
    assert st["persistent"] == 1 and st["pairLanes"] == 2, st


@pytest.mark.parametrize("iters,warm", [((8, 4), True), ((3, 0), True), ((1, 1), True), ((5, 2), False)],
                         ids=["8-4-warm", "3-0-warm", "1-1-warm", "5-2-cold"])
def test_every_way_into_a_solve_sweep(pile, iters, warm):
    """(8, 4): solve sweeps behind a warm start, relax sweeps behind s2IntegratePositions; (3, 0): warm-started sweeps only; (1, 1):
    one of each; (5, 2) cold: no warm start at all, every sweep prepares its own round 0."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, iters[0], iters[1], warm)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        resident_vs_oracle(s, params, pile, 5, "%s warm=%s" % (iters, warm), 3)
        on_the_wide_kernel(s)


@pytest.mark.parametrize("debug", [16, 64, 128], ids=["parked", "3_3", "4_2"])
def test_roomier_layouts_on_a_partition_that_does_not_need_them(pile, debug):
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        s.set_option("persist_debug", debug)
        resident_vs_oracle(s, params, pile, 3, "persist_debug %d" % debug, 3)
        on_the_wide_kernel(s)


def test_mixed_point_counts_and_empty_manifolds(pile):
    """The POINTS == 0 variant: one-point manifolds and manifolds without points (tests/test_gpu_selfstrips.py has the recipe)."""
    pre = common.copy3(pile)
    rng = np.random.default_rng(5)
    live = np.flatnonzero(pre[1]["pointCount"] == 2)
    pre[1]["pointCount"][rng.choice(live, size=400, replace=False)] = 1
    pre[1]["pointCount"][rng.choice(live, size=150, replace=False)] = 0
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        resident_vs_oracle(s, params, pre, 4, "mixed point counts", 3)
        on_the_wide_kernel(s)


@pytest.mark.parametrize("solver_name", ["SoftStep", "PGS_Soft"])
def test_the_other_soft_solvers_share_the_step_loop(pile, solver_name):
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        resident_vs_oracle(s, params, pile, 3, solver_name)
        on_the_wide_kernel(s)


def test_enqueued_steps_equal_synchronous_steps(pile):
    """12 steps enqueued back to back (no timing events on the stream) against 12 synchronous ones from the same upload; the first
    synchronous step afterwards reports its device time again."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    got = []
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        for enqueue in (0, 1):
            s.upload(*pile)
            s.set_option("async", enqueue)
            for _ in range(12):
                s.step_resident(params)
            s.synchronize()
            s.set_option("async", 0)
            out = common.copy3(pile)
            s.download(*out)
            got.append(out)
        on_the_wide_kernel(s)
        s.step_resident(params)
        assert s.stats()["deviceMs"] > 0, s.stats()
    (sb, sc, _), (ab, ac, _) = got
    for f in ("position", "rot", "linearVelocity", "angularVelocity"):
        assert np.array_equal(sb[f].view(np.uint32), ab[f].view(np.uint32)), f
    for f in ("normalImpulse", "tangentImpulse"):
        assert np.array_equal(sc["points"][f].view(np.uint32), ac["points"][f].view(np.uint32)), f


def test_the_world_step_still_times_its_solve():
    from tests import world_chain
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    world = synthetic.pyramid_world(40)
    with hip.Solver(0) as s:
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        info = s.world_step(params)
    assert info["solveMs"] > 0, info
