"""s2Solve_SoftStep and s2Solve_PGS_Soft on the 512-thread resident-island kernel (wide_kernel.hip: wideIslandKernel<KIND, ROUNDS,
SELF, POINTS>): worlds of many small islands, stepped resident through the C-ABI and compared BIT FOR BIT with the oracle swept in
the order the device reports -- the gate of tests/test_gpu_fullsize.py: test_config5_512_pyramids_tgs_soft.

s2amd_get_resident_kernel says which kernel swept the islands (2 islandStepKernel, 3 the 512-thread kernel between the body
prologue and epilogue, 4 the same as the step's only launch) and in which variant (6 or 8 colour rounds per lane).  The forms that
exist: PGS_Soft 6 and 8 rounds, SoftStep 6 rounds; a SoftStep world whose groups need a 7th or 8th round stays on islandStepKernel
(kernel 2) and is checked there.  The (kernel, rounds) each world is expected on were read from that query and are fixed below.
"""
import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import common, oraclebind, world_chain
# (the builders the variant census shares with this file live beside its case table)
from tests.variant_cases import fuzz_world, hub_pyramids, mixed_point_counts, mixed_pyramids, with_free_bodies

pytestmark = pytest.mark.gpu

SOLVERS = ["SoftStep", "PGS_Soft"]
SEEN = {}  # solver name -> set of (kernel, rounds) over the tests of this file that ran before the census at its end


def kinematic_world():
    """A kinematic body (no mass, a velocity of its own) as the top brick of some pyramids: an island reads it, nothing writes it."""
    b, c, j = synthetic.pyramid(12, count=6)
    per = len(b) // 6
    for k in (0, 2, 5):
        top = (k + 1) * per - 1
        assert b[top]["type"] == wire.BODY_DYNAMIC
        b[top]["type"] = wire.BODY_KINEMATIC
        for f in ("mass", "invMass", "I", "invI"):
            b[top][f] = 0.0
        b[top]["linearVelocity"] = (0.25, 0.0)
        b[top]["angularVelocity"] = 0.1
    return b, c, j


# world name -> (builder, options, {solver: (kernels allowed, rounds)})
FUZZ_OPTIONS = {"max_group_bodies": 64, "strip_patience": 0}
WORLDS = {
    "mixed_pyramids": (mixed_pyramids, {}, {"SoftStep": ((4,), 6), "PGS_Soft": ((4,), 6)}),
    "mixed_point_counts": (mixed_point_counts, {}, {"SoftStep": ((4,), 6), "PGS_Soft": ((4,), 6)}),
    "kinematic": (kinematic_world, {}, {"SoftStep": ((3,), 6), "PGS_Soft": ((3,), 6)}),
    "hub_pyramids": (hub_pyramids, {}, {"SoftStep": ((2,), 8), "PGS_Soft": ((4,), 8)}),
}


def params_of(solver_name, warm):
    vel, pos = common.DEFAULT_ITERS[solver_name]
    return wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, warm)


def resident_steps(pre, params, options, steps=3, what="", check=True):
    """`steps` resident steps; every step compared with the oracle in the device's order.  Returns the downloaded arrays, the contact
    orders and the (kernel, rounds) of each step."""
    outs, orders, kernels = [], [], []
    with hip.Solver(0) as s:
        for k, v in options.items():
            s.set_option(k, v)
        s.upload(*pre)
        want = common.copy3(pre)
        for step in range(steps):
            s.step_resident(params)
            order, offsets = s.contact_order()
            jorder, _ = s.joint_order()
            got = common.copy3(pre)
            s.download(*got)
            kernels.append(s.resident_kernel())
            if check:
                oraclebind.solve(params, *want, contact_order=order, joint_order=jorder)
                common.compare_exact(got, want, "%s step %d (kernel %r)" % (what, step, kernels[-1]))
            outs.append(got), orders.append((order.copy(), offsets.copy()))
        st = s.stats()
    return outs, orders, kernels, st


def note(solver_name, kernels):
    SEEN.setdefault(solver_name, set()).update(kernels)


@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("solver_name", SOLVERS)
@pytest.mark.parametrize("world", sorted(WORLDS))
def test_island_worlds_bit_exact_on_the_512_thread_kernel(world, solver_name, warm):
    build, options, expect = WORLDS[world]
    allowed, rounds = expect[solver_name]
    pre = build()
    _, _, kernels, st = resident_steps(pre, params_of(solver_name, warm), options, what="%s/%s" % (world, solver_name))
    print(world, solver_name, kernels, st["groupCount"], st["kernelLaunches"])
    note(solver_name, kernels)
    if 2 not in allowed:
        assert all(k in (3, 4) for k, _ in kernels), kernels
    assert kernels[-1][0] in allowed and kernels[-1][1] == rounds, kernels


# seeds whose groups need a 7th or 8th colour round under these options (read from s2amd_get_resident_kernel, then fixed here)
# (seed, bodies, contacts, rounds of the variant)
FUZZ_CASES = [(0, 60, 90, 8), (1, 60, 90, 8), (3, 60, 90, 8), (5, 60, 90, 8), (10, 60, 90, 6), (0, 120, 160, 6), (1, 120, 160, 6)]


@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("solver_name", SOLVERS)
@pytest.mark.parametrize("seed,n_bodies,n_contacts,rounds", FUZZ_CASES)
def test_fuzz_worlds_bit_exact_in_six_and_eight_rounds(seed, n_bodies, n_contacts, rounds, solver_name, warm):
    pre = fuzz_world(seed, n_bodies, n_contacts)
    _, _, kernels, st = resident_steps(pre, params_of(solver_name, warm), FUZZ_OPTIONS, what="fuzz %d/%s" % (seed, solver_name))
    print(seed, solver_name, kernels, st["groupCount"])
    note(solver_name, kernels)
    assert all(r == rounds for _, r in kernels), kernels
    if solver_name == "SoftStep" and rounds == 8:
        # no eight-round form for s2Solve_SoftStep (wide_kernel.hip: wideIslandVariants): the world stays on islandStepKernel
        assert all(k == 2 for k, _ in kernels), kernels
    else:
        assert all(k in (3, 4) for k, _ in kernels), kernels


@pytest.mark.parametrize("solver_name", SOLVERS)
def test_islands_beside_free_bodies_run_between_prologue_and_epilogue(solver_name):
    """The non-SELF form: kernel 3 in every step between the body launches, bit-exact; with "wide" = 0 the same world is on islandStepKernel."""
    pre = with_free_bodies(mixed_pyramids((5, 12, 23, 40, 9)))
    params = params_of(solver_name, True)
    outs, orders, kernels, st = resident_steps(pre, params, {}, what="free bodies/%s" % solver_name)
    note(solver_name, kernels)
    assert kernels == [(3, 6)] * 3 and st["kernelLaunches"] >= 3, (kernels, st)  # (prologue, islands, epilogue, and the free bodies' own launch)
    old_outs, old_orders, old_kernels, _ = resident_steps(pre, params, {"wide": 0}, what="free bodies/%s wide=0" % solver_name, check=False)
    assert old_kernels == [(2, 6)] * 3, old_kernels
    assert_same_runs(outs, orders, old_outs, old_orders)


def assert_same_runs(outs, orders, old_outs, old_orders):
    for step, (a, b) in enumerate(zip(outs, old_outs)):
        for x, y, name in zip(a, b, ("bodies", "contacts", "joints")):
            assert x.tobytes() == y.tobytes(), "step %d: %s differ between the defaults and wide = 0" % (step, name)
    for (o, off), (o2, off2) in zip(orders, old_orders):
        assert np.array_equal(o, o2) and np.array_equal(off, off2)


@pytest.mark.parametrize("solver_name", SOLVERS)
@pytest.mark.parametrize("world", sorted(WORLDS) + ["fuzz6", "fuzz8"])
def test_defaults_and_wide_off_return_the_same_bytes(world, solver_name):
    """No behaviour change: the kernel the defaults pick and islandStepKernel ("wide" = 0) return byte-identical bodies and contacts
    and report the same contact order."""
    if world.startswith("fuzz"):
        pre, options = fuzz_world(*[c for c in FUZZ_CASES if c[3] == int(world[4:])][0][:3]), FUZZ_OPTIONS
    else:
        pre, options = WORLDS[world][0](), WORLDS[world][1]
    params = params_of(solver_name, True)
    outs, orders, kernels, _ = resident_steps(pre, params, options, check=False)
    off = dict(options)
    off["wide"] = 0
    old_outs, old_orders, old_kernels, _ = resident_steps(pre, params, off, check=False)
    assert all(k == 2 for k, _ in old_kernels), old_kernels
    assert_same_runs(outs, orders, old_outs, old_orders)
    assert kernels[0][1] == old_kernels[0][1]


@pytest.mark.parametrize("solver_name", SOLVERS)
def test_whole_chain_of_eight_pyramids(solver_name):
    """Narrow phase -> solve -> refit on the device-resident world against the oracle chain, two steps."""
    params = params_of(solver_name, True)
    world = synthetic.pyramid_world(40, count=8)
    ref = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for step in range(2):
            info = s.world_step(params)
            order, _ = s.contact_order()
            world_chain.oracle_world_step(params, ref, contact_order=order)
            out = world_chain.copy_world(world)
            res = s.world_download(*[out[k] for k in world_chain.WORLD_KEYS])
            world_chain.assert_device_equals_oracle(dict(zip(world_chain.WORLD_KEYS, res[:6])), ref, "8 x pyramid40 %s world step %d" % (solver_name, step))
            assert info["separatedCount"] == 0
        kernel, rounds = s.resident_kernel()
        note(solver_name, [(kernel, rounds)])
        assert kernel in (3, 4) and rounds == 6, (kernel, rounds)


@pytest.mark.parametrize("solver_name", SOLVERS)
def test_config5_512_pyramids(solver_name):
    """512 independent base-40 pyramids in one world (BASELINE configs[4]): two resident steps against the oracle, the second one
    launch."""
    pre = synthetic.pyramid(40, count=512)
    params = params_of(solver_name, True)
    with hip.Solver(0) as s:
        s.upload(*pre)
        want = common.copy3(pre)
        for step in range(2):
            s.step_resident(params)
            order, _ = s.contact_order()
            oraclebind.solve(params, *want, contact_order=order)
            got = common.copy3(pre)
            s.download(*got)
            common.compare_exact(got, want, "512 x pyramid40 %s step %d" % (solver_name, step))
        st = s.stats()
        kernel, rounds = s.resident_kernel()
    note(solver_name, [(kernel, rounds)])
    assert st["groupCount"] == 512 and st["constraintCount"] == 1218560 and st["kernelLaunches"] == 1, st
    assert (kernel, rounds) == (4, 6)


@pytest.mark.parametrize("solver_name", SOLVERS)
def test_tolerance_library_on_an_island_world(solver_name):
    """libs2amd_fast.so (FMA contraction): within the tolerance tests/test_gpu_fast.py states for these solvers, rtol 1e-5 per sweep."""
    pre = mixed_pyramids((5, 12, 23, 40))
    params = params_of(solver_name, True)
    with hip.Solver(0, fast=True) as s:
        s.upload(*pre)
        s.step_resident(params)  # (the structure is built; the next step is the one launch)
        s.step_resident(params)
        before = common.copy3(pre)
        s.download(*before)
        s.step_resident(params)
        order, _ = s.contact_order()
        got = common.copy3(pre)
        s.download(*got)
        kernel, rounds = s.resident_kernel()
    assert (kernel, rounds) == (4, 6)
    want = common.copy3(before)
    oraclebind.solve(params, *want, contact_order=order)
    common.compare_close(got, want, common.sweeps_touching_bodies(params), "fast %s" % solver_name, rtol_per_sweep=1e-5, params=params)


def test_census_every_form_that_exists_was_seen():
    """Census over the file (runs last: pytest keeps definition order): PGS_Soft on the 512-thread kernel in 6 and in 8 rounds,
    SoftStep on it in 6 rounds and on islandStepKernel where a group needs 8."""
    assert SEEN, "a census of the tests above: run the file whole"
    pgs, soft = SEEN.get("PGS_Soft", set()), SEEN.get("SoftStep", set())
    assert {r for k, r in pgs if k in (3, 4)} == {6, 8}, pgs
    assert {r for k, r in soft if k in (3, 4)} == {6} and (2, 8) in soft, soft
    assert any(k == 3 for k, _ in pgs) and any(k == 4 for k, _ in pgs) and any(k == 3 for k, _ in soft) and any(k == 4 for k, _ in soft)
