"""TEST INFRASTRUCTURE.  One table of cases for the variant census (include/solver2d_amd.h: s2amd_get_variant_entry): worlds, solvers and
options that between them make the host select EVERY entry of the six variant tables of the register-resident soft kernels
(launch.h: KernelVariant -- wideStepKernel, wideIslandKernel, stripStepKernel, islandStepKernel, stripSoftKernel, pairStepKernel), and for
each case the exact set of (family, key) it must select.  tests/test_variant_reach_host.py runs the table against the stand-in HIP runtime
(host selection only), tests/test_gpu_variant_census.py on the GPU, every step bit for bit against the oracle; both assert that the union
over the table IS the library's enumeration.  A table entry exists if and only if a case here runs it.

A case is one of two kinds:
  * resident: (bodies, contacts, joints) uploaded once, `steps` calls of s2amd_step_resident;
  * chain: the same through s2amd_world_upload -- a resident WORLD is the only place a created contact can take an overflow position
    behind the strips (solver_internal.h: IncrementalStrips), which is what the SLICED and OVERFLOW forms of wideStepKernel exist for --,
    stepped by s2amd_step_resident all the same, so the manifolds stay the caller's (two points each, or mixed counts) and the host knows
    them.  The case creates a contact between two boxes several strips apart (s2amd_world_set_contacts) before step `touch_at`; the
    worker thread's rebuild is put off beyond the case's end (option "async_build_delay"), so the steps from there on run in that form.

Keys are written as the tables write them (launch.h: SoftKind / WarmKind; wide_kernel.hip: S2_WIDE_*)."""
import numpy as np

from solver2d_amd import synthetic, wire
from tests import common, fuzz_worlds

KIND = {"TGS_Soft": 0, "PGS_Soft": 1, "SoftStep": 3}  # SOFT_TGS, SOFT_PGS, SOFT_FIXED
WARM = {"TGS_Soft": 0, "PGS_Soft": 0, "SoftStep": 1}  # WARM_CURRENT, WARM_CURRENT, WARM_FIXED: the one warm start each driver's plan has
PLAIN, SELF, BODYWARM, SLICED, OVERFLOW = 0, 1, 2, 4, 8  # wideStepKernel's MODE
L32, L33, L42, L322, L3222 = (3, 2, 0, 0), (3, 3, 0, 0), (4, 2, 0, 0), (3, 2, 2, 0), (3, 2, 2, 2)  # its layouts <RPH, SR, SL, IL>
# option "persist_debug": the host picks a roomier layout than the partition needs (wide_kernel.hip: wideKey); no kernel reads them
FORCE_PARKED, FORCE_THIRD_SEAM, FORCE_FOURTH_PAIR = 16, 64, 128
FORCING_BITS = FORCE_PARKED | FORCE_THIRD_SEAM | FORCE_FOURTH_PAIR


def wide(solver, points, layout, mode=PLAIN):
    return ("wideStepKernel", (points,) + tuple(layout) + (mode, KIND[solver]))


def wide_island(solver, rounds, self_contained, points):
    return ("wideIslandKernel", (KIND[solver], rounds, 1 if self_contained else 0, points))


def strip_step(solver, points, rounds, seam_regs=0):
    return ("stripStepKernel", (KIND[solver], WARM[solver], points, rounds, seam_regs))


def island_step(solver, rounds):
    return ("islandStepKernel", (KIND[solver], WARM[solver], rounds))


def strip_soft(solver, with_warm_start):
    return ("stripSoftKernel", (KIND[solver], WARM[solver] if with_warm_start else -1))


def pair_step(solver, points):
    return ("pairStepKernel", (KIND[solver], WARM[solver], points))


# ---- worlds ----

def concat_worlds(parts):
    """Several (bodies, contacts, joints) worlds as one, body indices shifted."""
    bodies = np.concatenate([p[0] for p in parts])
    contacts, joints, base = [], [], 0
    for b, c, j in parts:
        c, j = c.copy(), j.copy()
        for arr in (c, j):
            if len(arr):
                live = arr["bodyA"] >= 0
                arr["bodyA"][live] += base
                arr["bodyB"][live] += base
        contacts.append(c), joints.append(j)
        base += len(b)
    return bodies, np.concatenate(contacts), np.concatenate(joints)


def mixed_pyramids(bases=(5, 8, 12, 17, 23, 31, 40, 9, 26, 40, 6, 14)):
    """Pyramids of mixed bases, each on its own static ground (a ground contact has a static side: the doubled contact hertz)."""
    parts = []
    for k, base in enumerate(bases):
        b, c, j = synthetic.pyramid(base)
        b = b.copy()
        b["position"][:, 0] += np.float32(64.0 * k)
        parts.append((b, c, j))
    return concat_worlds(parts)


def with_point_counts(world, seed=11):
    """The same graph with manifolds of 0, 1 and 2 points: the kernels' POINTS == 0 forms (per-point masking)."""
    b, c, j = common.copy3(world)
    rng = np.random.default_rng(seed)
    pick = rng.random(len(c))
    c["pointCount"][pick < 0.15] = 0
    c["pointCount"][(pick >= 0.15) & (pick < 0.40)] = 1
    assert {0, 1, 2} <= set(np.unique(c["pointCount"]).tolist())
    return b, c, j


def mixed_point_counts(seed=11):
    return with_point_counts(mixed_pyramids((5, 12, 20, 31, 7, 16)), seed)


def hub_pyramids():
    """Pyramids whose top brick also touches five bricks further down (copies of its own manifolds with another partner): a body
    with seven contacts, so its group needs a seventh colour round -- the eight-round variant, in an islands-only world."""
    b, c, j = synthetic.pyramid(12, count=4)
    per_b, per_c = len(b) // 4, len(c) // 4
    extra = []
    for k in range(4):
        top = (k + 1) * per_b - 1
        mine = [i for i in range(k * per_c, (k + 1) * per_c) if top in (int(c[i]["bodyA"]), int(c[i]["bodyB"]))]
        assert len(mine) == 2
        for n in range(5):
            e = c[mine[n % 2]].copy()
            partner = k * per_b + (1, 12, 13, 23, 24)[n]  # bricks at the ends of the lower rows (three or four contacts of their own)
            assert b[partner]["type"] == wire.BODY_DYNAMIC and partner != top
            if int(e["bodyA"]) == top:
                e["bodyB"] = partner
            else:
                e["bodyA"] = partner
            e["points"][0]["separation"] = 0.004 * n - 0.01
            extra.append(e)
    return b, np.concatenate([c, np.array(extra, dtype=c.dtype)]), j


def fuzz_world(seed, n_bodies, n_contacts):
    """tests/fuzz_worlds.random_world without joints: speculative and deep points, massless and kinematic bodies, off-centre
    centres of mass, free slots -- and, in the small dense ones, bodies with seven or eight contacts."""
    return fuzz_worlds.random_world(seed, n_bodies=n_bodies, n_contacts=n_contacts, n_joints=0)


def with_free_bodies(world, count=40):
    """The same islands beside dynamic bodies that touch nothing: the world is no longer islands only, so the body prologue and
    epilogue stay and the island kernel runs between them (its non-SELF form)."""
    b, c, j = world
    extra = np.zeros(count, dtype=wire.body_dtype)
    for i in range(count):
        synthetic._dynamic_body(extra[i], -50.0 - 2.0 * i, 30.0 + i, synthetic.BOX_MASS, synthetic.BOX_I)
        extra[i]["linearVelocity"] = (0.5, -0.25 * i)
        extra[i]["angularVelocity"] = 0.125 * i
    return np.concatenate([b, extra]), c.copy(), j.copy()


def box(base, i, j):
    """synthetic.pyramid(base): the body of row i from the ground, column j = i .. base - 1 (body 0 is the ground)."""
    return 1 + i * base - i * (i - 1) // 2 + (j - i)


def pile_with_hub(extra, base=100):
    """A body with 6 + `extra` constraints inside a strip (a ball in the pile): a seventh / eighth interior colour round on that strip.
    One box of the pyramid gets `extra` more contacts with boxes two hops away."""
    b, c, j = common.copy3(synthetic.pyramid(base))
    a0, b0 = c["bodyA"].astype(int), c["bodyB"].astype(int)
    nbrs = {}
    for x, y in zip(a0.tolist(), b0.tolist()):
        nbrs.setdefault(x, set()).add(y), nbrs.setdefault(y, set()).add(x)
    hub = next(i for i in range(len(b) // 2, len(b)) if len(nbrs.get(i, ())) == 6 and b["invMass"][i] > 0)
    two_hops = sorted({t for n in nbrs[hub] for t in nbrs[n] if t != hub and t not in nbrs[hub] and b["invMass"][t] > 0})
    added = c[:extra].copy()
    template = int(np.flatnonzero((a0 == hub) | (b0 == hub))[0])
    for e in range(extra):
        added[e] = c[template]
        added[e]["bodyA"], added[e]["bodyB"] = hub, two_hops[e]
    return b, np.concatenate([c, added]), j


def pile_with_row_hub(extra, base=100, row=30):
    """... the same with partners in the hub's own row (two boxes to the left and to the right): a pyramid's strips are bands of whole rows,
    so the hub's contacts stay inside its strip -- more interior rounds there, no seam the wiser."""
    b, c, j = common.copy3(synthetic.pyramid(base))
    col = (row + base) // 2
    hub = box(base, row, col)
    template = next(i for i in range(len(c)) if int(c[i]["bodyB"]) == hub and c[i]["normal"][0] == 1.0)  # (its left neighbour's side-by-side manifold)
    added = c[:extra].copy()
    for e in range(extra):
        added[e] = c[template]
        added[e]["bodyA"], added[e]["bodyB"] = box(base, row, col + (-2, 2)[e]), hub
    return b, np.concatenate([c, added]), j


def pile(base=100):
    return common.copy3(synthetic.pyramid(base))


def resident_world(base, mixed=False, pile_of=None):
    """synthetic.pyramid_world (a WORLD: shapes, pair states and origins resident beside the solver's arrays) with spare pool slots,
    optionally with manifolds of 0, 1 and 2 points and with the contacts of another pile of the same boxes (pile_of(base): pile_with_hub);
    world["far"] = two boxes many strips apart (the strips of a pyramid are bands of rows)."""
    w = synthetic.pyramid_world(base)
    if pile_of is not None:
        more = len(pile_of(base)[1]) - len(w["contacts"])
        w["contacts"] = pile_of(base)[1]
        pairs = np.zeros(more, dtype=wire.pair_state_dtype)
        pairs["shapeA"], pairs["shapeB"] = w["contacts"]["bodyA"][-more:], w["contacts"]["bodyB"][-more:]  # (one shape per body, same index)
        w["pairs"] = np.concatenate([w["pairs"], pairs])
    if mixed:
        w["contacts"] = with_point_counts((w["bodies"], w["contacts"], w["joints"]))[1]
    spare_c = np.zeros(16, dtype=wire.contact_dtype)
    spare_c["bodyA"], spare_c["bodyB"], spare_c["constraintIndex"] = -1, -1, -1
    spare_p = np.zeros(16, dtype=wire.pair_state_dtype)
    spare_p["shapeA"], spare_p["shapeB"] = -1, -1
    w["contacts"] = np.concatenate([w["contacts"], spare_c])
    w["pairs"] = np.concatenate([w["pairs"], spare_p])
    w["far"] = (box(base, base // 10, base // 10), box(base, 4 * base // 10, 7 * base // 10))
    return w


def far_contact(world, points=2):
    """(slot, contact, pair state) of a contact between the two far boxes: a copy of the manifold of two stacked boxes (solver input, not a
    scene: the geometry is made up), pressed in a little so that the sweeps have something to do; `points` manifold points."""
    a, b = world["far"]
    slot = int(np.flatnonzero(world["pairs"]["shapeA"] < 0)[0])
    c = world["contacts"]
    template = next(i for i in range(len(c)) if c[i]["bodyA"] > 0 and c[i]["normal"][1] == 1.0)
    contacts = c[template:template + 1].copy()
    contacts["bodyA"], contacts["bodyB"], contacts["constraintIndex"], contacts["pointCount"] = a, b, -1, points
    contacts["points"]["separation"] = -0.01
    contacts["points"]["normalImpulse"] = 0.0
    contacts["points"]["tangentImpulse"] = 0.0
    pairs = np.zeros(1, dtype=wire.pair_state_dtype)
    pairs["shapeA"], pairs["shapeB"] = a, b  # (one shape per body, same index)
    return slot, contacts, pairs


# ---- the table ----

class Case:
    def __init__(self, name, solver, options, build, expect, warm=True, chain=False, touch_at=2, steps=3, mixed=False, sliced=0, far_points=2):
        self.name, self.solver, self.options, self.build, self.expect = name, solver, dict(options), build, frozenset(expect)
        self.warm, self.chain, self.touch_at, self.steps, self.mixed, self.sliced = warm, chain, touch_at, steps, mixed, sliced
        self.far_points = far_points
        self.forced = (self.options.get("persist_debug", 0) & FORCING_BITS) != 0

    def params(self):
        vel, pos = common.DEFAULT_ITERS[self.solver]
        return wire.StepParams.make(self.solver, 1.0 / 60.0, vel, pos, self.warm)

    def __repr__(self):
        return self.name


def census_delta(before, after):
    """{(family, key)} selected between two hip.variant_census() calls."""
    return {(f, k) for f, keys in after.items() for k, n in keys.items() if n > before[f][k]}


def run_case(hip, case, check_resident=None, on_touch=None):
    """Runs the case on hip.Solver(0); returns the set of (family, key) the launchers selected in it.
    check_resident(s, step, pre): called after every step; on_touch(slot, contact): a chain case has created this contact."""
    params = case.params()
    before = hip.variant_census()
    with hip.Solver(0) as s:
        for k, v in case.options.items():
            s.set_option(k, v)
        if not case.chain:
            pre = case.build()
            if case.mixed:
                assert {0, 1, 2} <= set(np.unique(pre[1]["pointCount"][pre[1]["bodyA"] >= 0]).tolist()), case.name
            s.upload(*pre)
            for step in range(case.steps):
                s.step_resident(params)
                if check_resident is not None:
                    check_resident(s, step, pre)
        else:
            from tests import world_chain
            world = case.build()
            if case.mixed:
                assert {0, 1, 2} <= set(np.unique(world["contacts"]["pointCount"][world["contacts"]["bodyA"] >= 0]).tolist()), case.name
            s.set_option("async_build_delay", 1000)  # (the worker's structure is never adopted inside the case: the steps stay in the form)
            s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
            # Every live contact handed over once more, unchanged, as a caller that updates its contacts does.  The upload of a world reads
            # the slots' point counts back from a kernel's output; the stand-in runtime of tests/hostcheck runs no kernel, and this call
            # gives the host the same counts there as on the GPU -- so the same cases select the same two-point / per-point forms on both.
            live = np.flatnonzero(world["pairs"]["shapeA"] >= 0).astype(np.int32)
            s.world_set_contacts(live, world["contacts"][live], world["pairs"][live])
            pre = (world["bodies"], world["contacts"], world["joints"])
            seen = []
            for step in range(case.touch_at + case.steps):
                if step == case.touch_at:
                    a, b = world["far"]
                    owner, _seam, strips = s.strip_owners(len(world["bodies"]))
                    assert strips > 4 and owner[a] >= 0 and owner[b] >= 0 and abs(int(owner[a]) - int(owner[b])) >= 3, (strips, owner[a], owner[b])
                    slot, contacts, pairs = far_contact(world, case.far_points)
                    s.world_set_contacts(np.array([slot], dtype=np.int32), contacts, pairs)
                    if on_touch is not None:
                        on_touch(slot, contacts[0])
                s.step_resident(params)
                st = s.stats()
                seen.append((st["overflowContacts"], st["slicedStep"]))
                if check_resident is not None:
                    check_resident(s, step, pre)
            # the form the case is about has run in every step behind the touch (stats: as tests/test_gpu_world.py reads them)
            assert all(x == (0, 0) for x in seen[:case.touch_at]) and all(x == (1, case.sliced) for x in seen[case.touch_at:]), (case.name, seen)
    return census_delta(before, hip.variant_census())


def _cases():
    out = []
    two_or_mixed = ((2, False), (0, True))

    def points_of(build, mixed):
        return (lambda: with_point_counts(build())) if mixed else build

    def add(name, solver, options, build, expect, **kw):
        out.append(Case(name, solver, dict({"strip_patience": 0}, **options), build, expect, **kw))

    width = {"strip_min_bodies": 0, "strip_retry": 0}  # (with "strip_bodies": the strips as wide as the case says, no search)
    # wideStepKernel, plain form: every layout on a partition that NEEDS it (no forcing bit) -- the pile as it is (six interior and two seam
    # rounds: <3, 2>), with a box of seven contacts across a seam at three strip widths (a third seam round: <3, 3>; a fourth: <3, 2, 2>; and a
    # seventh interior round beside it: <3, 2, 2, 2>), with such a box inside a thick strip (a seventh interior round alone: <4, 2>)
    natural = [("3_2", L32, pile, {}), ("3_3", L33, lambda: pile_with_hub(1), dict(width, strip_bodies=16)),
               ("4_2", L42, lambda: pile_with_row_hub(1), dict(width, strip_bodies=320)), ("3_2_2", L322, lambda: pile_with_hub(1), {}),
               ("3_2_2_2", L3222, lambda: pile_with_hub(1), dict(width, strip_bodies=160))]
    for solver in ("TGS_Soft", "PGS_Soft"):
        for tag, layout, build, options in natural:
            for points, mixed in two_or_mixed:
                add("wide_%s_%s_p%d" % (tag, solver, points), solver, options, points_of(build, mixed), [wide(solver, points, layout)], mixed=mixed)
    for points, mixed in two_or_mixed:
        add("wide_3_2_SoftStep_p%d" % points, "SoftStep", {}, points_of(pile, mixed), [wide("SoftStep", points, L32)], mixed=mixed)
    # ... its sliced and overflow forms, on a resident world where a created contact waits behind the strips: every layout the kind has,
    # the roomier ones forced by "persist_debug" (<3, 2, 2, 2>: on the partition that needs it).  The steps
    # before the contact run the plain form of the same layout.
    forced = [("3_2", L32, 0, {}, 0), ("3_3", L33, 0, {"persist_debug": FORCE_THIRD_SEAM}, 0), ("4_2", L42, 0, {"persist_debug": FORCE_FOURTH_PAIR}, 0),
              ("3_2_2", L322, 0, {"persist_debug": FORCE_PARKED}, 0), ("3_2_2_2", L3222, 1, dict(width, strip_bodies=160), 1)]
    for solver in ("TGS_Soft", "PGS_Soft", "SoftStep"):
        for tag, layout, hub, options, _ in (forced if solver != "SoftStep" else forced[:1]):
            for form, name, overflow_kernel in ((SLICED, "sliced", 0), (OVERFLOW, "overflow", 1)):
                for points, mixed in two_or_mixed:
                    add("wide_%s_%s_%s_p%d" % (name, tag, solver, points), solver, dict(options, overflow_kernel=overflow_kernel),
                        (lambda mixed=mixed, hub=hub: resident_world(100, mixed, (lambda base: pile_with_hub(1, base)) if hub else None)), [wide(solver, points, layout), wide(solver, points, layout, form)],
                        chain=True, mixed=mixed, sliced=2 if overflow_kernel else 1)
        # (the overflow contact is not a strip constraint: a single point on it leaves the strips on their two-point forms, and the sweep
        # behind them masks per point)
        for form, name, overflow_kernel in ((SLICED, "sliced", 0), (OVERFLOW, "overflow", 1)):
            add("wide_%s_one_point_far_%s" % (name, solver), solver, {"overflow_kernel": overflow_kernel}, lambda: resident_world(100),
                [wide(solver, 2, L32), wide(solver, 2, L32, form)], chain=True, sliced=2 if overflow_kernel else 1, far_points=1)
    # ... and the two optional modes of s2Solve_TGS_Soft (the step that builds the structure runs between the body prologue and epilogue: plain)
    for points, mixed in two_or_mixed:
        build = points_of(pile, mixed)
        add("wide_self_p%d" % points, "TGS_Soft", {"self_contained_strips": 1}, build, [wide("TGS_Soft", points, L32), wide("TGS_Soft", points, L32, SELF)], mixed=mixed)
        add("wide_bodywarm_p%d" % points, "TGS_Soft", {"strip_body_warm": 1}, build, [wide("TGS_Soft", points, L32, BODYWARM)], mixed=mixed)
    add("wide_self_bodywarm_p2", "TGS_Soft", {"self_contained_strips": 1, "strip_body_warm": 1}, pile,
        [wide("TGS_Soft", 2, L32, BODYWARM), wide("TGS_Soft", 2, L32, SELF | BODYWARM)])
    # (mixed point counts with both: the self-contained form with the coloured warm start -- wide_kernel.hip: wideKey)
    add("wide_self_bodywarm_p0", "TGS_Soft", {"self_contained_strips": 1, "strip_body_warm": 1}, points_of(pile, True),
        [wide("TGS_Soft", 0, L32, BODYWARM), wide("TGS_Soft", 0, L32, SELF)], mixed=True)

    # the 256-thread persistent kernels ("wide" = 0): two lanes per constraint, or one -- with TGS_Soft's seam records in registers (the
    # per-point kernel whatever the counts) or in LDS, and in eight rounds on the partition with a seventh interior round
    eight = (lambda: pile_with_hub(1), dict(width, strip_bodies=160))
    for solver in ("TGS_Soft", "PGS_Soft", "SoftStep"):
        for points, mixed in two_or_mixed:
            add("pair_%s_p%d" % (solver, points), solver, {"wide": 0, "pair_lanes": 1}, points_of(pile, mixed), [pair_step(solver, points)], mixed=mixed)
            add("strip_6_%s_p%d" % (solver, points), solver, {"wide": 0, "pair_lanes": 0, "seam_regs": 0}, points_of(pile, mixed), [strip_step(solver, points, 6)], mixed=mixed)
            add("strip_8_%s_p%d" % (solver, points), solver, dict(eight[1], wide=0, pair_lanes=0), points_of(eight[0], mixed), [strip_step(solver, points, 8)], mixed=mixed)
        # neither persistent kernel: one lean launch per sweep and phase, the warm start folded into the interiors' first
        add("soft_%s" % solver, solver, {"persist": 0}, pile, [strip_soft(solver, True), strip_soft(solver, False)])
    add("strip_seamregs_TGS_Soft", "TGS_Soft", {"wide": 0, "pair_lanes": 0, "seam_regs": 1}, points_of(pile, True), [strip_step("TGS_Soft", 0, 6, 1)], mixed=True)

    # resident islands: a world of nothing else (the first step between the body launches, then the kernel alone), the same beside free bodies,
    # groups of six and of eight rounds (s2Solve_SoftStep's eight-round groups stay on islandStepKernel), and "wide" = 0
    islands = [(6, 2, mixed_pyramids), (6, 0, mixed_point_counts), (8, 2, hub_pyramids), (8, 0, lambda: with_point_counts(hub_pyramids()))]
    for solver in ("TGS_Soft", "PGS_Soft", "SoftStep"):
        for rounds, points, build in islands:
            mixed = points == 0
            if solver == "SoftStep" and rounds == 8:
                add("island_%s_r8_p%d" % (solver, points), solver, {}, build, [island_step(solver, 8)], mixed=mixed)
                continue
            add("wide_island_%s_r%d_p%d" % (solver, rounds, points), solver, {}, build,
                [wide_island(solver, rounds, False, points), wide_island(solver, rounds, True, points)], mixed=mixed)
            add("wide_island_free_%s_r%d_p%d" % (solver, rounds, points), solver, {}, (lambda build=build: with_free_bodies(build())),
                [wide_island(solver, rounds, False, points)], mixed=mixed)
        for rounds, build in ((6, mixed_point_counts), (8, hub_pyramids)):
            add("island_%s_r%d_wide0" % (solver, rounds), solver, {"wide": 0}, build, [island_step(solver, rounds)], mixed=rounds == 6)
        add("island_fuzz_%s" % solver, solver, {"max_group_bodies": 64}, lambda: fuzz_world(0, 60, 90),
            [island_step(solver, 8)] if solver == "SoftStep" else [wide_island(solver, 8, False, 0)])  # (massless and kinematic bodies: the body launches stay)

    # cold start (warmStart false): one case per family and kind -- a plan without a warm start is given its kind's (Executor::softPlan)
    for solver in ("TGS_Soft", "PGS_Soft", "SoftStep"):
        mixed_pile = points_of(pile, True)
        add("cold_wide_%s" % solver, solver, {}, mixed_pile, [wide(solver, 0, L32)], warm=False, mixed=True)
        add("cold_pair_%s" % solver, solver, {"wide": 0, "pair_lanes": 1}, mixed_pile, [pair_step(solver, 0)], warm=False, mixed=True)
        add("cold_strip_%s" % solver, solver, {"wide": 0, "pair_lanes": 0, "seam_regs": 0}, pile, [strip_step(solver, 2, 6)], warm=False)
        add("cold_soft_%s" % solver, solver, {"persist": 0}, mixed_pile, [strip_soft(solver, False)], warm=False, mixed=True)
        add("cold_wide_island_%s" % solver, solver, {}, mixed_point_counts, [wide_island(solver, 6, False, 0), wide_island(solver, 6, True, 0)], warm=False, mixed=True)
        add("cold_island_%s" % solver, solver, {"wide": 0}, hub_pyramids, [island_step(solver, 8)], warm=False)
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
