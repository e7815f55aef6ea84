"""The instruction streams of the 512-thread kernels (wide_kernel.hip: warmWide, prepWide, chainWide inside wideStepKernel and
wideIslandKernel) were shortened: the records are kept opaque to the compiler without an instruction (opaqueWide, not an XORed zero), the
prep hands the chain each point's soft scales, the last friction application stands in front of the write-bit branches and the velocity
records are read whole.  None of them may change a bit.  Small worlds -- pyramids of base 12 to 24 (the strips: base 16 in three strips, one of them with two seams), the strip and group limits forced down as
the cases of tests/variant_cases.py force them -- on the forms those edits sit in:

  * the plain <3, 2> strip form, two-point (the headline's variant) and per-point;
  * a form whose local anchors wait in LDS (<3, 3>: prepWide / warmWide LL);
  * a form with parked rounds (<3, 2, 2>: the records come through unparkWide);
  * the six- and the eight-round island form, between the body launches (step 0) and as the step's only launch (SELF).

Every world holds a one-point manifold (the masked POINTS path) unless it is the two-point case, a constraint with a static side (bit
30: the doubled hertz, the second soft triple) and a constraint whose write bit is off on one side (the ground's); each case asserts
that.  Three resident steps, every step compared BIT FOR BIT with the oracle swept in the order the device reports, and the variant
census must name the form the case is about.  The same cases on the tolerance-mode library within tests/test_gpu_fast.py's bound
(rtol 1e-5 per sweep, norm-wise, every step from the state the library itself left)."""
import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import common, oraclebind, variant_cases
from tests.variant_cases import L32, L33, L322, hub_pyramids, mixed_pyramids, wide, wide_island, with_point_counts

pytestmark = pytest.mark.gpu

STRIPS = {"strip_patience": 0, "max_group_bodies": 48, "strip_min_bodies": 0, "strip_bodies": 40, "strip_retry": 0}
ISLANDS = {"strip_patience": 0}


def pile16():
    return common.copy3(synthetic.pyramid(16))


def small_islands():
    return mixed_pyramids((12, 17, 24, 14))


# name -> (builder, options, the (family, key) entries that must have run)
CASES = {
    "strip_3_2_p2": (pile16, STRIPS, [wide("TGS_Soft", 2, L32)]),
    "strip_3_2_p0": (lambda: with_point_counts(pile16()), STRIPS, [wide("TGS_Soft", 0, L32)]),
    "strip_locals_in_lds_p0": (lambda: with_point_counts(pile16()), dict(STRIPS, persist_debug=variant_cases.FORCE_THIRD_SEAM), [wide("TGS_Soft", 0, L33)]),
    "strip_parked_p0": (lambda: with_point_counts(pile16()), dict(STRIPS, persist_debug=variant_cases.FORCE_PARKED), [wide("TGS_Soft", 0, L322)]),
    "island_r6_p2": (small_islands, ISLANDS, [wide_island("TGS_Soft", 6, False, 2), wide_island("TGS_Soft", 6, True, 2)]),
    "island_r6_p0": (lambda: with_point_counts(small_islands()), ISLANDS, [wide_island("TGS_Soft", 6, False, 0), wide_island("TGS_Soft", 6, True, 0)]),
    "island_r8_p2": (hub_pyramids, ISLANDS, [wide_island("TGS_Soft", 8, False, 2), wide_island("TGS_Soft", 8, True, 2)]),
    "island_r8_p0": (lambda: with_point_counts(hub_pyramids()), ISLANDS, [wide_island("TGS_Soft", 8, False, 0), wide_island("TGS_Soft", 8, True, 0)]),
}
PARAMS = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
WORLDS = {}


def world_of(name):
    """Built once per case and shared by the two libraries' tests (each steps a copy)."""
    if name not in WORLDS:
        b, c, j = CASES[name][0]()
        live = c["bodyA"] >= 0
        static = b["invMass"] == 0
        side = static[c["bodyA"][live]] != static[c["bodyB"][live]]
        assert (side & (c["pointCount"][live] > 0)).any(), "no constraint with a static side (its write bit off on that side)"
        if name.endswith("_p0"):
            assert {0, 1, 2} <= set(np.unique(c["pointCount"][live]).tolist()), "no one-point manifold"
        else:
            assert set(np.unique(c["pointCount"][live]).tolist()) == {2}
        WORLDS[name] = (b, c, j)
    return WORLDS[name]


def run(name, fast):
    pre = world_of(name)
    _, options, expect = CASES[name]
    before = hip.variant_census(fast)
    with hip.Solver(0, fast=fast) as s:
        for k, v in options.items():
            s.set_option(k, v)
        s.upload(*pre)
        want = common.copy3(pre)
        for step in range(3):
            s.step_resident(PARAMS)
            order, _ = s.contact_order()
            jorder, _ = s.joint_order()
            got = common.copy3(pre)
            s.download(*got)
            oraclebind.solve(PARAMS, *want, contact_order=order, joint_order=jorder)
            what = "%s%s step %d (resident kernel %r)" % (name, " fast" if fast else "", step, s.resident_kernel())
            if fast:
                common.compare_close(got, want, common.sweeps_touching_bodies(PARAMS), what, rtol_per_sweep=common.FAST_RTOL_PER_SWEEP, params=PARAMS)
                want = common.copy3(got)  # (the next step from what the library left: the bound is per solve)
            else:
                common.compare_exact(got, want, what)
    after = hip.variant_census(fast)
    ran = variant_cases.census_delta(before, after)
    assert set(expect) <= ran, "%s: expected %s, the launchers selected %s" % (name, sorted(expect), sorted(ran))


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_on_the_form(name):
    run(name, False)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tolerance_library_on_the_form(name):
    run(name, True)
