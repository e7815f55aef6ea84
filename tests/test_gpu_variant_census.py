"""Every entry of the six variant tables of the register-resident soft kernels (launch.h: KernelVariant -- wideStepKernel, wideIslandKernel,
stripStepKernel, islandStepKernel, stripSoftKernel, pairStepKernel) RUN on the GPU and bit-exact: the cases of tests/variant_cases.py, each
stepped resident through the C-ABI, every step compared with the oracle swept in the contact and joint order the device reports
(tests/common.py: compare_exact -- the project's gate, no tolerance), and each case's variant census (s2amd_get_variant_entry: which
entries the launchers selected while it ran) equal to the set the table states.  So "bit-exact" is a statement about THAT instantiation,
not about whatever the host fell back to.  The last test asserts that the union of what this file's cases selected is the library's whole
enumeration: a table entry exists if and only if a case here runs it.  There is no exemption list.

tests/test_variant_reach_host.py checks the same table's host side without a GPU."""
import numpy as np
import pytest

from solver2d_amd import hip
from tests import common, oraclebind, variant_cases

pytestmark = pytest.mark.gpu


def run_exact(case):
    """The case on the GPU, every step against the oracle; returns what the census says it selected."""
    state = {}
    params = case.params()

    def check(s, step, pre):
        if "want" not in state:
            state["want"] = common.copy3(pre)
        order, _ = s.contact_order()
        jorder, _ = s.joint_order()
        got = common.copy3(pre)
        s.download(*got)
        oraclebind.solve(params, *state["want"], contact_order=order, joint_order=jorder)
        st = s.stats()
        common.compare_exact(got, state["want"], "%s step %d (launches %d, persistent %d, pairLanes %d, sliced %d, resident kernel %r)" % (
            case.name, step, st["kernelLaunches"], st["persistent"], st["pairLanes"], st["slicedStep"], s.resident_kernel()))

    def touched(slot, contact):
        state["want"][1][slot] = contact  # (the oracle's side of s2amd_world_set_contacts)

    return variant_cases.run_case(hip, case, check_resident=check, on_touch=touched)


@pytest.mark.parametrize("case", variant_cases.CASES, ids=[c.name for c in variant_cases.CASES])
def test_case_is_bit_exact_on_exactly_its_variants(case):
    got = run_exact(case)
    print(case.name, sorted(got))
    assert got == set(case.expect), "%s: selected but not expected %s; expected but not selected %s" % (
        case.name, sorted(got - set(case.expect)), sorted(set(case.expect) - got))


def test_the_union_of_the_cases_is_the_whole_enumeration():
    """Self-contained (it depends on no other test having run): every case once more, each step exact, and the union of their census
    deltas against the enumeration of all six tables."""
    entries = {(family, key) for family, keys in hip.variant_census().items() for key in keys}
    selected = set()
    for case in variant_cases.CASES:
        selected |= run_exact(case)
    assert not entries - selected, "table entries no case runs (delete them or give them a case): %s" % sorted(entries - selected)
    assert not selected - entries, "cases selected entries the tables do not list: %s" % sorted(selected - entries)
    assert set().union(*[c.expect for c in variant_cases.CASES]) == entries
