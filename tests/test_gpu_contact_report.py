"""The contact report of the resident world (s2amd_world_set_report / _touch_events / _touching / _body_sums; solver2d_amd/csrc/
contact_report.hip) against its numpy statement (tests/contact_report_ref.py) on the oracle chain of tests/world_chain.py, stepped in
the order the device reports: every list, every record, every sum equal byte for byte."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import common, contact_report_ref as ref, world_chain
from tests.world_chain import oracle_find_pairs, oracle_world_step, rain_world
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, refuses, upload
from tests.world_chain import _create_contacts

pytestmark = pytest.mark.gpu


def assert_report_equals_reference(s, prev, world, what, totals=None, status=None):
    """The three getters against the reference statement on `world` (the oracle chain after the step) and the touching state before it."""
    want_began, want_ended = ref.events(prev, world)
    began, ended = s.world_touch_events()
    assert began.tolist() == want_began.tolist(), what + ": began"
    assert ended.tolist() == want_ended.tolist(), what + ": ended"
    want = ref.touching(world)
    got = s.world_touching(expected=max(len(want), 1))
    assert len(got) == len(want), "%s: %d touching records, reference %d" % (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        raise AssertionError("%s: touching records differ in %s" % (what, bad))
    want_sums = ref.body_sums(world)
    sums = s.world_body_sums()
    if sums.tobytes() != want_sums.tobytes():
        rows = np.flatnonzero([sums[i].tobytes() != want_sums[i].tobytes() for i in range(len(sums))])
        raise AssertionError("%s: body sums differ in rows %s: %s / %s" % (what, rows[:5].tolist(), sums[rows[:3]], want_sums[rows[:3]]))
    if totals is not None:
        totals["began"] += len(began)
        totals["ended"] += len(ended)
        totals["both"] += 1 if len(began) and len(ended) else 0
        totals["points"].update(got["pointCount"].tolist())
        totals["degree"] = max(totals["degree"], int(sums["touching"].max()))
        if status is not None:
            totals["ended_separated"] += int((status[ended] == wire.PAIR_SEPARATED).sum())


def whole_loop(s, params, world, steps, what, report_every=1, world_every=3, before_step=None):
    """The whole s2World_Step loop like tests/test_gpu_world.py: test_rain_world_loop, with the report checked against the oracle chain."""
    ref_world = world_chain.copy_world(world)
    totals = {"began": 0, "ended": 0, "both": 0, "ended_separated": 0, "points": set(), "degree": 0}
    upload(s, world)
    prev = ref.before_of(ref_world["contacts"])
    for step in range(steps):
        if world_chain.moved_any(ref_world):
            got = s.world_find_pairs()
            want = oracle_find_pairs(ref_world)
            assert np.array_equal(got, want), "%s step %d: new pairs" % (what, step)
            if len(got):
                slots, contacts, pairs = _create_contacts(ref_world, got)
                s.world_set_contacts(slots, contacts, pairs)
                prev[slots] = ref.before_of(contacts)
        if before_step is not None:
            before_step(step)
        info = s.world_step(params)
        order, _ = s.contact_order()
        status = oracle_world_step(params, ref_world, contact_order=order)
        assert info["separatedCount"] == int((status == wire.PAIR_SEPARATED).sum()), "%s step %d" % (what, step)
        if step % report_every == report_every - 1:
            assert_report_equals_reference(s, prev, ref_world, "%s step %d" % (what, step), totals, status)
        prev = ref.touching_mask(ref_world)
        if step % world_every == world_every - 1:
            got_world, _ = download(s, world)
            world_chain.assert_device_equals_oracle(got_world, ref_world, "%s step %d" % (what, step))
    return totals


@pytest.mark.parametrize("seed,count,solver_name", [(1, 107, "TGS_Soft"), (9, 163, "PGS_NGS_Block"), (6, 142, "Jacobi")])
def test_rain_loops_report_every_step(seed, count, solver_name):
    """Bodies of every shape type rain into a trough: contacts begin and end all the time, pairs separate and are destroyed on the
    device.  All flags on, every step: began / ended, the touching records and the body sums equal the reference statement."""
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        totals = whole_loop(s, params, rain_world(seed, count), 70, "rain %d %s" % (seed, solver_name))
    print(seed, solver_name, totals)
    # the test cannot pass on a quiet world
    assert totals["began"] >= 100 and totals["ended"] >= 50 and totals["both"] >= 10, totals
    assert totals["points"] >= {1, 2} and totals["degree"] >= 8, totals
    if solver_name == "Jacobi":
        # (its contact pass is order-free: the device's chain is the pool-order chain) touching pairs destroyed on the device
        assert totals["ended_separated"] >= 1, totals


def test_report_off_changes_nothing_and_the_getters_refuse():
    """Two solvers in lockstep, one with every flag and one with none: the same world bytes and counters every step; without a flag the
    getters refuse.  So that the comparison is not made on a world without contacts: the CPU oracle chain of this world (pool order)
    has created 69 contacts by the end of step 20, 7 of them touching (the bodies are still falling); half of the first and one of
    the second are required here."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    world = rain_world(3, 120)
    keys = ("separatedCount", "activeContacts", "graphChanged", "movedCount")
    with hip.Solver(0) as on, hip.Solver(0) as off:
        refuses(off, E_STATE, ("world_touch_events", "world_touching", "world_body_sums"))  # no resident world
        on.world_set_report(wire.REPORT_ALL)
        upload(on, world), upload(off, world)
        moved = True
        created = 0
        for step in range(20):
            state, _ = download(on, world)
            if moved:
                new = on.world_find_pairs()
                assert np.array_equal(new, off.world_find_pairs()), "step %d" % step
                if len(new):
                    created += len(new)
                    slots, contacts, pairs = _create_contacts(state, new)
                    on.world_set_contacts(slots, contacts, pairs), off.world_set_contacts(slots, contacts, pairs)
            a, b = on.world_step(params), off.world_step(params)
            assert [a[k] for k in keys] == [b[k] for k in keys], "step %d: %r / %r" % (step, a, b)
            moved = a["movedCount"] > 0
            on.world_touch_events(), on.world_touching(), on.world_body_sums()
            refuses(off, E_STATE, ("world_touch_events", "world_touching", "world_body_sums"))
            (wa, sa), (wb, sb) = download(on, world), download(off, world)
            assert np.array_equal(sa, sb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert created >= 34 and a["activeContacts"] >= 1, (created, a)


def test_flag_subsets_and_unknown_bits():
    params = wire.StepParams.make("PGS", 1.0 / 60.0, 4, 2, True)
    world = synthetic.pyramid_world(12)
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        for bad in (8, 15, -1, 1 << 20):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                s.world_set_report(bad)
        s.world_set_report(wire.REPORT_TOUCH)
        upload(s, world)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_touch_events()  # no step has run since the flag was set
        s.world_step(params)
        oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
        began, ended = s.world_touch_events()
        assert began.tolist() == [] and ended.tolist() == []
        refuses(s, E_STATE, ("world_touching", "world_body_sums"))
        # a flag set between two steps takes effect from the next step
        s.world_set_report(wire.REPORT_ALL)
        refuses(s, E_STATE, ("world_touching", "world_body_sums"))
        prev = ref.touching_mask(ref_world)
        s.world_step(params)
        oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
        assert_report_equals_reference(s, prev, ref_world, "all flags from the second step")
        # ... and one cleared as well
        s.world_set_report(wire.REPORT_BODY_SUMS)
        prev = ref.touching_mask(ref_world)
        s.world_step(params)
        oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
        assert s.world_body_sums().tobytes() == ref.body_sums(ref_world).tobytes()
        refuses(s, E_STATE, ("world_touch_events", "world_touching"))


def test_capacity_errors_set_the_counts_and_consume_nothing():
    """Through the raw C calls: a buffer one entry too small gives S2AMD_E_CAPACITY with the true counts; the same call with room succeeds."""
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    world = synthetic.pyramid_world(12)
    n = len(world["contacts"])
    world["contacts"]["pointCount"] = 0  # live pairs whose manifolds have no points yet: every one of them begins in the first step
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.world_set_report(wire.REPORT_ALL)
        upload(s, world)
        s.world_step(params)
        oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
        want_began, want_ended = ref.events(np.zeros(n, dtype=bool), ref_world)
        assert len(want_began) == n == 210 and len(want_ended) == 0
        nb, ne = ctypes.c_int32(-7), ctypes.c_int32(-7)
        began = np.full(n, -1, dtype=np.int32)
        rc = L.s2amd_world_touch_events(h, wire.as_ptr(began), n - 1, ctypes.byref(nb), None, 0, ctypes.byref(ne))
        assert (rc, nb.value, ne.value) == (E_CAPACITY, n, 0)
        rc = L.s2amd_world_touch_events(h, wire.as_ptr(began), n, ctypes.byref(nb), None, 0, ctypes.byref(ne))
        assert (rc, nb.value, ne.value) == (0, n, 0) and began.tolist() == want_began.tolist()
        out = np.zeros(n, dtype=wire.touching_contact_dtype)
        count = ctypes.c_int32(-7)
        rc = L.s2amd_world_touching(h, wire.as_ptr(out), n - 1, ctypes.byref(count))
        assert (rc, count.value) == (E_CAPACITY, n)
        rc = L.s2amd_world_touching(h, wire.as_ptr(out), n, ctypes.byref(count))
        assert (rc, count.value) == (0, n) and out.tobytes() == ref.touching(ref_world).tobytes()
        sums = np.zeros(len(world["bodies"]), dtype=wire.body_contact_sum_dtype)
        assert L.s2amd_world_body_sums(h, wire.as_ptr(sums), len(sums) - 1) == E_CAPACITY
        assert L.s2amd_world_body_sums(h, wire.as_ptr(sums), len(sums)) == 0 and sums.tobytes() == ref.body_sums(ref_world).tobytes()
        # the Python getters, asked afterwards, see the same step
        b2, e2 = s.world_touch_events(expected=1)
        assert b2.tolist() == want_began.tolist() and e2.tolist() == []


def test_uploaded_manifolds_do_not_begin_and_a_callers_destroy_does_not_end():
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    world = synthetic.pyramid_world(12)
    assert int((world["contacts"]["pointCount"] > 0).sum()) == len(world["contacts"]) == 210
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        upload(s, world)
        prev = ref.before_of(ref_world["contacts"])
        for step in range(3):
            s.world_step(params)
            oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
            began, ended = s.world_touch_events()
            assert len(began) == 0 and len(ended) == 0 and len(s.world_touching()) == 210, "step %d" % step
            assert_report_equals_reference(s, prev, ref_world, "resting pyramid step %d" % step)
            prev = ref.touching_mask(ref_world)
        # the caller's own s2DestroyContact of a touching slot
        victim = 100
        assert prev[victim]
        gone_c = np.zeros(1, dtype=wire.contact_dtype)
        gone_c["constraintIndex"] = -1
        gone_p = np.zeros(1, dtype=wire.pair_state_dtype)
        gone_p["shapeA"] = gone_p["shapeB"] = -1
        s.world_set_contacts(np.array([victim], dtype=np.int32), gone_c, gone_p)
        ref_world["contacts"][victim], ref_world["pairs"][victim] = gone_c[0], gone_p[0]
        prev[victim] = False
        s.world_step(params)
        oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
        began, ended = s.world_touch_events()
        assert victim not in ended.tolist() and len(s.world_touching()) == 209
        assert_report_equals_reference(s, prev, ref_world, "after the caller's destroy")


def test_report_reads_what_the_one_launch_island_kernel_stores():
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    world = synthetic.pyramid_world(40)
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        upload(s, world)
        prev = ref.before_of(ref_world["contacts"])
        kernels = []
        for step in range(5):
            s.world_step(params)
            kernels.append(s.resident_kernel())
            oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
            assert_report_equals_reference(s, prev, ref_world, "pyramid40 step %d" % step)
            prev = ref.touching_mask(ref_world)
        got_world, _ = download(s, world)
        world_chain.assert_device_equals_oracle(got_world, ref_world, "pyramid40")
    assert kernels[-1][0] == 4, kernels  # S2AMD_RESIDENT_WIDE_ONLY_LAUNCH


def test_report_reads_what_the_strip_paths_store():
    """tests/test_gpu_world.py: test_rain_world_loop_through_the_strip_paths' world and options for seed 9: the report reads the wire
    arrays every path stores into, not one path's side arrays."""
    seed, solver_name = 9, "TGS_Soft"
    rng = np.random.default_rng(5000 + seed)
    vel, pos = common.DEFAULT_ITERS[solver_name]
    params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
    world = rain_world(seed, int(rng.integers(300, 900)), spin=bool(seed % 2))
    with hip.Solver(0) as s:
        s.set_option("strip_patience", int(rng.integers(0, 3)))
        s.set_option("strip_min_bodies", 0)
        s.set_option("strip_bodies", int(rng.integers(30, 160)))
        s.set_option("max_group_bodies", int(rng.choice([32, 64, 128])))
        s.world_set_report(wire.REPORT_ALL)
        totals = whole_loop(s, params, world, 30, "rain-strips", report_every=5, world_every=5)
    assert totals["began"] > 0, totals


def test_a_body_with_more_entries_than_a_wave():
    """Base-66 pyramid: the static ground (body 0) touches 66 boxes -- its sum is gathered in two batches of the wave that owns it."""
    params = wire.StepParams.make("PGS_Soft", 1.0 / 60.0, *common.DEFAULT_ITERS["PGS_Soft"], True)
    world = synthetic.pyramid_world(66)
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        s.world_set_report(wire.REPORT_ALL)
        upload(s, world)
        prev = ref.before_of(ref_world["contacts"])
        for step in range(3):
            s.world_step(params)
            oracle_world_step(params, ref_world, contact_order=s.contact_order()[0])
            want = ref.body_sums(ref_world)
            assert want["touching"][0] == 66 and want["normalImpulse"][0] > 0
            got = s.world_body_sums()
            assert got[0].tobytes() == want[0].tobytes(), "step %d: ground %s / %s" % (step, got[0], want[0])
            assert_report_equals_reference(s, prev, ref_world, "pyramid66 step %d" % step)
            prev = ref.touching_mask(ref_world)
