"""The episodes without a GPU: the interface as declared and bound with the header's sizes and offsets, the statement
(tests/episode_ref.py) on hand-made cases with exactly representable numbers -- every kind and shape, OUTSIDE, a test exactly at a bound,
a NaN, the order of the float sum, every status in the stated priority order, the time limit beside a fired rule, the restart, the
re-base --, the setter's validation cases as data, the compiler's resource report of the new kernels, and the host side under
ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded)."""
import re

import numpy as np

from solver2d_amd import wire
from tests import episode_ref as ref, hostcheck_util

CALLS = ("s2amd_world_set_episodes", "s2amd_world_set_episode_report", "s2amd_world_episode_rewards", "s2amd_world_episode_flags",
         "s2amd_world_export_episode_step", "s2amd_world_export_episode_step_async", "s2amd_world_episode_states",
         "s2amd_world_episode_rule_states", "s2amd_world_episode_events", "s2amd_world_episode_counts")
F = np.float32
INF = F(np.inf)
VALUE, TEST, TERMINATE, TRUNCATE = ref.REWARD_VALUE, ref.REWARD_TEST, ref.TERMINATE, ref.TRUNCATE
OUTSIDE, OFF, DIFFERENCE = wire.EPISODE_RULE_OUTSIDE, wire.EPISODE_RULE_DISABLED, wire.EPISODE_RULE_DIFFERENCE
rule = wire.episode_rule


def bits(x):
    return np.atleast_1d(np.array(x, dtype=F)).view(np.uint32).reshape(-1).tolist()


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    hostcheck_util.assert_struct_layout(tmp_path, {"s2amdEpisodeRule": wire.episode_rule_dtype, "s2amdEpisodeState": wire.episode_state_dtype,
                                                   "s2amdEpisodeRuleState": wire.episode_rule_state_dtype, "s2amdEpisodeEvent": wire.episode_event_dtype})
    assert (wire.EPISODE_RULE_SIZE, wire.EPISODE_STATE_SIZE, wire.EPISODE_RULE_STATE_SIZE, wire.EPISODE_EVENT_SIZE) == (64, 32, 32, 16)


def test_header_defines_and_bindings():
    defines = {"S2AMD_MAX_EPISODE_AGENTS": wire.MAX_EPISODE_AGENTS, "S2AMD_MAX_EPISODE_RULES": wire.MAX_EPISODE_RULES,
               "S2AMD_EPISODE_REWARD_VALUE": ref.REWARD_VALUE, "S2AMD_EPISODE_REWARD_TEST": ref.REWARD_TEST, "S2AMD_EPISODE_TERMINATE": ref.TERMINATE,
               "S2AMD_EPISODE_TRUNCATE": ref.TRUNCATE, "S2AMD_EPISODE_SHAPE_LINEAR": ref.LINEAR, "S2AMD_EPISODE_SHAPE_ABS": ref.ABS,
               "S2AMD_EPISODE_SHAPE_SQUARE": ref.SQUARE, "S2AMD_EPISODE_RULE_DISABLED": wire.EPISODE_RULE_DISABLED,
               "S2AMD_EPISODE_RULE_DIFFERENCE": wire.EPISODE_RULE_DIFFERENCE, "S2AMD_EPISODE_RULE_OUTSIDE": wire.EPISODE_RULE_OUTSIDE,
               "S2AMD_EPISODE_STATUS_EVALUATED": ref.EVALUATED, "S2AMD_EPISODE_STATUS_DISABLED": ref.DISABLED, "S2AMD_EPISODE_STATUS_SKIPPED": ref.SKIPPED,
               "S2AMD_EPISODE_STATUS_SOURCE_OFF": ref.SOURCE_OFF, "S2AMD_EPISODE_TERMINATED": ref.TERMINATED, "S2AMD_EPISODE_TRUNCATED": ref.TRUNCATED,
               "S2AMD_EPISODE_TIME_LIMIT": ref.TIME_LIMIT, "S2AMD_EPISODE_REPORT_STEP": wire.EPISODE_REPORT_STEP,
               "S2AMD_EPISODE_REPORT_STATES": wire.EPISODE_REPORT_STATES, "S2AMD_EPISODE_REPORT_RULE_STATES": wire.EPISODE_REPORT_RULE_STATES,
               "S2AMD_EPISODE_REPORT_EVENTS": wire.EPISODE_REPORT_EVENTS, "S2AMD_API_VERSION": 5}
    header = hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_EPISODE_AGENTS, wire.MAX_EPISODE_RULES, wire.API_VERSION) == (16384, 65536, 5)
    assert (wire.EPISODE_RULE_DISABLED, wire.EPISODE_RULE_DIFFERENCE, wire.EPISODE_RULE_OUTSIDE) == (1, 2, 4)
    assert (wire.EPISODE_REPORT_STEP, wire.EPISODE_REPORT_STATES, wire.EPISODE_REPORT_RULE_STATES, wire.EPISODE_REPORT_EVENTS, wire.EPISODE_REPORT_ALL) == (1, 2, 4, 8, 15)
    # the observers' "Not offered" points here and names what remains
    assert re.search(r"Rewards and termination are the episode report's", header) and "resetting the bodies of a finished agent" in header


# ---- the statement on hand-made cases ----
# two frames of four channels; channel 3 of this step is a NaN
OBS = np.array([[2.0, -3.0, 0.5, np.nan], [1.5, -1.0, 0.5, 4.0]], dtype=F)


def one(r, obs=OBS, dims=None):
    rules = wire.episode_rule_list([r])
    assert ref.valid(rules, int(r["agent"]) + 1) == -1
    out = ref.step(ref.Accounting(int(r["agent"]) + 1), obs, rules, int(r["agent"]) + 1, None, dims)
    st = out["rule_states"][0]
    assert st["rule"] == 0 and out["counts"][st["status"]] == 1 and out["counts"][:4].sum() == 1
    assert bits(out["rewards"][int(r["agent"])]) == bits(F(0.0) + st["value"] if st["status"] == ref.EVALUATED else 0.0)
    return st, out


def test_every_kind_and_shape():
    # x = -3 through the three shapes: -3, 3, 9
    shaped = {ref.LINEAR: -3.0, ref.ABS: 3.0, ref.SQUARE: 9.0}
    for shape, f in shaped.items():
        st, out = one(rule(VALUE, 0, 1, shape=shape, gain=0.5, bias=1.0))
        assert (st["x"], st["f"], st["value"], st["fired"]) == (-3.0, f, 0.5 * f + 1.0, 0) and out["flags"][0] == 0
        # the clamp takes the rule's bounds
        assert one(rule(VALUE, 0, 1, shape=shape, gain=2.0, lower=-4.0, upper=5.0))[0]["value"] == max(-4.0, min(5.0, 2.0 * f))
        # a test: f inside [2.5, 9] or not
        st, _ = one(rule(TEST, 0, 1, shape=shape, gain=7.0, bias=-2.0, lower=2.5, upper=9.0))
        assert st["value"] == (7.0 if f >= 2.5 else -2.0) and st["fired"] == 0
        for kind, bit in ((TERMINATE, ref.TERMINATED), (TRUNCATE, ref.TRUNCATED)):
            st, out = one(rule(kind, 0, 1, shape=shape, gain=-5.0, lower=2.5, upper=9.0))
            fired = f >= 2.5
            assert st["fired"] == int(fired) and bits(st["value"]) == bits(-5.0 if fired else 0.0)
            assert out["flags"][0] == (bit if fired else 0) and out["states"]["rule"][0] == (0 if fired else -1)
            assert len(out["events"]) == int(fired) and out["counts"][4:].tolist() == [int(fired), int(fired and kind == TERMINATE), int(fired and kind == TRUNCATE), 0]
    # the square is one multiply: 2^-75 squared underflows to +0, 3e20 squared overflows
    assert bits(one(rule(VALUE, 0, 0, shape=ref.SQUARE), obs=np.array([[2.0 ** -75]], dtype=F))[0]["f"]) == [0]
    assert one(rule(VALUE, 0, 0, shape=ref.SQUARE), obs=np.array([[3e20]], dtype=F))[0]["f"] == INF
    # a difference is one subtract: frame 0 minus frame 1 of channel 0, and across channels
    assert one(rule(VALUE, 0, 0, minus=(0, 1)))[0]["x"] == 0.5 and one(rule(VALUE, 0, 0, frame=1, minus=(1, 0)))[0]["x"] == 4.5
    # no source: x = +0, the bias alone
    st, _ = one(rule(VALUE, 0, bias=-0.125))
    assert bits(st["x"]) == [0] and st["value"] == F(-0.125) and st["status"] == ref.EVALUATED


def test_outside_and_edges_exactly_at_a_bound():
    for f, lower, upper, inside in ((2.0, 2.0, 5.0, True), (2.0, -1.0, 2.0, True), (2.0, 2.0, 2.0, True), (2.0, np.nextafter(F(2.0), INF), 5.0, False),
                                    (2.0, -1.0, np.nextafter(F(2.0), -INF), False), (2.0, -INF, INF, True)):
        assert one(rule(TEST, 0, 0, gain=1.0, bias=-1.0, lower=lower, upper=upper))[0]["value"] == (1.0 if inside else -1.0), (lower, upper)
        assert one(rule(TEST, 0, 0, gain=1.0, bias=-1.0, lower=lower, upper=upper, flags=OUTSIDE))[0]["value"] == (-1.0 if inside else 1.0)
        assert one(rule(TERMINATE, 0, 0, lower=lower, upper=upper))[0]["fired"] == int(inside)
        assert one(rule(TRUNCATE, 0, 0, lower=lower, upper=upper, flags=OUTSIDE))[0]["fired"] == int(not inside)
    # -0 is inside [+0, +0]
    assert one(rule(TERMINATE, 0, 0, lower=0.0, upper=0.0), obs=np.array([[-0.0]], dtype=F))[0]["fired"] == 1


def test_a_nan_fires_outside_and_passes_through():
    # not inside whatever the bounds: an OUTSIDE termination fires, a plain one does not
    st, out = one(rule(TERMINATE, 0, 3, gain=-1.0, flags=OUTSIDE))
    assert np.isnan(st["x"]) and st["fired"] == 1 and st["value"] == -1.0 and out["flags"][0] == ref.TERMINATED
    assert one(rule(TERMINATE, 0, 3, gain=-1.0))[0]["fired"] == 0
    assert one(rule(TEST, 0, 3, gain=1.0, bias=-1.0))[0]["value"] == -1.0
    # REWARD_VALUE: unclamped, and the agent's reward and return are NaN
    st, out = one(rule(VALUE, 0, 3, lower=-1.0, upper=1.0))
    assert st["status"] == ref.EVALUATED and np.isnan(st["value"]) and np.isnan(out["rewards"][0]) and np.isnan(out["states"]["episodeReturn"][0])
    # an infinity is clamped
    assert one(rule(VALUE, 0, 0, lower=-1.0, upper=1.0), obs=np.array([[np.inf]], dtype=F))[0]["value"] == 1.0


def test_the_sum_takes_the_list_order():
    # 1e8 + 1 - 1e8: 1 is below half an ulp of 1e8 (8), so it is lost when added first to 1e8 and kept when the big terms cancel first
    triple = [rule(VALUE, 0, bias=1e8), rule(VALUE, 0, bias=1.0), rule(VALUE, 0, bias=-1e8)]
    forward = ref.step(ref.Accounting(1), None, wire.episode_rule_list(triple), 1, None)["rewards"][0]
    backward = ref.step(ref.Accounting(1), None, wire.episode_rule_list([triple[0], triple[2], triple[1]]), 1, None)["rewards"][0]
    assert bits(forward) == bits(0.0) and bits(backward) == bits(1.0)
    # the order is the list's per agent, whatever lies between one agent's rules
    mixed = wire.episode_rule_list([triple[0], rule(VALUE, 1, bias=3.0), triple[1], rule(VALUE, 1, bias=4.0), triple[2]])
    out = ref.step(ref.Accounting(2), None, mixed, 2, None)
    assert out["rewards"].tolist() == [0.0, 7.0]
    # r starts from +0: a single -0 gives +0
    assert bits(ref.step(ref.Accounting(1), None, wire.episode_rule_list([rule(VALUE, 0, bias=-0.0)]), 1, None)["rewards"]) == [0]


def test_every_status_in_the_stated_order():
    # DISABLED before everything: a channel beyond the list, a source that is off
    for r, obs, dims in ((rule(VALUE, 0, 9, bias=1.0, flags=OFF), OBS, None), (rule(VALUE, 0, 0, bias=1.0, flags=OFF), None, (2, 4)), (rule(VALUE, 0, bias=1.0, flags=OFF), None, (0, 0))):
        st, out = one(r, obs, dims)
        assert st["status"] == ref.DISABLED and bits([st["x"], st["f"], st["value"]]) == [0, 0, 0] and bits(out["rewards"]) == [0]
    # SKIPPED: a channel at the list's channels, a frame at its frames, either of a difference's second term
    for r in (rule(VALUE, 0, 4, bias=1.0), rule(VALUE, 0, 0, frame=2, bias=1.0), rule(VALUE, 0, 0, minus=(4, 0), bias=1.0), rule(TERMINATE, 0, 0, minus=(0, 2))):
        st, out = one(r)
        assert st["status"] == ref.SKIPPED and st["fired"] == 0 and bits(out["rewards"]) == [0] and out["flags"][0] == 0
        # ... before SOURCE_OFF: the list is set and did not report
        assert one(r, None, (2, 4))[0]["status"] == ref.SKIPPED
    # SOURCE_OFF: the report did not run; no list at all (there is nothing to be beyond)
    assert one(rule(VALUE, 0, 3, bias=1.0), None, (2, 4))[0]["status"] == ref.SOURCE_OFF
    st, out = one(rule(TERMINATE, 0, 99, gain=1.0), None, (0, 0))
    assert st["status"] == ref.SOURCE_OFF and st["fired"] == 0 and out["flags"][0] == 0
    # no source is never SKIPPED or SOURCE_OFF
    for obs, dims in ((OBS, None), (None, (2, 4)), (None, (0, 0))):
        assert one(rule(TEST, 0, gain=2.0, lower=0.0, upper=0.0), obs, dims)[0]["value"] == 2.0
    # the counts
    rules = wire.episode_rule_list([rule(VALUE, 0, 0), rule(VALUE, 1, 0, flags=OFF), rule(VALUE, 1, 4), rule(VALUE, 0, 5), rule(VALUE, 1)])
    assert ref.step(ref.Accounting(2), OBS, rules, 2, None)["counts"].tolist() == [2, 1, 2, 0, 0, 0, 0, 0]
    assert ref.step(ref.Accounting(2), None, rules, 2, None, (2, 4))["counts"].tolist() == [1, 1, 2, 1, 0, 0, 0, 0]


def test_time_limit_restart_and_rebase():
    # agent 0: terminates when channel 0 >= 3, limit 3; agent 1: no rule, limit 2; agent 2: a reward of 0.25 per step, no limit
    rules = wire.episode_rule_list([rule(VALUE, 0, 0, gain=0.5), rule(TERMINATE, 0, 0, gain=10.0, lower=3.0), rule(VALUE, 2, bias=0.25), rule(TRUNCATE, 0, 0, gain=0.0, lower=3.0)])
    limits = np.array([3, 2, 0], dtype=np.int32)
    acc = ref.Accounting(3)
    seen = []
    for value in (1.0, 2.0, 3.0, 1.0, 4.0, 1.0):
        seen.append(ref.step(acc, np.array([[value]], dtype=F), rules, 3, limits))
    a0 = [(int(o["states"]["flags"][0]), int(o["states"]["rule"][0]), float(o["states"]["reward"][0]), float(o["states"]["episodeReturn"][0]),
           int(o["states"]["episodeLength"][0]), int(o["states"]["episodes"][0]), float(o["states"]["lastReturn"][0]), int(o["states"]["lastLength"][0])) for o in seen]
    # step 3: the fired rules (both bits, the first one's index) and the time limit in the same step; step 4 restarts by itself
    assert a0 == [(0, -1, 0.5, 0.5, 1, 0, 0.0, 0), (0, -1, 1.0, 1.5, 2, 0, 0.0, 0), (7, 1, 11.5, 13.0, 3, 1, 13.0, 3),
                  (0, -1, 0.5, 0.5, 1, 1, 13.0, 3), (3, 1, 12.0, 12.5, 2, 2, 12.5, 2), (0, -1, 0.5, 0.5, 1, 2, 12.5, 2)]
    assert [int(o["flags"][1]) for o in seen] == [0, 6, 0, 6, 0, 6] and [int(o["states"]["episodeLength"][1]) for o in seen] == [1, 2, 1, 2, 1, 2]
    assert [int(o["states"]["episodes"][1]) for o in seen] == [0, 1, 1, 2, 2, 3] and not any(o["rewards"][1] for o in seen)
    assert [float(o["states"]["episodeReturn"][2]) for o in seen] == [0.25 * k for k in range(1, 7)] and seen[-1]["states"]["episodes"][2] == 0
    # events: ascending by agent, the values of step 5
    assert [o["events"]["agent"].tolist() for o in seen] == [[], [1], [0], [1], [0], [1]]
    assert seen[2]["events"][0].tolist() == (0, 7, 3, 13.0) and seen[1]["events"][0].tolist() == (1, 6, 2, 0.0)
    assert [o["counts"][4:].tolist() for o in seen[:3]] == [[0, 0, 0, 0], [1, 0, 1, 1], [1, 1, 1, 1]]
    # a limit of 1 is done every step
    every = ref.Accounting(1)
    for k in range(3):
        out = ref.step(every, None, rules[:0], 1, np.array([1], dtype=np.int32))
        assert (out["flags"][0], out["states"]["episodeLength"][0], out["states"]["episodes"][0]) == (6, 1, k + 1)
    # re-base: everything to zero, the next pass fresh
    acc.rebase()
    out = ref.step(acc, np.array([[1.0]], dtype=F), rules, 3, limits)
    assert out["states"]["episodeLength"].tolist() == [1, 1, 1] and not out["states"]["episodes"].any() and not out["states"]["lastLength"].any()
    assert out["states"]["episodeReturn"].tolist() == [0.5, 0.0, 0.25]


GOOD = [rule(VALUE, 0, 3, frame=1, minus=(2, 0), shape=2, gain=0.5, bias=1.0, lower=-1.0, upper=1.0), rule(TEST, 1, gain=1.0, bias=-1.0),
        rule(TERMINATE, 2, 0, gain=5.0, flags=OUTSIDE | OFF), rule(TRUNCATE, 0, 7, lower=0.0, upper=0.0)]
# (field, index into the field or None, value, record): every validation rule of the header
BAD = [("kind", None, 0, 0), ("kind", None, 5, 0), ("shape", None, -1, 0), ("shape", None, 3, 0), ("agent", None, -1, 0), ("agent", None, 3, 0),
       ("channelA", None, -2, 0), ("channelA", None, -1, 0), ("frameA", None, -1, 0), ("channelB", None, -1, 0), ("frameB", None, -1, 0),
       ("channelB", None, 1, 1), ("frameB", None, 1, 3), ("flags", None, 8, 1), ("flags", None, -1, 1), ("reserved", 0, 1, 1), ("reserved", 3, -1, 2),
       ("gain", None, np.nan, 0), ("gain", None, np.inf, 1), ("bias", None, np.nan, 0), ("bias", None, -np.inf, 1), ("lower", None, np.nan, 0),
       ("upper", None, np.nan, 0), ("lower", None, 2.0, 0), ("upper", None, -2.0, 0), ("bias", None, 0.5, 2), ("bias", None, -1.0, 3)]


def test_validation_rules_of_the_statement():
    good = wire.episode_rule_list(GOOD)
    assert ref.valid(good, 3) == -1 and ref.valid(good, 3, [0, 5, 0]) == -1 and ref.valid(good, wire.MAX_EPISODE_AGENTS) == -1
    assert ref.valid(good, 2) == 2 and ref.valid(good, 0) == 0 and ref.valid(good, -1) == 0 and ref.valid(good, wire.MAX_EPISODE_AGENTS + 1) == 0
    assert ref.valid(good[:0], 0) == -1 and ref.valid(good[:0], 5, [0] * 5) == -1 and ref.valid(good, 3, [0, -1, 0]) == 1
    assert ref.valid(np.zeros(wire.MAX_EPISODE_RULES + 1, dtype=wire.episode_rule_dtype), 1) == 0
    for name, index, value, record in BAD:
        wrong = good.copy()
        if index is None:
            wrong[name][record] = value
        else:
            wrong[name][record][index] = value
        assert ref.valid(wrong, 3) == record, (name, index, value)
    allowed = good.copy()
    allowed["lower"], allowed["upper"] = (np.inf, -np.inf, 0.0, -np.inf), (np.inf, -np.inf, 0.0, np.inf)  # lower == upper, infinities
    allowed["channelA"][0], allowed["frameA"][0] = 2 ** 31 - 1, 2 ** 31 - 1  # whether a channel fits is the device's to judge
    assert ref.valid(allowed, 3) == -1


def test_kernels_use_no_scratch():
    """hipcc's own report for episodes.hip (make resources-episodes), through tools/kernel_resources.py: each kernel of the file is there
    once, has no private frame, spills nothing and keeps four waves per SIMD or more."""
    kernels = dict.fromkeys(("episodeRulesKernel", "episodeAgentsKernel", "episodeEventsKernel", "reportBodyRangesKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-episodes", "resources_episodes.txt", kernels, floor=4, total=4)


@hostcheck_util.needs_sanitizers
def test_episode_host_code_under_asan_and_ubsan(tmp_path):
    """Every validation refusal, with and without a world and a list, each leaving the old list, its accounting and its answers standing
    -> the list held across uploads -> the re-bases by upload, replacement and flags -> the getters' state machine per flag -> every
    getter and both exports with too-small and exact heap buffers -> destroy, for 0, 1, 65, 257 and 16,384 agents and 0, 1 and 65,536
    rules, on the sanitizer build of tests/test_hostcheck.py (kernels never run there: the program plays the kernels' writes)."""
    hostcheck_util.run_sanitized(tmp_path, "episodes_main.cpp", "EPISODES MAIN OK", timeout=600)
