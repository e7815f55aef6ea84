"""The statement of the episodes (include/solver2d_amd.h: s2amd_world_set_episodes, s2amd_world_set_episode_report,
s2amd_world_episode_rewards, s2amd_world_episode_flags, s2amd_world_episode_states, s2amd_world_episode_rule_states,
s2amd_world_episode_events, s2amd_world_episode_counts), restated in numpy for the tests.  Test infrastructure only.

A rule reads the observation array of this step, float32[frames][channels] newest first (what s2amd_world_observations answers), or
None when the observation report did not run; `dims` = (frames, channels) of the observer list whether or not it reported, (0, 0) with no
list.  Every product, sum and difference is a float32 scalar rounded on its own; an agent's reward is the float32 sum of its rules'
values in list order, starting from +0."""
import numpy as np

from solver2d_amd import wire
from tests import actuator_ref

F = np.float32
EVALUATED, DISABLED, SKIPPED, SOURCE_OFF = 0, 1, 2, 3
REWARD_VALUE, REWARD_TEST, TERMINATE, TRUNCATE = 1, 2, 3, 4
LINEAR, ABS, SQUARE = 0, 1, 2
TERMINATED, TRUNCATED, TIME_LIMIT = 1, 2, 4


def valid(rules, agents, step_limits=None):
    """What the host checks before anything is replaced: -1, or the index of the first invalid record (0 for the call's own arguments,
    a step limit's index for a negative limit)."""
    if not 0 <= agents <= wire.MAX_EPISODE_AGENTS or len(rules) > wire.MAX_EPISODE_RULES or (len(rules) and agents == 0):
        return 0
    for i, r in enumerate(rules):
        flags = int(r["flags"])
        if not 1 <= r["kind"] <= 4 or not 0 <= r["shape"] <= 2 or not 0 <= r["agent"] < agents or r["channelA"] < -1 or r["frameA"] < 0:
            return i
        if flags & ~(wire.EPISODE_RULE_DISABLED | wire.EPISODE_RULE_DIFFERENCE | wire.EPISODE_RULE_OUTSIDE) or r["reserved"].any():
            return i
        if flags & wire.EPISODE_RULE_DIFFERENCE:
            if r["channelA"] < 0 or r["channelB"] < 0 or r["frameB"] < 0:
                return i
        elif r["channelB"] != 0 or r["frameB"] != 0:
            return i
        if not np.isfinite(r["gain"]) or not np.isfinite(r["bias"]) or not r["lower"] <= r["upper"]:
            return i
        if r["kind"] >= TERMINATE and r["bias"] != 0:
            return i
    if step_limits is not None:
        for i, limit in enumerate(step_limits):
            if limit < 0:
                return i
    return -1


def rule_value(obs, r, dims):
    """-> (status, x, f, y, fired) of one rule"""
    zero = F(0.0)
    flags, kind, shape = int(r["flags"]), int(r["kind"]), int(r["shape"])
    frames, channels = dims
    reads, difference = r["channelA"] >= 0, bool(flags & wire.EPISODE_RULE_DIFFERENCE)
    if flags & wire.EPISODE_RULE_DISABLED:
        return DISABLED, zero, zero, zero, 0
    if reads and channels > 0 and (r["channelA"] >= channels or r["frameA"] >= frames or (difference and (r["channelB"] >= channels or r["frameB"] >= frames))):
        return SKIPPED, zero, zero, zero, 0
    if reads and (obs is None or channels == 0):
        return SOURCE_OFF, zero, zero, zero, 0
    with np.errstate(all="ignore"):
        x = zero
        if reads:
            x = F(obs[int(r["frameA"])][int(r["channelA"])])
            if difference:
                x = F(x - F(obs[int(r["frameB"])][int(r["channelB"])]))
        f = F(np.abs(x)) if shape == ABS else (F(x * x) if shape == SQUARE else x)
        lower, upper, gain, bias = F(r["lower"]), F(r["upper"]), F(r["gain"]), F(r["bias"])
        inside = bool(lower <= f and f <= upper)
        test = inside != bool(flags & wire.EPISODE_RULE_OUTSIDE)
    if kind == REWARD_VALUE:
        return EVALUATED, x, f, actuator_ref.command(f, gain, bias, lower, upper), 0
    if kind == REWARD_TEST:
        return EVALUATED, x, f, gain if test else bias, 0
    return EVALUATED, x, f, gain if test else zero, int(test)


def evaluate(obs, rules, agents, step_limits, lengths, dims=None):
    """Steps 2 and 3 of the statement.  lengths: int32[agents], the episode lengths after step 1 (Accounting.lengths()).
    -> (rewards float32[agents], flags int32[agents], rule states wire.episode_rule_state_dtype[len(rules)], counts int32[8])"""
    if dims is None:
        dims = (0, 0) if obs is None else tuple(np.shape(obs))
    rewards, flags = np.zeros(agents, dtype=F), np.zeros(agents, dtype=np.int32)
    states = np.zeros(len(rules), dtype=wire.episode_rule_state_dtype)
    counts = np.zeros(8, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i, r in enumerate(rules):
            status, x, f, y, fired = rule_value(obs, r, dims)
            states[i] = (i, status, x, f, y, fired, (0, 0))
            counts[status] += 1
            if status == EVALUATED:
                a = int(r["agent"])
                rewards[a] = F(rewards[a] + y)
                if fired:
                    flags[a] |= TERMINATED if r["kind"] == TERMINATE else TRUNCATED
    for a in range(agents):
        limit = 0 if step_limits is None else int(step_limits[a])
        if limit > 0 and int(lengths[a]) + 1 >= limit:
            flags[a] |= TRUNCATED | TIME_LIMIT
    counts[4:] = [np.count_nonzero(flags & 3), np.count_nonzero(flags & TERMINATED), np.count_nonzero(flags & TRUNCATED), np.count_nonzero(flags & TIME_LIMIT)]
    return rewards, flags, states, counts


class Accounting:
    """Steps 1, 4 and 5: the agent records over the reporting steps.  rebase(): an upload, a new rule list, the flags from 0 to non-zero."""

    def __init__(self, agents):
        self.states = np.zeros(agents, dtype=wire.episode_state_dtype)
        self.fresh = True

    def rebase(self):
        self.states[:] = np.zeros(1, dtype=wire.episode_state_dtype)[0]
        self.fresh = True

    def lengths(self):
        """The episode lengths after step 1, which the time limit of this step is judged on"""
        restart = np.ones(len(self.states), dtype=bool) if self.fresh else (self.states["flags"] & 3) != 0
        return np.where(restart, 0, self.states["episodeLength"]).astype(np.int32)

    def push(self, rewards, flags, rules, rule_states):
        """One reporting step -> (agent states, events), copies"""
        st = self.states
        restart = np.ones(len(st), dtype=bool) if self.fresh else (st["flags"] & 3) != 0
        st["episodeLength"][restart] = 0
        st["episodeReturn"][restart] = 0.0
        st["rule"] = -1
        for i in np.flatnonzero(rule_states["fired"])[::-1]:
            st["rule"][int(rules["agent"][i])] = i
        st["episodeLength"] += 1
        with np.errstate(all="ignore"):
            st["episodeReturn"] = (st["episodeReturn"] + np.asarray(rewards, dtype=F)).astype(F)
        st["reward"], st["flags"] = rewards, flags
        done = (st["flags"] & 3) != 0
        st["episodes"][done] += 1
        st["lastReturn"][done], st["lastLength"][done] = st["episodeReturn"][done], st["episodeLength"][done]
        self.fresh = False
        events = np.zeros(int(done.sum()), dtype=wire.episode_event_dtype)
        events["agent"] = np.flatnonzero(done)
        events["flags"], events["episodeLength"], events["episodeReturn"] = st["flags"][done], st["episodeLength"][done], st["episodeReturn"][done]
        return st.copy(), events


def step(accounting, obs, rules, agents, step_limits, dims=None):
    """One reporting step of the whole statement -> dict(rewards, flags, rule_states, counts, states, events)"""
    rewards, flags, rule_states, counts = evaluate(obs, rules, agents, step_limits, accounting.lengths(), dims)
    states, events = accounting.push(rewards, flags, rules, rule_states)
    return dict(rewards=rewards, flags=flags, rule_states=rule_states, counts=counts, states=states, events=events)
