// TEST INFRASTRUCTURE.  The host side of the episodes (solver2d_amd/csrc/episodes.hip: validation, the grouping of the list by agent, the
// list's device block and its replacement, the re-bases, the getters' state machine per report flag, the two exports and the tenth entry
// of report_host.cpp's table) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and
// linked against _build/libs2amd_hostcheck.so.  Kernels never run here, so this program plays their writes: after a step it fills the
// rewards and the flags with that step's number and sets the count of done agents, and then checks that every way out gives them back.
// It also reads the setter's grouped copy back and checks it against the statement's order.  Every buffer is a heap block of exactly the
// size passed.  Built and run by tests/test_episodes_host.py.
#include "report_main_common.h"

#include <cstring>

static const int ALL = S2AMD_EPISODE_REPORT_STEP | S2AMD_EPISODE_REPORT_STATES | S2AMD_EPISODE_REPORT_RULE_STATES | S2AMD_EPISODE_REPORT_EVENTS;

// `count` rules over `agents` agents, one agent's rules not adjacent, every kind, shape and flag in turn
static std::vector<s2amdEpisodeRule> makeRules(int count, int agents)
{
	std::vector<s2amdEpisodeRule> list;
	for (int k = 0; k < count; ++k)
	{
		s2amdEpisodeRule r = {};
		r.kind = 1 + k % 4;
		r.agent = agents > 0 ? (int)(((long)k * 7) % agents) : 0;
		r.channelA = k % 5 == 0 ? -1 : k % 9;
		r.frameA = k % 3;
		r.shape = k % 3;
		r.flags = (k % 11 == 10 ? S2AMD_EPISODE_RULE_DISABLED : 0) | (k % 2 == 1 ? S2AMD_EPISODE_RULE_OUTSIDE : 0);
		if (r.channelA >= 0 && k % 4 == 2)
		{
			r.flags |= S2AMD_EPISODE_RULE_DIFFERENCE;
			r.channelB = k % 7, r.frameB = 1;
		}
		r.gain = 1.5f, r.bias = r.kind >= 3 ? 0.0f : -0.25f, r.lower = k % 2 == 0 ? -INFINITY : -2.0f, r.upper = k % 3 == 0 ? INFINITY : 2.0f;
		list.push_back(r);
	}
	return list;
}

static size_t roundUp(size_t bytes)
{
	return ((bytes > 0 ? bytes : 1) + 255) & ~size_t(255);
}

// (episodes.hip: episodeLayout) where the pieces lie in the list's block
struct Block
{
	int* counts;
	s2amdEpisodeRule* rules;
	int* first;
	int* limits;
	float* rewards;
	int* flags;
};

static Block blockOf(s2amdSolver* s)
{
	const size_t rules = s->hEpisodeRules.size(), agents = (size_t)s->episodeAgents;
	char* at = (char*)s->dEpisodes.p;
	Block b;
	b.counts = (int*)at, at += roundUp(16 * sizeof(int));
	b.rules = (s2amdEpisodeRule*)at, at += roundUp(rules * sizeof(s2amdEpisodeRule));
	b.first = (int*)at, at += roundUp((agents + 1) * sizeof(int));
	b.limits = (int*)at, at += roundUp(agents * sizeof(int));
	at += roundUp(rules * sizeof(float)) + roundUp(rules * sizeof(int)) + roundUp(agents * sizeof(s2amdEpisodeState));
	b.rewards = (float*)at, at += roundUp(agents * sizeof(float));
	b.flags = (int*)at;
	return b;
}

// the grouped copy: a stable order by (agent, list index), the list index kept, first[] the runs, the limits as given
static void checkGrouped(s2amdSolver* s, const std::vector<s2amdEpisodeRule>& list, const std::vector<int32_t>& limits)
{
	const int agents = s->episodeAgents, rules = (int)list.size();
	if (agents == 0)
	{
		return;
	}
	const Block b = blockOf(s);
	int wrong = 0;
	wrong += b.first[0] != 0 || b.first[agents] != rules ? 1 : 0;
	for (int a = 0; a < agents; ++a)
	{
		wrong += b.first[a] > b.first[a + 1] ? 1 : 0;
		wrong += b.limits[a] != (limits.empty() ? 0 : limits[(size_t)a]) ? 1 : 0;
		for (int p = b.first[a]; p < b.first[a + 1]; ++p)
		{
			const s2amdEpisodeRule& g = b.rules[p];
			const int index = g.reserved[0];
			wrong += g.agent != a || index < 0 || index >= rules || (p > b.first[a] && b.rules[p - 1].reserved[0] >= index) ? 1 : 0;
			if (index >= 0 && index < rules)
			{
				s2amdEpisodeRule plain = g;
				plain.reserved[0] = 0;
				wrong += memcmp(&plain, &list[(size_t)index], sizeof(plain)) != 0 ? 1 : 0;
			}
		}
	}
	EXPECT(wrong, 0);
}

// one step with the report on and the kernels' writes played: rewards and flags = the stamp, `done` agents done
static void stepOn(s2amdSolver* s, int stamp, int done)
{
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	const long passes = s->episodePasses;
	EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
	if (s->episodeAgents == 0)
	{
		EXPECT((int)(s->episodePasses - passes), 0);
		return;
	}
	EXPECT((int)(s->episodePasses - passes), 1);
	EXPECT(s->episodeFresh ? 1 : 0, 0);
	const Block b = blockOf(s);
	for (int a = 0; a < s->episodeAgents; ++a)
	{
		b.rewards[a] = (float)stamp + 0.5f * (float)a;
		b.flags[a] = stamp + a;
	}
	int* set = b.counts + 8 * (int)((s->episodePasses - 1) & 1);
	for (int k = 0; k < 8; ++k)
	{
		set[k] = k == 4 ? done : 100 * stamp + k;
	}
}

template <typename T, typename Fn> static void ask(Fn fn, s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<T> out(capacity);
	int32_t count = -7;
	EXPECT(fn(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

// every getter with a buffer of `slack` entries fewer than it needs (0: exact), for the flags the last step ran with
static void askAll(s2amdSolver* s, int stepFlags, int slack, int done)
{
	const int agents = s->episodeAgents, rules = (int)s->hEpisodeRules.size();
	const bool none = agents == 0;
	auto want = [&](int flag, int items, int* rc, int* count) {
		const bool open = (stepFlags & flag) != 0;
		const bool empty = none || items == 0;
		*rc = empty ? S2AMD_OK : (!open ? S2AMD_E_STATE : (slack > 0 ? S2AMD_E_CAPACITY : S2AMD_OK));
		*count = empty ? 0 : (open ? items : -7);
	};
	int rc = 0, count = 0;
	want(S2AMD_EPISODE_REPORT_STEP, agents, &rc, &count);
	ask<float>(s2amd_world_episode_rewards, s, std::max(agents - slack, 0), rc, count);
	ask<int32_t>(s2amd_world_episode_flags, s, std::max(agents - slack, 0), rc, count);
	want(S2AMD_EPISODE_REPORT_STATES, agents, &rc, &count);
	ask<s2amdEpisodeState>(s2amd_world_episode_states, s, std::max(agents - slack, 0), rc, count);
	want(S2AMD_EPISODE_REPORT_RULE_STATES, rules, &rc, &count);
	ask<s2amdEpisodeRuleState>(s2amd_world_episode_rule_states, s, std::max(rules - slack, 0), rc, count);
	const int listed = std::min(done, agents);
	want(S2AMD_EPISODE_REPORT_EVENTS, listed, &rc, &count);
	if (!none && listed == 0)
	{
		rc = (stepFlags & S2AMD_EPISODE_REPORT_EVENTS) != 0 ? S2AMD_OK : S2AMD_E_STATE, count = rc ? -7 : 0;
	}
	ask<s2amdEpisodeEvent>(s2amd_world_episode_events, s, std::max(listed - slack, 0), rc, count);
	Exact<int32_t> counts(8);
	EXPECT(s2amd_world_episode_counts(s, counts.p), none || stepFlags != 0 ? S2AMD_OK : S2AMD_E_STATE);
	if (!none && stepFlags != 0)
	{
		EXPECT(counts.p[4], done);
	}
	if (none)
	{
		EXPECT(counts.p[0] | counts.p[4] | counts.p[7], 0);
	}
	// the exports
	const size_t bytes = 4u * (size_t)std::max(agents, 1);
	void *rewards = nullptr, *flags = nullptr;
	EXPECT(s2amd_device_alloc(s, bytes, &rewards), S2AMD_OK);
	EXPECT(s2amd_device_alloc(s, bytes, &flags), S2AMD_OK);
	want(S2AMD_EPISODE_REPORT_STEP, agents, &rc, &count);
	EXPECT(s2amd_world_export_episode_step(s, rewards, flags, std::max(agents - slack, 0)), rc);
	EXPECT(s2amd_world_export_episode_step_async(s, rewards, flags, std::max(agents - slack, 0), 2), rc);
	EXPECT(s2amd_world_export_episode_step_async(s, rewards, flags, agents, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_export_episode_step_async(s, rewards, flags, agents, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_export_episode_step(s, rewards, flags, -1), S2AMD_E_INVALID);
	if (agents > 0)
	{
		EXPECT(s2amd_world_export_episode_step(s, nullptr, flags, agents), S2AMD_E_INVALID);
		EXPECT(s2amd_world_export_episode_step(s, rewards, nullptr, agents), S2AMD_E_INVALID);
	}
	if (rc == S2AMD_OK && agents > 0)
	{
		EXPECT(s2amd_export_wait(s, 2), S2AMD_OK);
		Exact<float> r(agents);
		Exact<int32_t> f(agents), hf(agents);
		Exact<float> hr(agents);
		int32_t n = 0;
		EXPECT(s2amd_device_read(s, r.p, rewards, 4u * (uint64_t)agents), S2AMD_OK);
		EXPECT(s2amd_device_read(s, f.p, flags, 4u * (uint64_t)agents), S2AMD_OK);
		EXPECT(s2amd_world_episode_rewards(s, hr.p, agents, &n), S2AMD_OK);
		EXPECT(s2amd_world_episode_flags(s, hf.p, agents, &n), S2AMD_OK);
		const Block b = blockOf(s);
		EXPECT(memcmp(r.p, b.rewards, 4u * (size_t)agents) | memcmp(f.p, b.flags, 4u * (size_t)agents), 0);
		EXPECT(memcmp(hr.p, b.rewards, 4u * (size_t)agents) | memcmp(hf.p, b.flags, 4u * (size_t)agents), 0);
	}
	EXPECT(s2amd_device_free(s, rewards), S2AMD_OK);
	EXPECT(s2amd_device_free(s, flags), S2AMD_OK);
	// bad arguments
	int32_t n = -7;
	float one = 0.0f;
	EXPECT(s2amd_world_episode_rewards(s, &one, -1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_episode_rewards(s, nullptr, 1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_episode_rewards(s, &one, 1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_episode_events(s, nullptr, 1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_episode_events(nullptr, nullptr, 0, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_episode_counts(s, nullptr), S2AMD_E_INVALID);
}

// every refusal; the old list and its accounting stand
static void refusals(s2amdSolver* s)
{
	const std::vector<s2amdEpisodeRule> list = makeRules(12, 5);
	const std::vector<int32_t> limits = {0, 3, 0, 1, 7};
	const size_t held = s->hEpisodeRules.size();
	const int heldAgents = s->episodeAgents, heldStepFlags = s->episodeReport.stepFlags;
	const bool heldFresh = s->episodeFresh;
	const long heldPasses = s->episodePasses;
	EXPECT(s2amd_world_set_episodes(s, list.data(), -1, 5, limits.data()), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, nullptr, 3, 5, limits.data()), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(nullptr, list.data(), 3, 5, limits.data()), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, list.data(), 12, 0, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, list.data(), 12, -1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, nullptr, 0, -1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, nullptr, 0, S2AMD_MAX_EPISODE_AGENTS + 1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, list.data(), 12, 4, nullptr), S2AMD_E_INVALID); // an agent beyond the agents
	const std::vector<s2amdEpisodeRule> many((size_t)S2AMD_MAX_EPISODE_RULES + 1, list[1]);
	EXPECT(s2amd_world_set_episodes(s, many.data(), S2AMD_MAX_EPISODE_RULES + 1, 5, nullptr), S2AMD_E_INVALID);
	const std::vector<int32_t> negative = {0, 3, -1, 1, 7};
	EXPECT(s2amd_world_set_episodes(s, list.data(), 12, 5, negative.data()), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episodes(s, nullptr, 0, 5, negative.data()), S2AMD_E_INVALID);
	for (int bad = 0; bad < 24; ++bad)
	{
		std::vector<s2amdEpisodeRule> wrong = list;
		// list[1]: REWARD_TEST, plain; list[2]: TERMINATE with DIFFERENCE; list[3]: TRUNCATE, plain
		s2amdEpisodeRule &plain = wrong[1], &diff = wrong[2], &ending = wrong[3];
		switch (bad)
		{
		case 0: plain.kind = 0; break;
		case 1: plain.kind = 5; break;
		case 2: plain.shape = -1; break;
		case 3: plain.shape = 3; break;
		case 4: plain.agent = -1; break;
		case 5: plain.agent = 5; break;
		case 6: plain.channelA = -2; break;
		case 7: plain.frameA = -1; break;
		case 8: plain.channelB = 1; break;
		case 9: plain.frameB = 1; break;
		case 10: diff.channelB = -1; break;
		case 11: diff.frameB = -1; break;
		case 12: diff.channelA = -1; break;
		case 13: plain.flags = 8; break;
		case 14: plain.flags = -1; break;
		case 15: plain.reserved[0] = 1; break;
		case 16: plain.reserved[3] = -1; break;
		case 17: plain.gain = NAN; break;
		case 18: plain.bias = INFINITY; break;
		case 19: plain.lower = NAN; break;
		case 20: plain.upper = NAN; break;
		case 21: plain.lower = 3.0f, plain.upper = 2.0f; break;
		case 22: ending.bias = 0.5f; break;
		default: diff.bias = -1.0f; break;
		}
		EXPECT(s2amd_world_set_episodes(s, wrong.data(), (int32_t)wrong.size(), 5, limits.data()), S2AMD_E_INVALID);
	}
	EXPECT(s2amd_world_set_episode_report(s, 16), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_episode_report(nullptr, 1), S2AMD_E_INVALID);
	EXPECT((int)s->hEpisodeRules.size(), (int)held);
	EXPECT(s->episodeAgents, heldAgents);
	EXPECT(s->episodeFresh ? 1 : 0, heldFresh ? 1 : 0);
	EXPECT((int)s->episodePasses, (int)heldPasses);
	EXPECT(s->episodeReport.stepFlags, heldStepFlags);
}

static void drive(const World& first, const World& second, int agents, int rules)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	// no list, no world
	refusals(s);
	askAll(s, 0, 0, 0);
	// a list before any world, the report on before any world
	const std::vector<s2amdEpisodeRule> list = makeRules(rules, agents);
	std::vector<int32_t> limits;
	for (int a = 0; a < agents; ++a)
	{
		limits.push_back(a % 4);
	}
	EXPECT(s2amd_world_set_episodes(s, rules > 0 ? list.data() : nullptr, rules, agents, agents > 0 ? limits.data() : nullptr), S2AMD_OK);
	checkGrouped(s, list, limits);
	EXPECT(s2amd_world_set_episode_report(s, ALL), S2AMD_OK);
	askAll(s, 0, 0, 0);
	int stamp = 1;
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		EXPECT(upload(s, *worlds[pass]), S2AMD_OK);
		EXPECT((int)s->hEpisodeRules.size(), rules); // the list holds across uploads
		EXPECT(s->episodeAgents, agents);
		EXPECT(s->episodeFresh ? 1 : 0, 1); // ... and the accounting is re-based
		checkGrouped(s, list, limits);
		refusals(s);
		askAll(s, 0, 0, 0); // no step since the upload
		for (int step = 0; step < 3; ++step)
		{
			const int done = step == 0 ? 0 : (step == 1 ? std::min(agents, 3) : agents);
			stepOn(s, stamp++, done);
			askAll(s, ALL, 0, done);
			askAll(s, ALL, 1, done);
		}
		refusals(s);
		askAll(s, ALL, 0, agents); // a refused list leaves the answers in place
		// a step with the flags at 0 is none: nothing is counted, the getters refuse, and turning them on again re-bases
		const long passes = s->episodePasses;
		EXPECT(s2amd_world_set_episode_report(s, 0), S2AMD_OK);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		EXPECT((int)(s->episodePasses - passes), 0);
		EXPECT(s->episodeFresh ? 1 : 0, agents > 0 ? 0 : 1);
		askAll(s, 0, 0, 0);
		// each flag alone opens its own getters
		const int each[4] = {S2AMD_EPISODE_REPORT_STEP, S2AMD_EPISODE_REPORT_STATES, S2AMD_EPISODE_REPORT_RULE_STATES, S2AMD_EPISODE_REPORT_EVENTS};
		for (int flag : each)
		{
			EXPECT(s2amd_world_set_episode_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_episode_report(s, flag), S2AMD_OK);
			EXPECT(s->episodeFresh ? 1 : 0, 1);
			stepOn(s, stamp++, std::min(agents, 2));
			askAll(s, flag, 0, std::min(agents, 2));
		}
		EXPECT(s2amd_world_set_episode_report(s, ALL), S2AMD_OK); // (non-zero to non-zero: no re-base)
		EXPECT(s->episodeFresh ? 1 : 0, agents > 0 ? 0 : 1);
		// replaced: re-based, the getters refuse until a step, and the new sizes hold
		const int fewerAgents = agents > 1 ? agents / 2 : agents, fewerRules = rules > 1 ? rules / 3 : rules;
		const std::vector<s2amdEpisodeRule> other = makeRules(fewerRules, fewerAgents);
		EXPECT(s2amd_world_set_episodes(s, fewerRules > 0 ? other.data() : nullptr, fewerRules, fewerAgents, nullptr), S2AMD_OK);
		EXPECT(s->episodeFresh ? 1 : 0, 1);
		EXPECT((int)s->episodePasses, 0);
		checkGrouped(s, other, std::vector<int32_t>());
		askAll(s, 0, 0, 0);
		stepOn(s, stamp++, fewerAgents);
		askAll(s, ALL, 0, fewerAgents);
		// cleared: count 0 at once
		EXPECT(s2amd_world_set_episodes(s, nullptr, 0, 0, nullptr), S2AMD_OK);
		askAll(s, 0, 0, 0);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		askAll(s, ALL, 0, 0);
		// the first list again, for the next upload
		EXPECT(s2amd_world_set_episodes(s, rules > 0 ? list.data() : nullptr, rules, agents, agents > 0 ? limits.data() : nullptr), S2AMD_OK);
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0), small = makeWorld(40), big = makeWorld(300);
	const int sizes[8][2] = {{0, 0}, {1, 0}, {1, 1}, {65, 1}, {65, 300}, {257, 1000}, {1, S2AMD_MAX_EPISODE_RULES}, {S2AMD_MAX_EPISODE_AGENTS, S2AMD_MAX_EPISODE_RULES}};
	for (const int* size : sizes)
	{
		drive(small, big, size[0], size[1]);
		if (size[1] <= 1000)
		{
			drive(none, small, size[0], size[1]);
		}
	}
	drive(big, none, S2AMD_MAX_EPISODE_AGENTS, 0);
	if (failures == 0)
	{
		printf("EPISODES MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
