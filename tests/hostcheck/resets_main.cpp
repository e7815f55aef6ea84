// TEST INFRASTRUCTURE.  The host side of the resets (solver2d_amd/csrc/resets.hip: validation, the lists' device block and its
// replacement, the mutual refusals with device trees and a refit order, the getters' state machine, the one-shot call's stage, the stale
// flags an enqueued pass clears and the eleventh entry of report_host.cpp's table) on the stand-in HIP runtime of tests/hostcheck, as a
// stand-alone program compiled with ASan + UBSan and linked against _build/libs2amd_hostcheck.so.  Kernels never run here, so this
// program plays their writes: after a pass it fills the counts and the agent records of the set the pass wrote, and then checks that
// the getters give them back.  Every buffer is a heap block of exactly the size passed.  Built and run by tests/test_resets_host.py.
#include "report_main_common.h"

#include <cstring>

static const int BOTH = S2AMD_RESET_ON_EPISODE_END | S2AMD_RESET_REPORT_STATES;
static const s2amdStepParams PARAMS = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};

// `count` body records on slots 1, 2, ... and count / 2 joint records, over `agents` agents
static void makeLists(int count, int agents, std::vector<s2amdResetBody>& bodies, std::vector<s2amdResetJoint>& joints)
{
	bodies.clear(), joints.clear();
	for (int k = 0; k < count; ++k)
	{
		s2amdResetBody r = {};
		r.agent = agents > 0 ? k % agents : 0;
		r.body = 1 + k;
		r.flags = k % 9 == 8 ? S2AMD_RESET_DISABLED : 0;
		r.position[0] = 0.5f * (float)k, r.position[1] = 2.0f;
		r.rot[0] = 0.0f, r.rot[1] = 1.0f;
		r.linearVelocity[0] = -0.0f;
		r.positionJitter[0] = k % 2 == 0 ? 0.25f : 0.0f;
		r.angularJitter = 0.5f;
		bodies.push_back(r);
	}
	for (int k = 0; k < count / 2; ++k)
	{
		s2amdResetJoint r = {};
		r.agent = agents > 0 ? k % agents : 0;
		r.joint = k;
		r.flags = k % 2 == 0 ? S2AMD_RESET_JOINT_SETTINGS : 0;
		r.enableMotor = 1, r.motorSpeed = 0.5f, r.targetA[0] = 1.0f;
		joints.push_back(r);
	}
}

static size_t roundUp(size_t bytes)
{
	return ((bytes > 0 ? bytes : 1) + 255) & ~size_t(255);
}

// (resets.hip: resetLayout) where the pieces lie in the list's block
struct Block
{
	int* counts;
	s2amdResetBody* bodies;
	s2amdResetJoint* joints;
	s2amdResetState* states;
	int* trigger;
};

static Block blockOf(s2amdSolver* s)
{
	const size_t agents = (size_t)s->resetAgents;
	char* at = (char*)s->dResets.p;
	Block b;
	b.counts = (int*)at, at += roundUp(16 * sizeof(int));
	b.bodies = (s2amdResetBody*)at, at += roundUp(s->hResetBodies.size() * sizeof(s2amdResetBody));
	b.joints = (s2amdResetJoint*)at, at += roundUp(s->hResetJoints.size() * sizeof(s2amdResetJoint));
	b.states = (s2amdResetState*)at, at += roundUp(2 * agents * sizeof(s2amdResetState));
	b.trigger = (int*)at;
	return b;
}

static int set(s2amdSolver* s, const std::vector<s2amdResetBody>& bodies, const std::vector<s2amdResetJoint>& joints, int agents, uint32_t seed = 7u)
{
	return s2amd_world_set_resets(s, bodies.empty() ? nullptr : bodies.data(), (int32_t)bodies.size(), joints.empty() ? nullptr : joints.data(), (int32_t)joints.size(), agents,
								  seed);
}

// the device copy is the caller's list, in list order, and the counters are zero
static void checkBlock(s2amdSolver* s, const std::vector<s2amdResetBody>& bodies, const std::vector<s2amdResetJoint>& joints)
{
	if (s->resetAgents == 0)
	{
		return;
	}
	const Block b = blockOf(s);
	EXPECT(bodies.empty() ? 0 : memcmp(b.bodies, bodies.data(), bodies.size() * sizeof(s2amdResetBody)), 0);
	EXPECT(joints.empty() ? 0 : memcmp(b.joints, joints.data(), joints.size() * sizeof(s2amdResetJoint)), 0);
	int nonzero = 0;
	for (int k = 0; k < 16; ++k)
	{
		nonzero += b.counts[k] != 0 ? 1 : 0;
	}
	for (int a = 0; a < 2 * s->resetAgents; ++a)
	{
		nonzero += b.states[a].resets != 0 || b.states[a].triggered != 0 ? 1 : 0;
	}
	EXPECT(nonzero, 0);
	EXPECT((int)s->resetPasses, 0);
	EXPECT(s->resetCountsKnown ? 1 : 0, 0);
}

// the kernels' writes of the pass that was just enqueued: counts {stamp + k}, every agent's record {stamp, 1}
static void playPass(s2amdSolver* s, int stamp)
{
	const Block b = blockOf(s);
	int* setNow = b.counts + 8 * (int)((s->resetPasses - 1) & 1);
	for (int k = 0; k < 8; ++k)
	{
		setNow[k] = stamp + k;
	}
	s2amdResetState* written = b.states + (size_t)s->resetAgents * (size_t)(s->resetPasses & 1);
	for (int a = 0; a < s->resetAgents; ++a)
	{
		written[a].resets = stamp + a, written[a].triggered = 1;
	}
}

// the getters after a pass that was played with `stamp` (stamp < 0: no pass known; sourceOff: the counts say so)
static void askAll(s2amdSolver* s, bool statesOpen, int stamp, bool sourceOff)
{
	const int agents = s->resetAgents;
	for (int slack = 0; slack < 2; ++slack)
	{
		const int capacity = std::max(agents - slack, 0);
		Exact<s2amdResetState> out(capacity);
		int32_t count = -7;
		const int want = agents == 0 ? S2AMD_OK : (!statesOpen ? S2AMD_E_STATE : (slack > 0 ? S2AMD_E_CAPACITY : S2AMD_OK));
		EXPECT(s2amd_world_reset_states(s, out.p, capacity, &count), want);
		EXPECT(count, agents == 0 ? 0 : (statesOpen ? agents : -7));
		if (want == S2AMD_OK && agents > 0 && stamp >= 0 && !sourceOff)
		{
			EXPECT(out.p[agents - 1].resets, stamp + agents - 1);
			EXPECT(out.p[0].triggered, 1);
		}
	}
	Exact<int32_t> counts(8);
	const bool known = stamp >= 0 || sourceOff;
	EXPECT(s2amd_world_reset_counts(s, counts.p), agents == 0 || known ? S2AMD_OK : S2AMD_E_STATE);
	if (agents > 0 && known)
	{
		EXPECT(counts.p[0], sourceOff ? 0 : stamp);
		EXPECT(counts.p[6], sourceOff ? 0 : stamp + 6);
		EXPECT(counts.p[7], sourceOff ? 1 : stamp + 7);
	}
	if (agents == 0)
	{
		EXPECT(counts.p[0] | counts.p[1] | counts.p[7], 0);
	}
	int32_t n = -7;
	s2amdResetState one;
	EXPECT(s2amd_world_reset_states(s, &one, -1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_states(s, nullptr, 1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_states(s, &one, 1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_states(nullptr, &one, 1, &n), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_counts(s, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_counts(nullptr, counts.p), S2AMD_E_INVALID);
}

// every refusal of the setters, one case per rule; the old list, its counters and its answers stand
static void refusals(s2amdSolver* s)
{
	std::vector<s2amdResetBody> bodies;
	std::vector<s2amdResetJoint> joints;
	makeLists(12, 5, bodies, joints);
	const size_t heldBodies = s->hResetBodies.size(), heldJoints = s->hResetJoints.size();
	const int heldAgents = s->resetAgents, heldStepFlags = s->resetReport.stepFlags;
	const long heldPasses = s->resetPasses;
	const uint32_t heldSeed = s->resetSeed;
	const bool heldKnown = s->resetCountsKnown;
	EXPECT(s2amd_world_set_resets(nullptr, bodies.data(), 12, joints.data(), 6, 5, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, bodies.data(), -1, joints.data(), 6, 5, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, bodies.data(), 12, joints.data(), -1, 5, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, nullptr, 12, joints.data(), 6, 5, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, bodies.data(), 12, nullptr, 6, 5, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, bodies.data(), 12, joints.data(), 6, 0, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, nullptr, 0, joints.data(), 6, 0, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, nullptr, 0, nullptr, 0, -1, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, nullptr, 0, nullptr, 0, S2AMD_MAX_RESET_AGENTS + 1, 1u), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_resets(s, bodies.data(), 12, joints.data(), 6, 4, 1u), S2AMD_E_INVALID); // an agent beyond the agents
	{
		const std::vector<s2amdResetBody> many((size_t)S2AMD_MAX_RESET_BODIES + 1, bodies[0]);
		EXPECT(s2amd_world_set_resets(s, many.data(), S2AMD_MAX_RESET_BODIES + 1, nullptr, 0, 5, 1u), S2AMD_E_INVALID);
		const std::vector<s2amdResetJoint> manyJoints((size_t)S2AMD_MAX_RESET_JOINTS + 1, joints[0]);
		EXPECT(s2amd_world_set_resets(s, nullptr, 0, manyJoints.data(), S2AMD_MAX_RESET_JOINTS + 1, 5, 1u), S2AMD_E_INVALID);
	}
	for (int bad = 0; bad < 27; ++bad)
	{
		std::vector<s2amdResetBody> wb = bodies;
		std::vector<s2amdResetJoint> wj = joints;
		s2amdResetBody& b = wb[3];
		s2amdResetJoint& j = wj[2];
		switch (bad)
		{
		case 0: b.agent = -1; break;
		case 1: b.agent = 5; break;
		case 2: b.body = -1; break;
		case 3: b.flags = S2AMD_RESET_JOINT_SETTINGS; break; // a joint record's
		case 4: b.flags = 4; break;
		case 5: b.flags = -1; break;
		case 6: b.reserved = 1; break;
		case 7: b.position[1] = NAN; break;
		case 8: b.rot[0] = INFINITY; break;
		case 9: b.linearVelocity[0] = -INFINITY; break;
		case 10: b.angularVelocity = NAN; break;
		case 11: b.positionJitter[0] = NAN; break;
		case 12: b.positionJitter[1] = -0.5f; break;
		case 13: b.velocityJitter[0] = -1.0f; break;
		case 14: b.velocityJitter[1] = INFINITY; break;
		case 15: b.angularJitter = -0.25f; break;
		case 16: b.angularJitter = NAN; break;
		case 17: b.body = wb[7].body; break; // a body slot named twice
		case 18: b.body = wb[8].body; break; // ... by a DISABLED record too
		case 19: j.agent = -1; break;
		case 20: j.agent = 5; break;
		case 21: j.joint = -1; break;
		case 22: j.flags = 4; break;
		case 23: j.motorSpeed = NAN; break;
		case 24: j.targetA[1] = INFINITY; break;
		case 25: j.joint = wj[5].joint; break; // a joint slot named twice
		default: wb[0].reserved = -1; break;
		}
		EXPECT(set(s, wb, wj, 5), S2AMD_E_INVALID);
	}
	EXPECT(s2amd_world_set_reset_report(s, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_reset_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_reset_report(nullptr, 1), S2AMD_E_INVALID);
	int32_t who[2] = {0, 0};
	EXPECT(s2amd_world_reset_agents(nullptr, who, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_agents(s, nullptr, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_agents(s, who, -1), S2AMD_E_INVALID); // (S2AMD_RESET_ALL goes with NULL)
	EXPECT(s2amd_world_reset_agents(s, who, -2), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_agents(s, nullptr, -2), S2AMD_E_INVALID);
	EXPECT(s2amd_world_reset_agents(s, who, S2AMD_MAX_RESET_AGENTS + 1), S2AMD_E_INVALID);
	if (s->worldResident && s->resetAgents > 0)
	{
		who[1] = s->resetAgents;
		EXPECT(s2amd_world_reset_agents(s, who, 2), S2AMD_E_INVALID);
		who[1] = -1;
		EXPECT(s2amd_world_reset_agents(s, who, 2), S2AMD_E_INVALID);
	}
	else
	{
		EXPECT(s2amd_world_reset_agents(s, who, 1), S2AMD_E_STATE); // no resident world, or no list
		EXPECT(s2amd_world_reset_agents(s, nullptr, S2AMD_RESET_ALL), S2AMD_E_STATE);
	}
	EXPECT((int)s->hResetBodies.size(), (int)heldBodies);
	EXPECT((int)s->hResetJoints.size(), (int)heldJoints);
	EXPECT(s->resetAgents, heldAgents);
	EXPECT((int)s->resetPasses, (int)heldPasses);
	EXPECT((int)s->resetSeed, (int)heldSeed);
	EXPECT(s->resetCountsKnown ? 1 : 0, heldKnown ? 1 : 0);
	EXPECT(s->resetReport.stepFlags, heldStepFlags);
}

// an enqueued pass leaves none of the three caches standing
static void staleFlagsSet(s2amdSolver* s)
{
	s->pairCacheValid = true, s->slotBytesFresh = true, s->stepBackValid = true;
}
static void expectStaleFlags(s2amdSolver* s, int standing)
{
	EXPECT((s->pairCacheValid ? 1 : 0) + (s->slotBytesFresh ? 1 : 0) + (s->stepBackValid ? 1 : 0), standing);
	s->pairCacheValid = false, s->slotBytesFresh = false, s->stepBackValid = false;
}

static std::vector<int32_t> refitOrderOf(const World& w)
{
	std::vector<int32_t> order;
	for (size_t k = 0; k < w.shapes.size(); ++k)
	{
		if (w.shapes[k].type != S2AMD_SHAPE_FREE && w.shapes[k].body > 0)
		{
			order.push_back((int32_t)k);
		}
	}
	return order;
}

static void drive(const World& first, const World& second, int agents, int records)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdWorldStepInfo info;
	// no list, no world
	refusals(s);
	askAll(s, false, -1, false);
	// a list before any world, the flags on before any world
	std::vector<s2amdResetBody> bodies;
	std::vector<s2amdResetJoint> joints;
	makeLists(records, agents, bodies, joints);
	EXPECT(set(s, bodies, joints, agents), S2AMD_OK);
	checkBlock(s, bodies, joints);
	EXPECT(s2amd_world_set_reset_report(s, BOTH), S2AMD_OK);
	askAll(s, false, -1, false);
	refusals(s);
	int stamp = 10;
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World& w = *worlds[pass];
		EXPECT(upload(s, w), S2AMD_OK);
		EXPECT((int)s->hResetBodies.size(), (int)bodies.size()); // the list holds across uploads
		EXPECT(s->resetAgents, agents);
		checkBlock(s, bodies, joints); // ... and the counters are zero again
		if (agents > 0 && !w.bodies.empty())
		{
			EXPECT(s->dResetMark.bytes >= w.bodies.size() ? 1 : 0, 1);
		}
		refusals(s);
		askAll(s, false, -1, false); // no pass since the upload

		// a step with the flags on and no episode list: the source is off, nothing is enqueued, nothing goes stale
		long passes = s->resetPasses;
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		staleFlagsSet(s);
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		EXPECT((int)(s->resetPasses - passes), 0);
		askAll(s, true, -1, agents > 0);

		// with an episode list that reports: one pass per step, the three caches cleared by it
		const int32_t limits[2] = {1, 3};
		EXPECT(s2amd_world_set_episodes(s, nullptr, 0, 2, limits), S2AMD_OK);
		EXPECT(s2amd_world_set_episode_report(s, S2AMD_EPISODE_REPORT_STEP), S2AMD_OK);
		for (int step = 0; step < 3; ++step)
		{
			passes = s->resetPasses;
			EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
			EXPECT((int)(s->resetPasses - passes), agents > 0 ? 1 : 0);
			expectStaleFlags(s, 0);
			if (agents > 0)
			{
				playPass(s, ++stamp);
				askAll(s, true, stamp, false);
			}
		}
		// the episode report off again: source off at the next step, and the caches of that step stand
		EXPECT(s2amd_world_set_episode_report(s, 0), S2AMD_OK);
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		askAll(s, true, -1, agents > 0);
		EXPECT(s2amd_world_set_episodes(s, nullptr, 0, 0, nullptr), S2AMD_OK);

		// each flag alone: ON_EPISODE_END keeps the states getter shut, REPORT_STATES alone runs no pass and opens it
		EXPECT(s2amd_world_set_reset_report(s, S2AMD_RESET_ON_EPISODE_END), S2AMD_OK);
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		askAll(s, false, -1, agents > 0);
		EXPECT(s2amd_world_set_reset_report(s, S2AMD_RESET_REPORT_STATES), S2AMD_OK);
		passes = s->resetPasses;
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		EXPECT((int)(s->resetPasses - passes), 0);
		askAll(s, true, -1, agents > 0);

		// the flags at 0: a step enqueues nothing and every caller's cache stands; the one-shot call is a pass all the same
		EXPECT(s2amd_world_set_reset_report(s, 0), S2AMD_OK);
		staleFlagsSet(s);
		passes = s->resetPasses;
		EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
		EXPECT((int)(s->resetPasses - passes), 0);
		EXPECT(s->resetReport.stepFlags, 0);
		if (agents > 0)
		{
			staleFlagsSet(s);
			EXPECT(s2amd_world_reset_agents(s, nullptr, 0), S2AMD_OK); // nobody: nothing is enqueued
			expectStaleFlags(s, 3);
			staleFlagsSet(s);
			EXPECT(s2amd_world_reset_agents(s, nullptr, S2AMD_RESET_ALL), S2AMD_OK);
			expectStaleFlags(s, 0);
			playPass(s, ++stamp);
			askAll(s, false, stamp, false);
			// listed agents, twice in a row (the second call waits for the first one's staged copy), one agent named twice
			std::vector<int32_t> who = {agents - 1, 0, agents - 1};
			EXPECT(s2amd_world_set_reset_report(s, S2AMD_RESET_REPORT_STATES), S2AMD_OK);
			staleFlagsSet(s);
			EXPECT(s2amd_world_reset_agents(s, who.data(), 3), S2AMD_OK);
			expectStaleFlags(s, 0);
			EXPECT(blockOf(s).trigger[agents - 1], 1);
			EXPECT(blockOf(s).trigger[0], 1);
			EXPECT(agents > 2 ? blockOf(s).trigger[1] : 0, 0);
			EXPECT(s2amd_world_reset_agents(s, who.data() + 1, 1), S2AMD_OK);
			EXPECT(agents > 1 ? blockOf(s).trigger[agents - 1] : 0, 0);
			playPass(s, ++stamp);
			askAll(s, true, stamp, false);
			EXPECT((int)(s->resetPasses - passes), 3);
		}

		// the mutual refusals: while a list is set, no trees and no refit order; while either is set, no list
		const std::vector<int32_t> order = refitOrderOf(w);
		if (agents > 0)
		{
			EXPECT(s2amd_world_set_tree(s, 0, nullptr, 0, -1), S2AMD_E_STATE);
			if (!order.empty())
			{
				EXPECT(s2amd_world_set_refit_order(s, order.data(), (int32_t)order.size()), S2AMD_E_STATE);
			}
			EXPECT(s2amd_world_set_refit_order(s, nullptr, 0), S2AMD_OK); // (clearing an order is no order)
		}
		EXPECT(set(s, {}, {}, 0), S2AMD_OK); // cleared: count 0 at once, every getter answers nothing
		askAll(s, false, -1, false);
		if (agents > 0)
		{
			EXPECT(s2amd_world_set_tree(s, 0, nullptr, 0, -1), S2AMD_OK);
			EXPECT(set(s, bodies, joints, agents), S2AMD_E_STATE);
			EXPECT(s->resetAgents, 0);
			EXPECT(set(s, {}, {}, 0), S2AMD_OK); // (an empty list is no list)
			EXPECT(upload(s, w), S2AMD_OK);		 // the upload forgets the trees
			if (!order.empty())
			{
				EXPECT(s2amd_world_set_refit_order(s, order.data(), (int32_t)order.size()), S2AMD_OK);
				EXPECT(set(s, bodies, joints, agents), S2AMD_E_STATE);
				EXPECT(s2amd_world_set_refit_order(s, nullptr, 0), S2AMD_OK);
			}
		}
		// replaced by a shorter list under another seed: counters zero, the getters shut until a pass
		std::vector<s2amdResetBody> fewer;
		std::vector<s2amdResetJoint> fewerJoints;
		const int fewerAgents = agents > 1 ? agents / 2 : agents;
		makeLists(records / 3, fewerAgents, fewer, fewerJoints);
		EXPECT(set(s, fewer, fewerJoints, fewerAgents, 99u), S2AMD_OK);
		EXPECT((int)s->resetSeed, fewerAgents > 0 ? 99 : (int)s->resetSeed);
		checkBlock(s, fewer, fewerJoints);
		askAll(s, false, -1, false);
		// the first list again, for the next upload
		EXPECT(set(s, bodies, joints, agents), S2AMD_OK);
		checkBlock(s, bodies, joints);
		EXPECT(s2amd_world_set_reset_report(s, BOTH), S2AMD_OK);
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0), small = makeWorld(40), big = makeWorld(300);
	const int sizes[6][2] = {{0, 0}, {1, 1}, {3, 12}, {65, 300}, {257, 1025}, {S2AMD_MAX_RESET_AGENTS, S2AMD_MAX_RESET_BODIES}};
	for (const int* size : sizes)
	{
		drive(small, big, size[0], size[1]);
		if (size[1] <= 1025)
		{
			drive(none, small, size[0], size[1]);
		}
	}
	if (failures == 0)
	{
		printf("RESETS MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
