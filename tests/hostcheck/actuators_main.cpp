// TEST INFRASTRUCTURE.  The host side of the actuators (solver2d_amd/csrc/actuators.hip: validation, the grouping by target the setter
// makes, the list's device block and its replacement, the two writers with their pinned stage, the getters' state machine and the step
// hook in world.hip) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and linked
// against _build/libs2amd_hostcheck.so: every validation rule -> the calls without a list and without a world -> uploads with other
// capacities -> lists set, replaced, refused and cleared between steps -> writes of whole and partial ranges -> destroy.  Kernels never
// run here: what is checked is that the host side touches only memory it owns -- every buffer is a heap block of exactly the size
// passed -- and the bookkeeping the header states.  Built and run by tests/test_actuators_host.py.
#include "report_main_common.h"

static int widthOf(int kind)
{
	return kind == 1 || kind == 3 || kind == 7 ? 2 : 1;
}

// `count` actuators over `targets` body slots (every kind 1..4 in turn; with joints == true kinds 5..7 too), channels packed
static std::vector<s2amdActuator> makeList(int count, int targets, bool joints, int* channels)
{
	std::vector<s2amdActuator> list;
	int at = 0;
	for (int k = 0; k < count; ++k)
	{
		s2amdActuator a = {};
		a.kind = 1 + k % (joints ? 7 : 4);
		a.target = targets > 0 ? k % targets : 0;
		a.channel = at;
		a.flags = k % 5 == 4 ? S2AMD_ACTUATOR_DISABLED : 0;
		a.gain = 1.5f, a.bias = -0.25f, a.lower = k % 2 == 0 ? -INFINITY : -2.0f, a.upper = k % 3 == 0 ? INFINITY : 2.0f;
		a.axis[0] = 0.6f, a.axis[1] = 0.8f, a.kp = 2.0f, a.maxSpeed = k % 4 == 0 ? INFINITY : 1.0f;
		at += widthOf(a.kind);
		list.push_back(a);
	}
	*channels = at > 0 ? at : 1;
	return list;
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdActuatorState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_actuator_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
	Exact<int32_t> counts(4);
	EXPECT(s2amd_world_actuator_counts(s, counts.p), wantRc == S2AMD_E_CAPACITY || wantRc == S2AMD_E_INVALID ? S2AMD_OK : wantRc);
}

static void refusals(s2amdSolver* s)
{
	int channels = 0;
	const std::vector<s2amdActuator> list = makeList(9, 1, false, &channels);
	const size_t held = s->hActuators.size();
	const int heldChannels = s->actuatorChannels;
	EXPECT(s2amd_world_set_actuators(s, list.data(), -1, channels), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actuators(s, nullptr, 3, channels), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actuators(nullptr, list.data(), 3, channels), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actuators(s, list.data(), 9, 0), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actuators(s, list.data(), 9, S2AMD_MAX_ACTION_CHANNELS + 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actuators(s, list.data(), 9, channels - 1), S2AMD_E_INVALID); // the last actuator's channels
	const std::vector<s2amdActuator> many((size_t)S2AMD_MAX_ACTUATORS + 1, list[1]);
	EXPECT(s2amd_world_set_actuators(s, many.data(), S2AMD_MAX_ACTUATORS + 1, channels), S2AMD_E_INVALID);
	for (int bad = 0; bad < 18; ++bad)
	{
		std::vector<s2amdActuator> wrong = list;
		s2amdActuator& a = wrong[(size_t)(bad % 9)];
		switch (bad)
		{
		case 0: a.kind = 0; break;
		case 1: a.kind = 8; break;
		case 2: a.target = -1; break;
		case 3: a.channel = -1; break;
		case 4: a.channel = channels; break;
		case 5: a.flags = 2; break;
		case 6: a.flags = -1; break;
		case 7: a.reserved[3] = 1; break;
		case 8: a.gain = NAN; break;
		case 9: a.bias = INFINITY; break;
		case 10: a.axis[1] = NAN; break;
		case 11: a.kp = -INFINITY; break;
		case 12: a.lower = NAN; break;
		case 13: a.upper = NAN; break;
		case 14: a.lower = 3.0f, a.upper = 2.0f; break;
		case 15: a.maxSpeed = -1.0f; break;
		case 16: a.maxSpeed = NAN; break;
		default: a.channel = INT32_MAX; break; // (channel + width must not wrap)
		}
		EXPECT(s2amd_world_set_actuators(s, wrong.data(), (int32_t)wrong.size(), channels), S2AMD_E_INVALID);
	}
	if (s->worldResident)
	{
		std::vector<s2amdActuator> wrong = list;
		wrong[2].target = s->bodyCapacity;
		EXPECT(s2amd_world_set_actuators(s, wrong.data(), (int32_t)wrong.size(), channels), S2AMD_E_INVALID);
	}
	EXPECT((int)s->hActuators.size(), (int)held); // the old list and its buffer stand
	EXPECT(s->actuatorChannels, heldChannels);
}

static void writers(s2amdSolver* s, int channels)
{
	Exact<float> values(channels);
	for (int i = 0; i < channels; ++i)
	{
		values.p[i] = 0.25f * (float)i;
	}
	void* device = nullptr;
	EXPECT(s2amd_device_alloc(s, 4u * (uint64_t)channels, &device), S2AMD_OK);
	EXPECT(s2amd_device_write(s, device, values.p, 4u * (uint64_t)channels), S2AMD_OK);
	EXPECT(s2amd_device_write(s, nullptr, values.p, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_device_write(s, device, nullptr, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_device_write(s, nullptr, nullptr, 0), S2AMD_OK);
	const bool have = !s->hActuators.empty();
	const int ok = have ? S2AMD_OK : S2AMD_E_STATE;
	EXPECT(s2amd_world_set_actions(s, values.p, 0, have ? s->actuatorChannels : channels), ok);
	EXPECT(s2amd_world_set_actions(s, values.p, 0, 1), ok); // (twice in a row: the stage's event)
	EXPECT(s2amd_world_import_actions(s, device, 0, have ? s->actuatorChannels : channels), ok);
	if (have)
	{
		const int n = s->actuatorChannels;
		EXPECT(s2amd_world_set_actions(s, values.p, n - 1, 1), S2AMD_OK);
		EXPECT(s2amd_world_import_actions(s, device, n - 1, 1), S2AMD_OK);
		EXPECT(s2amd_world_set_actions(s, values.p, n, 0), S2AMD_OK);
		EXPECT(s2amd_world_set_actions(s, values.p, n, 1), S2AMD_E_INVALID);
		EXPECT(s2amd_world_set_actions(s, values.p, 1, n), S2AMD_E_INVALID);
		EXPECT(s2amd_world_import_actions(s, device, INT32_MAX, 2), S2AMD_E_INVALID);
	}
	EXPECT(s2amd_world_set_actions(s, nullptr, 0, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_actions(s, values.p, -1, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_import_actions(s, device, 0, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_import_actions(nullptr, device, 0, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_device_free(s, device), S2AMD_OK);
}

static void drive(const World& first, const World& second, int count, int targets)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	int channels = 0;
	// no list, no world
	refusals(s);
	askStates(s, 4, S2AMD_OK, 0);
	writers(s, 8);
	// a list before any world: targets are not bounded yet, joint kinds included
	std::vector<s2amdActuator> list = makeList(count, targets, true, &channels);
	EXPECT(s2amd_world_set_actuators(s, list.data(), count, channels), S2AMD_OK);
	EXPECT((int)s->hActuators.size(), count);
	EXPECT(s->actuatorsRepeated ? 1 : 0, count > targets ? 1 : 0);
	askStates(s, count, count > 0 ? S2AMD_E_STATE : S2AMD_OK, count > 0 ? -7 : 0);
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World* w = worlds[pass];
		const int nb = (int)w->bodies.size();
		EXPECT(upload(s, *w), S2AMD_OK);
		EXPECT((int)s->hActuators.size(), count); // the list holds across uploads
		refusals(s);
		askStates(s, count, count > 0 ? S2AMD_E_STATE : S2AMD_OK, count > 0 ? -7 : 0); // no step since the upload
		writers(s, channels);
		for (int step = 0; step < 3; ++step)
		{
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK); // (targets outside this world: the kernel's own bounds tests)
			askStates(s, -1, S2AMD_E_INVALID, -7);
			if (count > 0)
			{
				askStates(s, count - 1, S2AMD_E_CAPACITY, count);
			}
			askStates(s, count, S2AMD_OK, count);
			askStates(s, count + 2, S2AMD_OK, count);
		}
		refusals(s);
		askStates(s, count, S2AMD_OK, count);
		// replaced by a list inside this world, on distinct targets where it has that many bodies
		int here = 0;
		const int distinct = std::min(count, nb);
		std::vector<s2amdActuator> inside = makeList(distinct, nb, false, &here);
		for (int k = 0; k < distinct; ++k)
		{
			inside[(size_t)k].target = k;
		}
		EXPECT(s2amd_world_set_actuators(s, inside.data(), distinct, here), S2AMD_OK);
		EXPECT(s->actuatorsRepeated ? 1 : 0, 0);
		if (count > 0 && count <= S2AMD_MAX_ACTUATORS / 4)
		{
			// a longer list whose block cannot be had: the setter fails with the allocation's message before it commits anything
			int more = 0;
			std::vector<s2amdActuator> longer = makeList(4 * count + 64, nb, false, &more);
			setenv("S2_HOSTCHECK_FAIL_MALLOC", "1", 1);
			EXPECT(s2amd_world_set_actuators(s, longer.data(), (int32_t)longer.size(), more), S2AMD_E_DEVICE);
			unsetenv("S2_HOSTCHECK_FAIL_MALLOC");
			EXPECT(strstr(s2amd_last_error(), "hipMalloc") != nullptr, 1);
			EXPECT((int)s->hActuators.size(), distinct);
			EXPECT(s->actuatorChannels, here);
		}
		askStates(s, distinct, distinct > 0 ? S2AMD_E_STATE : S2AMD_OK, distinct > 0 ? -7 : 0);
		writers(s, here);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		askStates(s, distinct, S2AMD_OK, distinct);
		// cleared: count 0 at once, and a step enqueues nothing
		EXPECT(s2amd_world_set_actuators(s, nullptr, 0, 0), S2AMD_OK);
		askStates(s, 0, S2AMD_OK, 0);
		writers(s, 4);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		// the first list again, for the next upload: bounded by this world now
		std::vector<s2amdActuator> again = makeList(count, std::min(targets, nb), false, &channels);
		EXPECT(s2amd_world_set_actuators(s, again.data(), count, channels), S2AMD_OK);
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0), small = makeWorld(40), big = makeWorld(700);
	const int counts[6] = {0, 1, 65, 257, 1000, S2AMD_MAX_ACTUATORS};
	for (int count : counts)
	{
		drive(small, big, count, 30);
		drive(big, none, count, 700);
		drive(none, small, count, 1);
	}
	if (failures == 0)
	{
		printf("ACTUATORS MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
