// TEST INFRASTRUCTURE.  The host side of the force fields (solver2d_amd/csrc/force_field.hip: validation, the one-shot call with its
// pinned stage, the persistent list and its replacement, the states getter's state machine, the lazily built body -> shapes list and
// the step hook in world.hip) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and
// linked against _build/libs2amd_hostcheck.so: every validation rule -> the calls without a world -> uploads with other capacities ->
// one-shot calls with and without states -> lists set, replaced, refused and cleared between steps -> destroy.  Kernels never run here:
// what is checked is that the host side touches only memory it owns -- every buffer is a heap block of exactly the size passed -- and
// the bookkeeping the header states.  Built and run by tests/test_force_field_host.py.
#include "report_main_common.h"

static s2amdField makeField(int k, int bodies)
{
	s2amdField f = {};
	f.count = 1 + k % 8;
	for (int i = 0; i < f.count; ++i)
	{
		f.vertices[i][0] = 0.1f * (float)i, f.vertices[i][1] = 0.05f * (float)(i * i);
	}
	f.radius = 0.25f, f.range = k % 3 == 0 ? 0.0f : 2.0f;
	f.position[0] = 0.5f * (float)(k % 40), f.position[1] = 1.0f;
	f.rot[0] = 0.0f, f.rot[1] = 1.0f;
	f.maskBits = 0xffffffffu;
	f.body = k % 2 == 0 || bodies <= 0 ? -1 : k % bodies;
	f.kind = 1 + k % 3;
	f.flags = k % 8;
	f.strength = k % 2 == 0 ? 1.5f : -0.5f;
	f.direction[0] = 0.6f, f.direction[1] = -0.8f;
	return f;
}

static std::vector<s2amdField> makeList(int count, int bodies)
{
	std::vector<s2amdField> list;
	for (int k = 0; k < count; ++k)
	{
		list.push_back(makeField(k, bodies));
	}
	return list;
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdFieldState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_field_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

// every rule, through both entry points (validation comes before the state check, so the answer is the same without a world)
static void refusals(s2amdSolver* s, int bodies)
{
	const std::vector<s2amdField> list = makeList(9, bodies);
	const size_t held = s->hFields.size();
	EXPECT(s2amd_world_set_fields(s, list.data(), -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_fields(s, nullptr, 3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_fields(nullptr, list.data(), 3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_apply_fields(s, list.data(), -1, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_apply_fields(s, nullptr, 3, nullptr), S2AMD_E_INVALID);
	EXPECT(s2amd_world_apply_fields(nullptr, list.data(), 3, nullptr), S2AMD_E_INVALID);
	const std::vector<s2amdField> many((size_t)S2AMD_MAX_FIELDS + 1, list[0]);
	EXPECT(s2amd_world_set_fields(s, many.data(), S2AMD_MAX_FIELDS + 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_apply_fields(s, many.data(), S2AMD_MAX_FIELDS + 1, nullptr), S2AMD_E_INVALID);
	for (int bad = 0; bad < 17; ++bad)
	{
		std::vector<s2amdField> wrong = list;
		s2amdField& f = wrong[(size_t)(bad % 9)];
		switch (bad)
		{
		case 0: f.count = 0; break;
		case 1: f.count = 9; break;
		case 2: f.radius = -0.5f; break;
		case 3: f.range = -1.0f; break;
		case 4: f.range = INFINITY; break;
		case 5: f.vertices[0][1] = NAN; break;
		case 6: f.flags = 8; break;
		case 7: f.rot[0] = NAN; break;
		case 8: f.kind = 0; break;
		case 9: f.kind = 4; break;
		case 10: f.reserved = 1; break;
		case 11: f.strength = NAN; break;
		case 12: f.strength = -INFINITY; break;
		case 13: f.direction[1] = INFINITY; break;
		case 14: f.position[0] = NAN; break;
		case 15: f.radius = NAN; break;
		default: f.flags = -1; break;
		}
		EXPECT(s2amd_world_set_fields(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
		EXPECT(s2amd_world_apply_fields(s, wrong.data(), (int32_t)wrong.size(), nullptr), S2AMD_E_INVALID);
	}
	if (s->worldResident)
	{
		std::vector<s2amdField> wrong = list;
		wrong[2].body = s->bodyCapacity;
		EXPECT(s2amd_world_set_fields(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
		EXPECT(s2amd_world_apply_fields(s, wrong.data(), (int32_t)wrong.size(), nullptr), S2AMD_E_INVALID);
	}
	EXPECT((int)s->hFields.size(), (int)held); // the old list stands
}

static void drive(const World& first, const World& second, int fields)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	// no resident world: validation first, then S2AMD_E_STATE; the setter is accepted and the list held for the upload
	refusals(s, 0);
	std::vector<s2amdField> list = makeList(fields, (int)first.bodies.size());
	askStates(s, 4, S2AMD_E_STATE, -7);
	EXPECT(s2amd_world_apply_fields(s, list.data(), fields, nullptr), S2AMD_E_STATE);
	EXPECT(s2amd_world_set_fields(s, list.data(), fields), S2AMD_OK);
	EXPECT((int)s->hFields.size(), fields);
	askStates(s, fields, S2AMD_E_STATE, -7);
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World* w = worlds[pass];
		const int nb = (int)w->bodies.size();
		const long builds = s->fieldAdjBuilds;
		EXPECT(upload(s, *w), S2AMD_OK);
		EXPECT(s->fieldAdjValid ? 1 : 0, 0); // an upload builds nothing for the fields
		EXPECT((int)(s->fieldAdjBuilds - builds), 0);
		EXPECT((int)s->hFields.size(), fields); // the list holds across uploads
		refusals(s, nb);
		// no step since the upload
		askStates(s, fields, fields > 0 ? S2AMD_E_STATE : S2AMD_OK, fields > 0 ? -7 : 0);
		// a list whose bodies are inside this world (validation bounds them now)
		std::vector<s2amdField> here = makeList(fields, nb);
		if (pass == 1)
		{
			// the one-shot call first: it builds the list of the world, the step after it does not build again
			Exact<s2amdFieldState> states(fields);
			EXPECT(s2amd_world_apply_fields(s, here.data(), fields, states.p), S2AMD_OK);
			EXPECT((int)(s->fieldAdjBuilds - builds), fields > 0 ? 1 : 0);
			EXPECT(s2amd_world_apply_fields(s, here.data(), fields, nullptr), S2AMD_OK);
			// ... with a shorter and a longer list than the stage holds
			EXPECT(s2amd_world_apply_fields(s, here.data(), fields / 2, nullptr), S2AMD_OK);
			const std::vector<s2amdField> longer = makeList(std::min(S2AMD_MAX_FIELDS, 2 * fields + 3), nb);
			Exact<s2amdFieldState> more((int)longer.size());
			EXPECT(s2amd_world_apply_fields(s, longer.data(), (int32_t)longer.size(), more.p), S2AMD_OK);
			EXPECT((int)(s->fieldAdjBuilds - builds), 1);
			askStates(s, fields, fields > 0 ? S2AMD_E_STATE : S2AMD_OK, fields > 0 ? -7 : 0); // a one-shot call is no step
		}
		EXPECT(s2amd_world_set_fields(s, here.data(), fields), S2AMD_OK);
		for (int step = 0; step < 3; ++step)
		{
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			EXPECT((int)(s->fieldAdjBuilds - builds), fields > 0 || pass == 1 ? 1 : 0); // built once per upload, only when used
			askStates(s, -1, S2AMD_E_INVALID, -7);
			if (fields > 0)
			{
				askStates(s, fields - 1, S2AMD_E_CAPACITY, fields);
			}
			askStates(s, fields, S2AMD_OK, fields);
			askStates(s, fields + 2, S2AMD_OK, fields);
		}
		// a refused list leaves the old one and its states
		refusals(s, nb);
		askStates(s, fields, S2AMD_OK, fields);
		// replaced: the last application is not of this list; cleared: count 0 at once, and a step enqueues nothing
		std::vector<s2amdField> reversed(here.rbegin(), here.rend());
		EXPECT(s2amd_world_set_fields(s, reversed.data(), fields), S2AMD_OK);
		askStates(s, fields, fields > 0 ? S2AMD_E_STATE : S2AMD_OK, fields > 0 ? -7 : 0);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		askStates(s, fields, S2AMD_OK, fields);
		EXPECT(s2amd_world_set_fields(s, nullptr, 0), S2AMD_OK);
		askStates(s, 0, S2AMD_OK, 0);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		askStates(s, 0, S2AMD_OK, 0);
		const std::vector<s2amdField> one = makeList(1, nb);
		EXPECT(s2amd_world_set_fields(s, one.data(), 1), S2AMD_OK); // a shorter list in the block of the longer one
		askStates(s, 1, S2AMD_E_STATE, -7);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		askStates(s, 1, S2AMD_OK, 1);
		EXPECT(s2amd_world_set_fields(s, here.data(), fields), S2AMD_OK); // (held for the next upload, whose world may be smaller)
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0);
	World empty = makeWorld(3);
	empty.shapes.clear(); // no shape slots at all: nothing to sort, no apply launch
	const World small = makeWorld(40), big = makeWorld(700);
	const int counts[5] = {0, 1, 129, 257, S2AMD_MAX_FIELDS};
	for (int fields : counts)
	{
		drive(small, big, fields);
		drive(big, none, fields);
		drive(empty, small, fields);
	}
	if (failures == 0)
	{
		printf("FORCE FIELD MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
