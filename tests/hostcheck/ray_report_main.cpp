// TEST INFRASTRUCTURE.  The host side of the ray report (solver2d_amd/csrc/ray_report.hip: layout, prepare, enqueue, the two setters, the
// four getters, and report_host.cpp behind them) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with
// ASan + UBSan and linked against _build/libs2amd_hostcheck.so: the setter with good and bad lists -> every flag combination 0..7 ->
// every getter with too-small, exact and ample buffers -> the list replaced and cleared between steps -> uploads with other capacities
// -> destroy, for 0, 1, 257 and 16,384 rays.  Kernels never run here, so the head the events pass would leave (the event count) is
// written by this program at the report state's headOffset: what is checked is that the host side touches only memory it owns -- every
// output buffer is a heap block of exactly the size passed.  Built and run by tests/test_ray_report_host.py.
#include "report_main_common.h"

static void writeHead(s2amdSolver* s, int events)
{
	const int32_t head[4] = {events, 0, 0, 0};
	memcpy((char*)s->rayReport.block.p + s->rayReport.headOffset, head, sizeof(head));
	s->rayReport.headKnown = false;
}

static s2amdRaySensor makeRay(int k, int bodies)
{
	s2amdRaySensor q = {};
	q.p1[0] = 0.5f * (float)(k % 40), q.p1[1] = 3.0f;
	q.p2[0] = q.p1[0] + 0.01f * (float)(k % 64), q.p2[1] = -1.0f;
	q.maxFraction = k % 3 == 0 ? 0.0f : 1.0f;
	q.maskBits = 0xffffffffu;
	q.body = k % 2 == 0 || bodies <= 0 ? -1 : k % bodies;
	q.flags = k % 5 == 4 ? S2AMD_RAY_SENSOR_DISABLED : k % 5 == 3 ? S2AMD_RAY_SENSOR_SKIP_STATIC : 0;
	return q;
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdRayState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_ray_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void askRanges(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<float> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_ray_ranges(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

// (device memory of the stand-in runtime is host memory: the export's destination is an exact heap block as well)
static void askExport(s2amdSolver* s, int capacity, int wantRc)
{
	Exact<float> out(capacity);
	EXPECT(s2amd_world_export_ray_ranges(s, out.p, capacity), wantRc);
}

static void askEvents(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdRayEvent> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_ray_events(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void gettersRefuse(s2amdSolver* s, int rays)
{
	askStates(s, rays + 1, S2AMD_E_STATE, -7);
	askRanges(s, rays + 1, S2AMD_E_STATE, -7);
	askExport(s, rays + 1, S2AMD_E_STATE);
	askEvents(s, rays + 1, S2AMD_E_STATE, -7);
}

static void gettersAfterStep(s2amdSolver* s, int flags, int rays, int pass)
{
	const int events = std::min(rays, pass == 0 ? 0 : pass == 1 ? 3 : rays);
	if (rays > 0 && (flags & S2AMD_RAY_REPORT_EVENTS) != 0)
	{
		writeHead(s, events);
	}
	if ((flags & S2AMD_RAY_REPORT_STATES) != 0)
	{
		askStates(s, -1, S2AMD_E_INVALID, -7);
		if (rays > 0)
		{
			askStates(s, rays - 1, S2AMD_E_CAPACITY, rays);
			askStates(s, 0, S2AMD_E_CAPACITY, rays);
		}
		askStates(s, rays, S2AMD_OK, rays);
		askStates(s, rays + 2, S2AMD_OK, rays);
	}
	else
	{
		askStates(s, rays + 1, S2AMD_E_STATE, -7);
	}
	if ((flags & S2AMD_RAY_REPORT_RANGES) != 0)
	{
		askRanges(s, -1, S2AMD_E_INVALID, -7);
		askExport(s, -1, S2AMD_E_INVALID);
		if (rays > 0)
		{
			askRanges(s, rays - 1, S2AMD_E_CAPACITY, rays);
			askExport(s, rays - 1, S2AMD_E_CAPACITY);
		}
		askRanges(s, rays, S2AMD_OK, rays);
		askRanges(s, rays + 5, S2AMD_OK, rays);
		askExport(s, rays, S2AMD_OK);
		askExport(s, rays + 5, S2AMD_OK);
	}
	else
	{
		askRanges(s, rays + 1, S2AMD_E_STATE, -7);
		askExport(s, rays + 1, S2AMD_E_STATE);
	}
	if ((flags & S2AMD_RAY_REPORT_EVENTS) != 0)
	{
		askEvents(s, -1, S2AMD_E_INVALID, -7);
		if (events > 0)
		{
			askEvents(s, events - 1, S2AMD_E_CAPACITY, events);
			askEvents(s, 0, S2AMD_E_CAPACITY, events);
		}
		askEvents(s, events, S2AMD_OK, events);
		askEvents(s, events + 3, S2AMD_OK, events);
	}
	else
	{
		askEvents(s, rays + 1, S2AMD_E_STATE, -7);
	}
}

static void setterRefusals(s2amdSolver* s, int bodies)
{
	std::vector<s2amdRaySensor> list;
	for (int k = 0; k < 9; ++k)
	{
		list.push_back(makeRay(k, bodies));
	}
	EXPECT(s2amd_world_set_ray_sensors(s, list.data(), -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_ray_sensors(s, nullptr, 3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_ray_sensors(nullptr, list.data(), 3), S2AMD_E_INVALID);
	std::vector<s2amdRaySensor> many((size_t)S2AMD_MAX_RAY_SENSORS + 1, list[0]);
	EXPECT(s2amd_world_set_ray_sensors(s, many.data(), S2AMD_MAX_RAY_SENSORS + 1), S2AMD_E_INVALID);
	for (int bad = 0; bad < 7; ++bad)
	{
		std::vector<s2amdRaySensor> wrong = list;
		s2amdRaySensor& q = wrong[(size_t)bad];
		switch (bad)
		{
		case 0: q.maxFraction = -0.5f; break;
		case 1: q.maxFraction = 100000.0f; break;
		case 2: q.maxFraction = NAN; break;
		case 3: q.p1[1] = INFINITY; break;
		case 4: q.p2[0] = NAN; break;
		case 5: q.flags = 4; break;
		default: q.flags = -1; break;
		}
		EXPECT(s2amd_world_set_ray_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
	if (s->worldResident)
	{
		std::vector<s2amdRaySensor> wrong = list;
		wrong[2].body = s->bodyCapacity;
		EXPECT(s2amd_world_set_ray_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
}

static void drive(const World& first, const World& second, int rays, bool flagsFirst)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	EXPECT(s2amd_world_set_ray_report(s, 8), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_ray_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_ray_report(nullptr, 7), S2AMD_E_INVALID);
	gettersRefuse(s, 3); // no resident world
	setterRefusals(s, 0);
	std::vector<s2amdRaySensor> list;
	for (int k = 0; k < rays; ++k)
	{
		list.push_back(makeRay(k, (int)first.bodies.size()));
	}
	EXPECT(s2amd_world_set_ray_sensors(s, list.data(), rays), S2AMD_OK); // before any world: held for the upload
	EXPECT((int)s->hRaySensors.size(), rays);
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_ray_report(s, 7), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World* w = worlds[pass];
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_ray_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_ray_report(s, 7), S2AMD_OK); // prepares on the resident world
		}
		gettersRefuse(s, rays);					  // no step since the upload
		setterRefusals(s, (int)w->bodies.size()); // ... and the list that holds is still the good one
		EXPECT((int)s->hRaySensors.size(), rays);
		for (int flags = 7; flags >= 0; --flags)
		{
			EXPECT(s2amd_world_set_ray_report(s, flags), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			if (flags != 0)
			{
				gettersAfterStep(s, flags, rays, (flags + pass) % 3);
			}
			else
			{
				gettersRefuse(s, rays);
			}
			if (flags == 4 || flags == 7)
			{
				// the list replaced between steps (the same rays in reverse), and cleared and set again: the last report is void
				std::vector<s2amdRaySensor> reversed(list.rbegin(), list.rend());
				for (s2amdRaySensor& q : reversed)
				{
					q.body = q.body >= (int)w->bodies.size() ? -1 : q.body;
				}
				EXPECT(s2amd_world_set_ray_sensors(s, reversed.data(), rays), S2AMD_OK);
				gettersRefuse(s, rays);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, rays, 2);
				EXPECT(s2amd_world_set_ray_sensors(s, nullptr, 0), S2AMD_OK);
				gettersRefuse(s, 0);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, 0, 1);
				EXPECT(s2amd_world_set_ray_sensors(s, reversed.data(), rays), S2AMD_OK);
				if (rays <= S2AMD_MAX_RAY_SENSORS / 4)
				{
					// a longer list whose block cannot be had (longer than any before it: the block never shrinks): the setter fails
					// with the allocation's message, and the list before stands with its block, prepared again -- the next step reports it
					std::vector<s2amdRaySensor> longer((size_t)4 * rays + 1024, makeRay(1, 0));
					setenv("S2_HOSTCHECK_FAIL_MALLOC", "1", 1);
					EXPECT(s2amd_world_set_ray_sensors(s, longer.data(), (int32_t)longer.size()), S2AMD_E_DEVICE);
					unsetenv("S2_HOSTCHECK_FAIL_MALLOC");
					EXPECT(strstr(s2amd_last_error(), "hipMalloc") != nullptr, 1);
					EXPECT((int)s->hRaySensors.size(), rays);
					EXPECT(rays == 0 || memcmp(s->hRaySensors.data(), reversed.data(), (size_t)rays * sizeof(s2amdRaySensor)) == 0, 1);
					gettersRefuse(s, rays);
					EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
					gettersAfterStep(s, flags, rays, 1);
				}
			}
		}
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0);
	World empty = makeWorld(3);
	empty.shapes.clear(); // no shape slots at all: no tile is launched
	const World small = makeWorld(40), big = makeWorld(700); // one tile; more than three
	const int counts[4] = {0, 1, 257, S2AMD_MAX_RAY_SENSORS};
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		for (int rays : counts)
		{
			drive(small, big, rays, flagsFirst != 0);
			drive(big, none, rays, flagsFirst != 0);
			drive(empty, small, rays, flagsFirst != 0);
		}
	}
	if (failures == 0)
	{
		printf("RAY REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
