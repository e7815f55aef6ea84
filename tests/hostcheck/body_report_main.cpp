// TEST INFRASTRUCTURE.  The host side of the body report (solver2d_amd/csrc/body_report.hip: layout, prepare, enqueue, setters, getters)
// on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and linked against
// _build/libs2amd_hostcheck.so: upload -> every flag combination -> thresholds set, changed and refused -> every getter with too-small,
// exact and ample buffers -> uploads with other capacities -> destroy.  Kernels never run here, so the head the write pass would leave
// (counts and summary) is written by this program at the report state's headOffset: what is checked is that the host side touches only memory
// it owns -- every output buffer is a heap block of exactly the size passed.  Built and run by tests/test_body_report_host.py.
#include "report_main_common.h"

// in place of the write pass: {records, rested, woke, islands} and a summary
static void writeHead(s2amdSolver* s, int records, int rested, int woke, int islands)
{
	struct
	{
		int32_t counts[4];
		s2amdBodySummary summary;
	} head = {};
	head.counts[0] = records, head.counts[1] = rested, head.counts[2] = woke, head.counts[3] = islands;
	head.summary.bodies = records, head.summary.islands = islands;
	memcpy((char*)s->bodyReport.block.p + s->bodyReport.headOffset, &head, sizeof(head));
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdBodyState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_body_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void askIslands(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdIslandState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_islands(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void askEvents(s2amdSolver* s, int capacityR, int capacityW, int wantRc, int wantR, int wantW)
{
	Exact<int32_t> rested(capacityR), woke(capacityW);
	int32_t nR = -7, nW = -7;
	EXPECT(s2amd_world_body_rest_events(s, rested.p, capacityR, &nR, woke.p, capacityW, &nW), wantRc);
	EXPECT(nR, wantR);
	EXPECT(nW, wantW);
}

static void gettersAfterStep(s2amdSolver* s, int flags, int nb)
{
	// the largest counts the passes can leave: every slot a record and an island, every slot in one of the lists
	const int records = nb, rested = nb / 2, woke = nb - nb / 2, islands = nb;
	writeHead(s, records, rested, woke, islands);
	s2amdBodySummary summary;
	EXPECT(s2amd_world_body_summary(s, &summary), flags != 0 ? S2AMD_OK : S2AMD_E_STATE);
	if (flags != 0)
	{
		EXPECT(summary.bodies, records);
	}
	if ((flags & S2AMD_BODY_REPORT_STATES) != 0)
	{
		askStates(s, -1, S2AMD_E_INVALID, -7);
		if (records > 0)
		{
			askStates(s, records - 1, S2AMD_E_CAPACITY, records);
			askStates(s, 0, S2AMD_E_CAPACITY, records);
		}
		askStates(s, records, S2AMD_OK, records);
		askStates(s, records + 5, S2AMD_OK, records);
	}
	else
	{
		askStates(s, 4, S2AMD_E_STATE, -7);
	}
	if ((flags & S2AMD_BODY_REPORT_ISLANDS) != 0)
	{
		askIslands(s, -1, S2AMD_E_INVALID, -7);
		if (islands > 0)
		{
			askIslands(s, islands - 1, S2AMD_E_CAPACITY, islands);
		}
		askIslands(s, islands, S2AMD_OK, islands);
		askIslands(s, islands + 7, S2AMD_OK, islands);
	}
	else
	{
		askIslands(s, 4, S2AMD_E_STATE, -7);
	}
	if ((flags & S2AMD_BODY_REPORT_REST) != 0)
	{
		if (rested > 0)
		{
			askEvents(s, rested - 1, woke, S2AMD_E_CAPACITY, rested, woke);
		}
		if (woke > 0)
		{
			askEvents(s, rested, woke - 1, S2AMD_E_CAPACITY, rested, woke);
		}
		askEvents(s, rested, woke, S2AMD_OK, rested, woke);
		askEvents(s, rested + 3, woke + 9, S2AMD_OK, rested, woke);
	}
	else
	{
		askEvents(s, 4, 4, S2AMD_E_STATE, -7, -7);
	}
}

static void drive(const World& first, const World& second, bool flagsFirst)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	s2amdBodySummary summary;
	EXPECT(s2amd_world_set_body_report(s, 16), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_body_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_body_summary(s, &summary), S2AMD_E_STATE); // no resident world
	EXPECT(s2amd_world_set_rest_thresholds(s, -0.5f, 1.0f, 1.0f), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_rest_thresholds(s, 0.5f, NAN, 1.0f), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_rest_thresholds(s, 0.5f, 1.0f, -1.0f), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_rest_thresholds(s, 0.5f, 1.745f, 0.05f), S2AMD_OK); // before any world: held for the upload
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_body_report(s, 15), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	for (const World* w : worlds)
	{
		const int nb = (int)w->bodies.size();
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_body_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_body_report(s, 15), S2AMD_OK); // prepares on the resident world
		}
		EXPECT(s2amd_world_body_summary(s, &summary), S2AMD_E_STATE); // no step since the upload
		for (int flags = 15; flags >= 0; --flags)
		{
			EXPECT(s2amd_world_set_body_report(s, flags), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			if (flags != 0)
			{
				gettersAfterStep(s, flags, nb);
			}
			else
			{
				EXPECT(s2amd_world_body_summary(s, &summary), S2AMD_E_STATE);
				askStates(s, 4, S2AMD_E_STATE, -7);
				askIslands(s, 4, S2AMD_E_STATE, -7);
			}
			// the thresholds changed between steps, to zero as well; bad ones leave them as they were
			EXPECT(s2amd_world_set_rest_thresholds(s, 0.25f * (float)(flags % 3), 0.5f * (float)(flags % 2), 0.125f * (float)(flags % 4)), S2AMD_OK);
			EXPECT(s2amd_world_set_rest_thresholds(s, NAN, 0.0f, 0.0f), S2AMD_E_INVALID);
		}
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0); // the static ground alone: nobody is reported
	World empty = makeWorld(3);
	empty.bodies.clear(), empty.origins.clear(), empty.shapes.clear(); // no body slots at all: the head is known without the device
	const World small = makeWorld(40), big = makeWorld(700); // one tile; more than three
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		drive(small, big, flagsFirst != 0);
		drive(big, none, flagsFirst != 0);
		drive(empty, small, flagsFirst != 0);
	}
	if (failures == 0)
	{
		printf("BODY REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
