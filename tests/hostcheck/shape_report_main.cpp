// TEST INFRASTRUCTURE.  The host side of the shape report (solver2d_amd/csrc/shape_report.hip: layout, prepare, enqueue, setters, getters)
// on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and linked against
// _build/libs2amd_hostcheck.so: upload -> every flag combination -> a view set, changed and cleared -> every getter with too-small, exact
// and ample buffers -> a second upload with other capacities -> destroy.  Kernels never run here, so the head the write pass would leave
// (counts and summary) is written by this program at the report state's headOffset: what is checked is that the host side touches only memory
// it owns -- every output buffer is a heap block of exactly the size passed.  Built and run by tests/test_shape_report_host.py.
#include "report_main_common.h"

// in place of the write pass: {in view, entered, left} and a summary
static void writeHead(s2amdSolver* s, int inView, int entered, int left)
{
	struct
	{
		int32_t counts[4];
		s2amdShapeSummary summary;
	} head = {};
	head.counts[0] = inView, head.counts[1] = entered, head.counts[2] = left;
	head.summary.liveShapes = inView, head.summary.inView = inView;
	memcpy((char*)s->shapeReport.block.p + s->shapeReport.headOffset, &head, sizeof(head));
}

static void askDraws(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdShapeDraw> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_shape_draws(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void askEvents(s2amdSolver* s, int capacityE, int capacityL, int wantRc, int wantE, int wantL)
{
	Exact<int32_t> entered(capacityE), left(capacityL);
	int32_t nE = -7, nL = -7;
	EXPECT(s2amd_world_shape_view_events(s, entered.p, capacityE, &nE, left.p, capacityL, &nL), wantRc);
	EXPECT(nE, wantE);
	EXPECT(nL, wantL);
}

static void gettersAfterStep(s2amdSolver* s, int flags, int ns)
{
	// the largest counts the passes can leave: every slot in view, every slot in one of the lists
	const int inView = ns, entered = ns / 2, left = ns - ns / 2;
	writeHead(s, inView, entered, left);
	s2amdShapeSummary summary;
	EXPECT(s2amd_world_shape_summary(s, &summary), flags != 0 ? S2AMD_OK : S2AMD_E_STATE);
	if (flags != 0)
	{
		EXPECT(summary.inView, inView);
	}
	if ((flags & S2AMD_SHAPE_REPORT_DRAW) != 0)
	{
		askDraws(s, -1, S2AMD_E_INVALID, -7);
		if (inView > 0)
		{
			askDraws(s, inView - 1, S2AMD_E_CAPACITY, inView);
			askDraws(s, 0, S2AMD_E_CAPACITY, inView);
		}
		askDraws(s, inView, S2AMD_OK, inView);
		askDraws(s, inView + 5, S2AMD_OK, inView);
	}
	else
	{
		askDraws(s, 4, S2AMD_E_STATE, -7);
	}
	if ((flags & S2AMD_SHAPE_REPORT_VIEW) != 0)
	{
		if (entered > 0)
		{
			askEvents(s, entered - 1, left, S2AMD_E_CAPACITY, entered, left);
		}
		if (left > 0)
		{
			askEvents(s, entered, left - 1, S2AMD_E_CAPACITY, entered, left);
		}
		askEvents(s, entered, left, S2AMD_OK, entered, left);
		askEvents(s, entered + 3, left + 9, S2AMD_OK, entered, left);
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
	s2amdShapeSummary summary;
	EXPECT(s2amd_world_set_shape_report(s, 8), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_shape_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_shape_summary(s, &summary), S2AMD_E_STATE); // no resident world
	const float upsideDown[4] = {1.0f, 0.0f, 0.0f, 1.0f}, withNaN[4] = {0.0f, 0.0f, NAN, 1.0f}, wide[4] = {-100.0f, -100.0f, 100.0f, 100.0f};
	const float narrow[4] = {2.0f, 0.0f, 6.0f, 4.0f}, point[4] = {1.0f, 1.0f, 1.0f, 1.0f};
	EXPECT(s2amd_world_set_shape_view(s, upsideDown), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_shape_view(s, withNaN), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_shape_view(s, narrow), S2AMD_OK); // before any world: held for the upload
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_shape_report(s, 7), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	for (const World* w : worlds)
	{
		const int ns = (int)w->shapes.size();
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_shape_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_shape_report(s, 7), S2AMD_OK); // prepares on the resident world
		}
		EXPECT(s2amd_world_shape_summary(s, &summary), S2AMD_E_STATE); // no step since the upload
		for (int flags = 7; flags >= 0; --flags)
		{
			EXPECT(s2amd_world_set_shape_report(s, flags), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			if (flags != 0)
			{
				gettersAfterStep(s, flags, ns);
			}
			else
			{
				EXPECT(s2amd_world_shape_summary(s, &summary), S2AMD_E_STATE);
				askDraws(s, 4, S2AMD_E_STATE, -7);
			}
			// the view changed, set to a point and cleared between steps; a bad one leaves it as it was
			const float* views[4] = {wide, point, nullptr, narrow};
			EXPECT(s2amd_world_set_shape_view(s, views[flags % 4]), S2AMD_OK);
			EXPECT(s2amd_world_set_shape_view(s, withNaN), S2AMD_E_INVALID);
		}
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0);
	World empty = makeWorld(3);
	empty.shapes.clear(); // no shape slots at all: the head is known without the device
	const World small = makeWorld(40), big = makeWorld(700); // one tile; more than three
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		drive(small, big, flagsFirst != 0);
		drive(big, none, flagsFirst != 0);
		drive(empty, small, flagsFirst != 0);
	}
	if (failures == 0)
	{
		printf("SHAPE REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
