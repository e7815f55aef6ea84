// TEST INFRASTRUCTURE.  The host side of the step metrics (solver2d_amd/csrc/step_metrics.hip: layout, prepare, enqueue, setter, the two
// getters and the wrap split of the history copy) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with
// ASan + UBSan and linked against _build/libs2amd_hostcheck.so: every flag combination -> history lengths 1, 5 and 4096 -> more steps
// than the ring holds -> both getters with too-small, exact and ample buffers -> a restart by the setter and one by an upload -> uploads
// with other capacities -> destroy.  Kernels never run here, so this program writes into the ring what the finishing kernel would (the
// record's `step` at position step % length): what is checked is that the host side touches only memory it owns -- every output buffer
// is a heap block of exactly the size passed -- and that the history comes out oldest first.  Built and run by
// tests/test_step_metrics_host.py.
#include "report_main_common.h"

// body 0 static with a ground box; `count` unit-mass bodies above it, one small box each that collides with nothing; `contactSlots` free
// contact slots and `jointSlots` free joint slots (the metrics' tiles are sized by the capacities, whatever the slots hold)
static World makeWorld(int count, int contactSlots, int jointSlots)
{
	World w;
	w.bodies.assign((size_t)count + 1, s2amdBody{});
	w.origins.assign(2 * ((size_t)count + 1), 0.0f);
	for (size_t i = 0; i < w.bodies.size(); ++i)
	{
		s2amdBody& b = w.bodies[i];
		b.rot[0] = 0.0f, b.rot[1] = 1.0f;
		b.gravityScale = 1.0f;
		b.type = i == 0 ? S2AMD_BODY_STATIC : S2AMD_BODY_DYNAMIC;
		if (i > 0)
		{
			b.position[0] = 0.5f * (float)(i % 40), b.position[1] = 1.0f + 0.5f * (float)(i / 40);
			b.mass = 1.0f, b.invMass = 1.0f, b.I = 0.5f, b.invI = 2.0f;
		}
		w.origins[2 * i] = b.position[0], w.origins[2 * i + 1] = b.position[1];
	}
	w.shapes.assign((size_t)count + 1, s2amdShape{});
	for (int body = 0; body <= count; ++body)
	{
		s2amdShape& sh = w.shapes[(size_t)body];
		const float h = body == 0 ? 10.0f : 0.125f;
		const float px = w.bodies[(size_t)body].position[0], py = w.bodies[(size_t)body].position[1];
		sh.body = body, sh.type = S2AMD_SHAPE_POLYGON;
		sh.categoryBits = 1, sh.maskBits = 0;
		sh.proxyKey = (body << 4) | w.bodies[(size_t)body].type;
		sh.count = 4;
		const float v[4][2] = {{-h, -0.125f}, {h, -0.125f}, {h, 0.125f}, {-h, 0.125f}};
		const float n[4][2] = {{0.0f, -1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}};
		for (int i = 0; i < 4; ++i)
		{
			sh.vertices[i][0] = v[i][0], sh.vertices[i][1] = v[i][1];
			sh.normals[i][0] = n[i][0], sh.normals[i][1] = n[i][1];
		}
		sh.aabb[0] = px - h, sh.aabb[1] = py - 0.125f, sh.aabb[2] = px + h, sh.aabb[3] = py + 0.125f;
		sh.fatAABB[0] = sh.aabb[0] - 0.1f, sh.fatAABB[1] = sh.aabb[1] - 0.1f, sh.fatAABB[2] = sh.aabb[2] + 0.1f, sh.fatAABB[3] = sh.aabb[3] + 0.1f;
	}
	w.contacts.assign((size_t)contactSlots, s2amdContact{});
	w.pairs.assign((size_t)contactSlots, s2amdPairState{});
	for (size_t i = 0; i < w.contacts.size(); ++i)
	{
		w.contacts[i].constraintIndex = -1;
		w.pairs[i].shapeA = w.pairs[i].shapeB = -1;
	}
	w.joints.assign((size_t)jointSlots, s2amdJoint{});
	for (s2amdJoint& j : w.joints)
	{
		j.type = S2AMD_JOINT_FREE;
	}
	return w;
}

// in place of the finishing kernel: the record of step `step` at its ring position
static void writeRecord(s2amdSolver* s, int step, int flags, int length)
{
	s2amdStepMetrics r = {};
	r.step = step, r.flags = flags;
	memcpy((s2amdStepMetrics*)s->dMetricsRing.p + step % length, &r, sizeof(r));
}

// the history with a buffer of `capacity` records; on success the steps are wantFirst, wantFirst + 1, ...
static void askHistory(s2amdSolver* s, int capacity, int wantRc, int wantCount, int wantFirst)
{
	Exact<s2amdStepMetrics> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_metrics_history(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
	if (wantRc == S2AMD_OK)
	{
		for (int k = 0; k < wantCount; ++k)
		{
			EXPECT(out.p[k].step, wantFirst + k);
		}
	}
}

static void gettersAfterStep(s2amdSolver* s, int written, int length)
{
	const int n = written < length ? written : length, first = written - n;
	s2amdStepMetrics last;
	EXPECT(s2amd_world_metrics(s, &last), S2AMD_OK);
	EXPECT(last.step, written - 1);
	EXPECT(s2amd_world_metrics(s, nullptr), S2AMD_E_INVALID);
	askHistory(s, -1, S2AMD_E_INVALID, -7, 0);
	askHistory(s, n - 1, S2AMD_E_CAPACITY, n, 0);
	askHistory(s, 0, S2AMD_E_CAPACITY, n, 0);
	askHistory(s, n, S2AMD_OK, n, first);
	askHistory(s, n + 3, S2AMD_OK, n, first);
	askHistory(s, n, S2AMD_OK, n, first); // reading never clears the ring
}

static void drive(const World& first, const World& second, bool flagsFirst, bool longRun)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	s2amdStepMetrics record;
	EXPECT(s2amd_world_set_metrics(s, 8, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_metrics(s, -1, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_metrics(s, 7, 0), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_metrics(s, 1, -3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_metrics(s, 7, 4097), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_metrics(s, 0, 0), S2AMD_OK);	   // the length is ignored with flags 0
	EXPECT(s2amd_world_set_metrics(s, 0, 99999), S2AMD_OK);
	EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE); // no resident world
	askHistory(s, 4, S2AMD_E_STATE, -7, 0);
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_metrics(s, 7, 5), S2AMD_OK); // before any world: held for the upload
		EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE);
		askHistory(s, 4, S2AMD_E_STATE, -7, 0);
	}
	const World* worlds[3] = {&first, &second, &first};
	const int lengths[3] = {5, 1, 4096};
	for (int round = 0; round < 3; ++round)
	{
		const World& w = *worlds[round];
		EXPECT(upload(s, w), S2AMD_OK);
		if (flagsFirst && round == 0)
		{
			// flags and length of before the upload hold: three steps into the ring of 5
			EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE); // no step since the upload
			askHistory(s, 0, S2AMD_OK, 0, 0);
			for (int step = 0; step < 3; ++step)
			{
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				writeRecord(s, step, 7, 5);
				gettersAfterStep(s, step + 1, 5);
			}
		}
		for (int flags = 7; flags >= 0; --flags)
		{
			for (int length : lengths)
			{
				EXPECT(s2amd_world_set_metrics(s, flags, length), S2AMD_OK); // restarts the recorder
				EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE);		 // no step since
				if (flags == 0)
				{
					askHistory(s, 4, S2AMD_E_STATE, -7, 0);
					EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
					EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE);
					askHistory(s, 4, S2AMD_E_STATE, -7, 0);
					continue;
				}
				askHistory(s, 0, S2AMD_OK, 0, 0);
				// more steps than a ring of 1 or 5 holds; the ring of 4096 is filled past its end once (`longRun`)
				const int steps = length == 4096 ? (longRun && round == 0 && flags == 7 ? 4100 : 3) : 12;
				for (int step = 0; step < steps; ++step)
				{
					EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
					writeRecord(s, step, flags, length);
					if (step < 13 || step > steps - 4)
					{
						gettersAfterStep(s, step + 1, length);
					}
				}
			}
		}
		// a restart by the upload: the flags and the length hold, the ring is empty, the next record is step 0
		EXPECT(s2amd_world_set_metrics(s, 5, 5), S2AMD_OK);
		for (int step = 0; step < 7; ++step)
		{
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			writeRecord(s, step, 5, 5);
		}
		gettersAfterStep(s, 7, 5);
		EXPECT(upload(s, *worlds[(round + 1) % 3]), S2AMD_OK);
		EXPECT(s2amd_world_metrics(s, &record), S2AMD_E_STATE);
		askHistory(s, 0, S2AMD_OK, 0, 0);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		writeRecord(s, 0, 5, 5);
		gettersAfterStep(s, 1, 5);
		EXPECT(s2amd_world_set_metrics(s, 9, 5), S2AMD_E_INVALID); // refused: the recorder goes on
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		writeRecord(s, 1, 5, 5);
		gettersAfterStep(s, 2, 5);
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0, 0, 0); // the static ground alone, no contact or joint slots: only body tiles
	World empty = makeWorld(3, 0, 0);
	empty.bodies.clear(), empty.origins.clear(), empty.shapes.clear(); // no slots at all: the gather pass has no tile
	const World small = makeWorld(40, 4, 3), big = makeWorld(700, 2300, 300); // one tile each; three, nine and two
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		drive(small, big, flagsFirst != 0, flagsFirst == 0);
		drive(big, none, flagsFirst != 0, false);
		drive(empty, small, flagsFirst != 0, false);
	}
	if (failures == 0)
	{
		printf("STEP METRICS MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
