// TEST INFRASTRUCTURE.  The host side of the sensor report (solver2d_amd/csrc/sensor_report.hip: layout, prepare, enqueue, the two setters,
// the three getters, and report_host.cpp behind them) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled
// with ASan + UBSan and linked against _build/libs2amd_hostcheck.so: the setter with good and bad lists -> every flag combination ->
// every getter with too-small, exact and ample buffers -> listCapacity 0, small and ample (the getters' rebuild path among them), and
// changed after a step (the getters must refuse) ->
// uploads with other capacities -> destroy.  Kernels never run here, so the head the offsets pass would leave (the three totals) is
// written by this program at the report state's headOffset: what is checked is that the host side touches only memory it owns -- every
// output buffer is a heap block of exactly the size passed.  Built and run by tests/test_sensor_report_host.py.
#include "report_main_common.h"

static void writeHead(s2amdSolver* s, int inside, int entered, int left)
{
	const int32_t head[4] = {inside, entered, left, 0};
	memcpy((char*)s->sensorReport.block.p + s->sensorReport.headOffset, head, sizeof(head));
	s->sensorReport.headKnown = false;
}

static s2amdSensor makeSensor(int k, int bodies)
{
	s2amdSensor q = {};
	q.count = 1 + k % 8;
	for (int i = 0; i < q.count; ++i)
	{
		q.vertices[i][0] = 0.1f * (float)i, q.vertices[i][1] = 0.05f * (float)(i * i);
	}
	q.radius = 0.25f, q.margin = k % 3 == 0 ? 0.0f : 0.1f;
	q.position[0] = 0.5f * (float)(k % 40), q.position[1] = 1.0f;
	q.rot[0] = 0.0f, q.rot[1] = 1.0f;
	q.maskBits = 0xffffffffu;
	q.body = k % 2 == 0 || bodies <= 0 ? -1 : k % bodies;
	q.flags = k % 5 == 4 ? S2AMD_SENSOR_DISABLED : k % 5 == 3 ? S2AMD_SENSOR_SKIP_STATIC : 0;
	return q;
}

static void askInside(s2amdSolver* s, int sensors, int capacity, int wantRc, int wantTotal)
{
	Exact<int32_t> offsets(sensors + 1), shapes(capacity);
	int32_t total = -7;
	EXPECT(s2amd_world_sensor_inside(s, offsets.p, shapes.p, capacity, &total), wantRc);
	EXPECT(total, wantTotal);
}

static void askEvents(s2amdSolver* s, int capacityE, int capacityL, int wantRc, int wantE, int wantL)
{
	Exact<s2amdSensorEvent> entered(capacityE), left(capacityL);
	int32_t nE = -7, nL = -7;
	EXPECT(s2amd_world_sensor_events(s, entered.p, capacityE, &nE, left.p, capacityL, &nL), wantRc);
	EXPECT(nE, wantE);
	EXPECT(nL, wantL);
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdSensorState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_sensor_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

static void gettersAfterStep(s2amdSolver* s, int flags, int sensors, int ns, int pass)
{
	// totals below, at and above what listCapacity holds; never more than sensors x shape slots
	const long long most = (long long)sensors * ns;
	const int inside = (int)std::min<long long>(most, pass == 0 ? 3 : pass == 1 ? 12 : 700);
	const int entered = inside / 2, left = inside - inside / 2;
	if (sensors > 0)
	{
		writeHead(s, inside, entered, left);
	}
	const int wantInside = sensors > 0 ? inside : 0, wantE = sensors > 0 ? entered : 0, wantL = sensors > 0 ? left : 0;
	if ((flags & S2AMD_SENSOR_REPORT_INSIDE) != 0)
	{
		askInside(s, sensors, -1, S2AMD_E_INVALID, -7);
		if (wantInside > 0)
		{
			askInside(s, sensors, wantInside - 1, S2AMD_E_CAPACITY, wantInside);
			askInside(s, sensors, 0, S2AMD_E_CAPACITY, wantInside);
		}
		askInside(s, sensors, wantInside, S2AMD_OK, wantInside);
		askInside(s, sensors, wantInside + 5, S2AMD_OK, wantInside);
	}
	else
	{
		askInside(s, sensors, 4, S2AMD_E_STATE, -7);
	}
	if ((flags & S2AMD_SENSOR_REPORT_EVENTS) != 0)
	{
		if (wantE > 0)
		{
			askEvents(s, wantE - 1, wantL, S2AMD_E_CAPACITY, wantE, wantL);
		}
		if (wantL > 0)
		{
			askEvents(s, wantE, wantL - 1, S2AMD_E_CAPACITY, wantE, wantL);
		}
		askEvents(s, wantE, wantL, S2AMD_OK, wantE, wantL);
		askEvents(s, wantE + 3, wantL + 9, S2AMD_OK, wantE, wantL);
	}
	else
	{
		askEvents(s, 4, 4, S2AMD_E_STATE, -7, -7);
	}
	if ((flags & S2AMD_SENSOR_REPORT_STATES) != 0)
	{
		if (sensors > 0)
		{
			askStates(s, sensors - 1, S2AMD_E_CAPACITY, sensors);
		}
		askStates(s, sensors, S2AMD_OK, sensors);
		askStates(s, sensors + 2, S2AMD_OK, sensors);
	}
	else
	{
		askStates(s, 4, S2AMD_E_STATE, -7);
	}
}

static void setterRefusals(s2amdSolver* s, int bodies)
{
	std::vector<s2amdSensor> list;
	for (int k = 0; k < 9; ++k)
	{
		list.push_back(makeSensor(k, bodies));
	}
	EXPECT(s2amd_world_set_sensors(s, list.data(), -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_sensors(s, nullptr, 3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_sensors(nullptr, list.data(), 3), S2AMD_E_INVALID);
	std::vector<s2amdSensor> many((size_t)S2AMD_MAX_SENSORS + 1, list[0]);
	EXPECT(s2amd_world_set_sensors(s, many.data(), S2AMD_MAX_SENSORS + 1), S2AMD_E_INVALID);
	for (int bad = 0; bad < 8; ++bad)
	{
		std::vector<s2amdSensor> wrong = list;
		s2amdSensor& q = wrong[(size_t)bad];
		switch (bad)
		{
		case 0: q.count = 0; break;
		case 1: q.count = 9; break;
		case 2: q.radius = -0.5f; break;
		case 3: q.margin = -1.0f; break;
		case 4: q.margin = INFINITY; break;
		case 5: q.vertices[0][1] = NAN; break;
		case 6: q.flags = 4; break;
		default: q.rot[0] = NAN; break;
		}
		EXPECT(s2amd_world_set_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
	if (s->worldResident)
	{
		std::vector<s2amdSensor> wrong = list;
		wrong[2].body = s->bodyCapacity;
		EXPECT(s2amd_world_set_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
}

static void drive(const World& first, const World& second, int sensors, bool flagsFirst)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	EXPECT(s2amd_world_set_sensor_report(s, 8, 0), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_sensor_report(s, -1, 0), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_sensor_report(s, 7, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_sensor_report(nullptr, 7, 0), S2AMD_E_INVALID);
	askStates(s, 4, S2AMD_E_STATE, -7); // no resident world
	askInside(s, 3, 4, S2AMD_E_STATE, -7);
	setterRefusals(s, 0);
	std::vector<s2amdSensor> list;
	for (int k = 0; k < sensors; ++k)
	{
		list.push_back(makeSensor(k, (int)first.bodies.size()));
	}
	EXPECT(s2amd_world_set_sensors(s, list.data(), sensors), S2AMD_OK); // before any world: held for the upload
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_sensor_report(s, 7, 16), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	const int capacities[3] = {0, 16, 100000};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World* w = worlds[pass];
		const int ns = (int)w->shapes.size();
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_sensor_report(s, 0, 16), S2AMD_OK);
			EXPECT(s2amd_world_set_sensor_report(s, 7, 16), S2AMD_OK); // prepares on the resident world
		}
		askStates(s, sensors, S2AMD_E_STATE, -7); // no step since the upload
		setterRefusals(s, (int)w->bodies.size());  // ... and the list that holds is still the good one
		for (int flags = 7; flags >= 0; --flags)
		{
			// every listCapacity with every flag set: the lists in the block, and rebuilt by the getters
			EXPECT(s2amd_world_set_sensor_report(s, flags, capacities[(flags + pass) % 3]), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			if (flags != 0)
			{
				gettersAfterStep(s, flags, sensors, ns, flags % 3);
			}
			else
			{
				askStates(s, sensors, S2AMD_E_STATE, -7);
				askInside(s, sensors, 4, S2AMD_E_STATE, -7);
			}
			if (flags == 7 || flags == 3)
			{
				// listCapacity changed AFTER the step, with flags 0 and with the flags kept: the last report was laid out under the old
				// value, so every getter refuses instead of reading lists at the new layout's offsets; the next step reports again;
				// flags 0 with the value unchanged leaves that report standing
				const int other = capacities[(flags + pass + 1) % 3], third = capacities[(flags + pass + 2) % 3];
				EXPECT(s2amd_world_set_sensor_report(s, 0, other), S2AMD_OK);
				askInside(s, sensors, 700, S2AMD_E_STATE, -7);
				askEvents(s, 700, 700, S2AMD_E_STATE, -7, -7);
				askStates(s, sensors, S2AMD_E_STATE, -7);
				EXPECT(s2amd_world_set_sensor_report(s, flags, other), S2AMD_OK);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, sensors, ns, (flags + 1) % 3);
				EXPECT(s2amd_world_set_sensor_report(s, flags, third), S2AMD_OK);
				askInside(s, sensors, 700, S2AMD_E_STATE, -7);
				askEvents(s, 700, 700, S2AMD_E_STATE, -7, -7);
				askStates(s, sensors, S2AMD_E_STATE, -7);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, sensors, ns, (flags + 2) % 3);
				EXPECT(s2amd_world_set_sensor_report(s, 0, third), S2AMD_OK);
				gettersAfterStep(s, flags, sensors, ns, (flags + 2) % 3);
			}
			if (flags == 4)
			{
				// the list replaced between steps (the same sensors in reverse), and cleared and set again: the last report is void
				std::vector<s2amdSensor> reversed(list.rbegin(), list.rend());
				for (s2amdSensor& q : reversed)
				{
					q.body = q.body >= (int)w->bodies.size() ? -1 : q.body;
				}
				EXPECT(s2amd_world_set_sensors(s, reversed.data(), sensors), S2AMD_OK);
				askStates(s, sensors, S2AMD_E_STATE, -7);
				EXPECT(s2amd_world_set_sensors(s, nullptr, 0), S2AMD_OK);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				askStates(s, 0, S2AMD_OK, 0);
				EXPECT(s2amd_world_set_sensors(s, reversed.data(), sensors), S2AMD_OK);
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
	const int counts[4] = {0, 1, 257, S2AMD_MAX_SENSORS};
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		for (int sensors : counts)
		{
			drive(small, big, sensors, flagsFirst != 0);
			drive(big, none, sensors, flagsFirst != 0);
			drive(empty, small, sensors, flagsFirst != 0);
		}
	}
	if (failures == 0)
	{
		printf("SENSOR REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
