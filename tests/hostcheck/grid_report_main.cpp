// TEST INFRASTRUCTURE.  The host side of the grid report (solver2d_amd/csrc/grid_report.hip: layout, tile table, prepare, enqueue, the
// two setters, the five getters, and report_host.cpp behind them) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone
// program compiled with ASan + UBSan and linked against _build/libs2amd_hostcheck.so: the setter with good and bad lists -> every flag
// combination 0..15 -> every getter and the export with too-small, exact and ample buffers -> the list replaced and cleared between
// steps -> uploads with other capacities, a world without shape slots among them -> destroy, for 0, 1, 257 and 1,024 grids, one list at
// exactly S2AMD_MAX_GRID_CELLS and one a cell over.  Kernels never run here: what is checked is that the host side touches only memory
// it owns -- every output buffer is a heap block of exactly the size passed.  Built and run by tests/test_grid_report_host.py.
#include "report_main_common.h"

static s2amdGridSensor makeGrid(int k, int bodies)
{
	s2amdGridSensor q = {};
	q.position[0] = 0.5f * (float)(k % 40), q.position[1] = 2.0f;
	q.rot[0] = 0.0f, q.rot[1] = 1.0f;
	q.cellSize = 0.25f;
	q.width = 1 + k % 9, q.height = 1 + (k / 3) % 17;
	q.maskBits = 0xffffffffu;
	q.body = k % 2 == 0 || bodies <= 0 ? -1 : k % bodies;
	q.flags = k % 5 == 4 ? S2AMD_GRID_SENSOR_DISABLED : k % 5 == 3 ? S2AMD_GRID_SENSOR_SKIP_STATIC : 0;
	q.pad[0] = 0x7fffffff, q.pad[5] = -1; // (not the library's to trust)
	return q;
}

static int cellsOf(const std::vector<s2amdGridSensor>& list)
{
	int cells = 0;
	for (const s2amdGridSensor& q : list)
	{
		cells += q.width * q.height;
	}
	return cells;
}

template <typename T> static void askCells(int (*fn)(s2amdSolver*, T*, int32_t, int32_t*), s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<T> out(capacity);
	int32_t count = -7;
	EXPECT(fn(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

// (device memory of the stand-in runtime is host memory: the export's destination is an exact heap block as well)
static void askExport(s2amdSolver* s, int capacity, int wantRc)
{
	Exact<float> out(capacity);
	EXPECT(s2amd_world_export_grid_occupancy(s, out.p, capacity), wantRc);
}

template <typename T> static void askAll(int (*fn)(s2amdSolver*, T*, int32_t, int32_t*), s2amdSolver* s, bool on, int n)
{
	if (!on)
	{
		askCells<T>(fn, s, n + 1, S2AMD_E_STATE, -7);
		return;
	}
	askCells<T>(fn, s, -1, S2AMD_E_INVALID, -7);
	if (n > 0)
	{
		askCells<T>(fn, s, n - 1, S2AMD_E_CAPACITY, n);
		askCells<T>(fn, s, 0, S2AMD_E_CAPACITY, n);
	}
	askCells<T>(fn, s, n, S2AMD_OK, n);
	askCells<T>(fn, s, n + 3, S2AMD_OK, n);
}

static void gettersAfterStep(s2amdSolver* s, int flags, int grids, int cells)
{
	askAll<uint32_t>(s2amd_world_grid_categories, s, (flags & S2AMD_GRID_REPORT_CATEGORIES) != 0, cells);
	askAll<int32_t>(s2amd_world_grid_shapes, s, (flags & S2AMD_GRID_REPORT_SHAPES) != 0, cells);
	askAll<float>(s2amd_world_grid_occupancy, s, (flags & S2AMD_GRID_REPORT_OCCUPANCY) != 0, cells);
	askAll<s2amdGridState>(s2amd_world_grid_states, s, (flags & S2AMD_GRID_REPORT_STATES) != 0, grids);
	if ((flags & S2AMD_GRID_REPORT_OCCUPANCY) != 0)
	{
		askExport(s, -1, S2AMD_E_INVALID);
		if (cells > 0)
		{
			askExport(s, cells - 1, S2AMD_E_CAPACITY);
		}
		askExport(s, cells, S2AMD_OK);
		askExport(s, cells + 5, S2AMD_OK);
	}
	else
	{
		askExport(s, cells + 1, S2AMD_E_STATE);
	}
}

static void gettersRefuse(s2amdSolver* s, int grids, int cells)
{
	gettersAfterStep(s, 0, grids, cells);
}

static void setterRefusals(s2amdSolver* s, int bodies)
{
	std::vector<s2amdGridSensor> list;
	for (int k = 0; k < 9; ++k)
	{
		list.push_back(makeGrid(k, bodies));
	}
	EXPECT(s2amd_world_set_grid_sensors(s, list.data(), -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_grid_sensors(s, nullptr, 3), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_grid_sensors(nullptr, list.data(), 3), S2AMD_E_INVALID);
	std::vector<s2amdGridSensor> many((size_t)S2AMD_MAX_GRID_SENSORS + 1, list[0]);
	EXPECT(s2amd_world_set_grid_sensors(s, many.data(), S2AMD_MAX_GRID_SENSORS + 1), S2AMD_E_INVALID);
	for (int bad = 0; bad < 12; ++bad)
	{
		std::vector<s2amdGridSensor> wrong = list;
		s2amdGridSensor& q = wrong[(size_t)(bad % 9)];
		switch (bad)
		{
		case 0: q.width = 0; break;
		case 1: q.width = S2AMD_MAX_GRID_SIDE + 1; break;
		case 2: q.height = 0; break;
		case 3: q.height = -4; break;
		case 4: q.height = S2AMD_MAX_GRID_SIDE + 1; break;
		case 5: q.cellSize = 0.0f; break;
		case 6: q.cellSize = -1.0f; break;
		case 7: q.cellSize = NAN; break;
		case 8: q.cellSize = INFINITY; break;
		case 9: q.position[1] = INFINITY; break;
		case 10: q.rot[0] = NAN; break;
		default: q.flags = 4; break;
		}
		EXPECT(s2amd_world_set_grid_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
	if (s->worldResident)
	{
		std::vector<s2amdGridSensor> wrong = list;
		wrong[2].body = s->bodyCapacity;
		EXPECT(s2amd_world_set_grid_sensors(s, wrong.data(), (int32_t)wrong.size()), S2AMD_E_INVALID);
	}
}

static void drive(const World& first, const World& second, int grids, bool flagsFirst)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	EXPECT(s2amd_world_set_grid_report(s, 16), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_grid_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_grid_report(nullptr, 15), S2AMD_E_INVALID);
	gettersRefuse(s, 3, 3); // no resident world
	setterRefusals(s, 0);
	std::vector<s2amdGridSensor> list;
	for (int k = 0; k < grids; ++k)
	{
		list.push_back(makeGrid(k, (int)first.bodies.size()));
	}
	const int cells = cellsOf(list);
	EXPECT(s2amd_world_set_grid_sensors(s, list.data(), grids), S2AMD_OK); // before any world: held for the upload
	EXPECT((int)s->hGridSensors.size(), grids);
	EXPECT((int)s->gridCells, cells);
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_grid_report(s, 15), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		const World* w = worlds[pass];
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_grid_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_grid_report(s, 15), S2AMD_OK); // prepares on the resident world
		}
		gettersRefuse(s, grids, cells);			  // no step since the upload
		setterRefusals(s, (int)w->bodies.size()); // ... and the list that holds is still the good one
		EXPECT((int)s->hGridSensors.size(), grids);
		for (int flags = 15; flags >= 0; --flags)
		{
			EXPECT(s2amd_world_set_grid_report(s, flags), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			gettersAfterStep(s, flags, grids, cells);
			if (flags == 4 || flags == 15)
			{
				// the list replaced between steps (the same grids in reverse), and cleared and set again: the last report is void
				std::vector<s2amdGridSensor> reversed(list.rbegin(), list.rend());
				for (s2amdGridSensor& q : reversed)
				{
					q.body = q.body >= (int)w->bodies.size() ? -1 : q.body;
				}
				EXPECT(s2amd_world_set_grid_sensors(s, reversed.data(), grids), S2AMD_OK);
				gettersRefuse(s, grids, cells);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, grids, cells);
				EXPECT(s2amd_world_set_grid_sensors(s, nullptr, 0), S2AMD_OK);
				gettersRefuse(s, 0, 0);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				gettersAfterStep(s, flags, 0, 0);
				EXPECT(s2amd_world_set_grid_sensors(s, reversed.data(), grids), S2AMD_OK);
				if (grids <= 300)
				{
					// a list of more than twice the grids and cells, whose block cannot be had (larger than any before it: the block
					// never shrinks): the setter fails with the allocation's message, and the list before stands -- the grids, their
					// tiles and their cell count -- with its block, prepared again: the next step reports it
					const size_t tilesBefore = s->hGridTiles.size();
					std::vector<s2amdGridSensor> longer;
					for (int k = 0; k < 2 * grids + 64; ++k)
					{
						longer.push_back(makeGrid(k, 0));
					}
					setenv("S2_HOSTCHECK_FAIL_MALLOC", "1", 1);
					EXPECT(s2amd_world_set_grid_sensors(s, longer.data(), (int32_t)longer.size()), S2AMD_E_DEVICE);
					unsetenv("S2_HOSTCHECK_FAIL_MALLOC");
					EXPECT(strstr(s2amd_last_error(), "hipMalloc") != nullptr, 1);
					EXPECT((int)s->hGridSensors.size(), grids);
					EXPECT((int)s->gridCells, cells);
					EXPECT((int)s->hGridTiles.size(), (int)tilesBefore);
					gettersRefuse(s, grids, cells);
					EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
					gettersAfterStep(s, flags, grids, cells);
				}
			}
		}
	}
	s2amd_destroy(s);
}

// one list at exactly S2AMD_MAX_GRID_CELLS (16 grids of 256 x 256), and one a cell over: refused, the full list stands
static void cellLimit(const World& w)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	s2amdGridSensor big = makeGrid(0, 0);
	big.width = big.height = S2AMD_MAX_GRID_SIDE;
	std::vector<s2amdGridSensor> full(16, big);
	EXPECT(upload(s, w), S2AMD_OK);
	EXPECT(s2amd_world_set_grid_report(s, 15), S2AMD_OK);
	EXPECT(s2amd_world_set_grid_sensors(s, full.data(), 16), S2AMD_OK);
	std::vector<s2amdGridSensor> over = full;
	s2amdGridSensor one = makeGrid(0, 0);
	one.width = one.height = 1;
	over.push_back(one);
	EXPECT(s2amd_world_set_grid_sensors(s, over.data(), 17), S2AMD_E_INVALID);
	EXPECT((int)s->gridCells, S2AMD_MAX_GRID_CELLS);
	EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
	gettersAfterStep(s, 15, 16, S2AMD_MAX_GRID_CELLS);
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0);
	World empty = makeWorld(3);
	empty.shapes.clear(); // no shape slots at all: no candidates pass is launched
	const World small = makeWorld(40), big = makeWorld(700); // one tile; more than three
	const int counts[4] = {0, 1, 257, S2AMD_MAX_GRID_SENSORS};
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		for (int grids : counts)
		{
			drive(small, big, grids, flagsFirst != 0);
			drive(big, none, grids, flagsFirst != 0);
			drive(empty, small, grids, flagsFirst != 0);
		}
	}
	cellLimit(small);
	if (failures == 0)
	{
		printf("GRID REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
