// TEST INFRASTRUCTURE.  The host side of s2amd_world_move_shapes (solver2d_amd/csrc/mover_query.hip on query_host.h's queryRounds) on the
// stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and linked against
// _build/libs2amd_hostcheck.so, in the manner of query_main.cpp: every argument refusal and the call without a world -> a world without
// shape slots, count == 0 and count 3 -> a world of two shape tiles: every rule of the validation on the first and on the last record,
// 1, 128, 129, 256 and 600 movers with and without a plane array, one and eight rounds, the batch limit -> a smaller world in the block
// the larger one left -> destroy.  Every caller buffer is a heap block of exactly the size passed, filled with 0xf9 bytes; after every
// call the program prints "RC <code> <s2amd_last_error() when the code is not 0>" and one line that names the call and what became of
// its outputs.  Kernels never run here and the program zeroes the queries' device block before a call: what is checked is that the host
// side touches only memory it owns, the return codes with their texts, the size of the device block, and -- with
// S2_HOSTCHECK_TRACE_CALLS set -- the launches, copies, memsets and waits of every call, which hip_stub.cpp prints between the lines of
// this program.  tests/hostcheck/mover_transcript.txt is that output; tests/test_mover_hostcheck.py builds and runs the program and
// compares.
#include "report_main_common.h"

#include <cstring>

static s2amdSolver* solver = nullptr;
static const bool tracing = getenv("S2_HOSTCHECK_TRACE_CALLS") != nullptr;
static size_t blockBytes = 0;

static void traceOff()
{
	if (tracing)
	{
		unsetenv("S2_HOSTCHECK_TRACE_CALLS");
	}
}

static void traceOn()
{
	if (tracing)
	{
		setenv("S2_HOSTCHECK_TRACE_CALLS", "1", 1);
	}
}

static void place(const char* what, const World& w)
{
	printf("== %s: %d bodies, %d shape slots\n", what, (int)w.bodies.size(), (int)w.shapes.size());
	traceOff();
	EXPECT(upload(solver, w), S2AMD_OK);
	traceOn();
}

static void prime()
{
	if (solver->dQuery.p != nullptr)
	{
		memset(solver->dQuery.p, 0, solver->dQuery.bytes);
	}
}

static void answered(int code)
{
	if (code == 0)
	{
		printf("RC 0\n");
	}
	else
	{
		printf("RC %d %s\n", code, s2amd_last_error());
	}
	if (solver != nullptr && solver->dQuery.bytes != blockBytes)
	{
		blockBytes = solver->dQuery.bytes;
		printf("BLOCK %zu\n", blockBytes);
	}
}

// a heap block of exactly n elements, every byte 0xf9
template <typename T> struct Filled : Exact<T>
{
	int n;
	explicit Filled(int count) : Exact<T>(count), n(count)
	{
		if (n > 0)
		{
			memset((void*)this->p, 0xf9, (size_t)n * sizeof(T));
		}
	}
	const char* state() const
	{
		if (n <= 0)
		{
			return "none";
		}
		const unsigned char* b = (const unsigned char*)this->p;
		size_t kept = 0, zero = 0;
		const size_t bytes = (size_t)n * sizeof(T);
		for (size_t i = 0; i < bytes; ++i)
		{
			kept += b[i] == 0xf9, zero += b[i] == 0;
		}
		return kept == bytes ? "kept" : zero == bytes ? "zero" : "mixed";
	}
};

static void makeMover(int k, s2amdMover* m, int iterations)
{
	*m = {};
	m->count = 1 + k % 8;
	for (int i = 0; i < m->count; ++i)
	{
		m->vertices[i][0] = 0.1f * (float)i, m->vertices[i][1] = 0.05f * (float)(i * i);
	}
	m->radius = 0.25f;
	m->position[0] = 0.5f * (float)(k % 40), m->position[1] = 9.0f;
	m->rot[0] = 0.0f, m->rot[1] = 1.0f;
	m->translation[0] = 0.25f, m->translation[1] = -10.0f;
	m->maxIterations = iterations, m->maskBits = 0xffffffffu;
	m->ignoreBody = k % 3 == 0 ? -1 : k % 3 == 1 ? 0 : -1000; // (any negative value: none)
	m->flags = k % 2 == 0 ? 0u : (uint32_t)S2AMD_MOVER_STATIC_ONLY;
}

struct Movers : Exact<s2amdMover>
{
	Movers(int count, int iterations) : Exact<s2amdMover>(count)
	{
		for (int k = 0; k < count; ++k)
		{
			makeMover(k, this->p + k, iterations);
		}
	}
};

// every rule of the validation
struct Rule
{
	const char* name;
	void (*spoil)(s2amdMover*);
};
static int bodySlots = 0;
static const Rule rules[] = {
	{"count 0", [](s2amdMover* m) { m->count = 0; }},
	{"count 9", [](s2amdMover* m) { m->count = 9; }},
	{"a NaN vertex", [](s2amdMover* m) { m->vertices[0][1] = NAN; }},
	{"a negative radius", [](s2amdMover* m) { m->radius = -0.25f; }},
	{"an infinite radius", [](s2amdMover* m) { m->radius = INFINITY; }},
	{"an infinite position", [](s2amdMover* m) { m->position[0] = INFINITY; }},
	{"a NaN rot", [](s2amdMover* m) { m->rot[1] = NAN; }},
	{"a NaN translation", [](s2amdMover* m) { m->translation[0] = NAN; }},
	{"an infinite translation", [](s2amdMover* m) { m->translation[1] = -INFINITY; }},
	{"maxIterations 0", [](s2amdMover* m) { m->maxIterations = 0; }},
	{"maxIterations 9", [](s2amdMover* m) { m->maxIterations = 9; }},
	{"maxIterations -1", [](s2amdMover* m) { m->maxIterations = -1; }},
	{"flag bit 1", [](s2amdMover* m) { m->flags = 2u; }},
	{"flag bit 31", [](s2amdMover* m) { m->flags = 0x80000001u; }},
	{"reserved[0]", [](s2amdMover* m) { m->reserved[0] = 1; }},
	{"reserved[3]", [](s2amdMover* m) { m->reserved[3] = -1; }},
	{"ignoreBody == body slots", [](s2amdMover* m) { m->ignoreBody = bodySlots; }},
	{"ignoreBody beyond", [](s2amdMover* m) { m->ignoreBody = 0x7fffffff; }},
};

static void ask(int count, int iterations, bool withPlanes, const Rule* rule = nullptr, int bad = -1)
{
	Movers movers(count, iterations);
	if (rule != nullptr)
	{
		rule->spoil(movers.p + bad);
	}
	Filled<s2amdMoverResult> results(count);
	Filled<s2amdMoverPlane> planes(withPlanes ? count * S2AMD_MOVER_MAX_ITERATIONS : 0);
	prime();
	answered(s2amd_world_move_shapes(solver, movers.p, count, results.p, planes.p));
	printf("-- move_shapes count %d iterations %d%s%s%s: results %s planes %s\n", count, iterations, rule ? ", " : "", rule ? rule->name : "",
		   rule == nullptr ? "" : bad == 0 ? " in record 0" : " in the last record", results.state(), planes.state());
}

static void refusals()
{
	printf("-- move_shapes: a null solver, a negative count, null movers, null results\n");
	Movers movers(3, 4);
	Filled<s2amdMoverResult> results(3);
	Filled<s2amdMoverPlane> planes(3 * S2AMD_MOVER_MAX_ITERATIONS);
	answered(s2amd_world_move_shapes(nullptr, movers.p, 3, results.p, planes.p));
	answered(s2amd_world_move_shapes(solver, movers.p, -1, results.p, planes.p));
	answered(s2amd_world_move_shapes(solver, nullptr, 3, results.p, planes.p));
	answered(s2amd_world_move_shapes(solver, movers.p, 3, nullptr, planes.p));
	printf("OUT results %s planes %s\n", results.state(), planes.state());
}

static void batches(bool few)
{
	const int counts[5] = {1, 128, 129, 256, 600};
	for (int count : counts)
	{
		if (!few || count == 600)
		{
			ask(count, 4, true);
			ask(count, 4, false);
		}
	}
	if (!few)
	{
		ask(5, 1, true);
		ask(5, 8, true);
		// the rounds are those of the mover that asks for most
		Movers movers(3, 2);
		movers.p[1].maxIterations = 7;
		Filled<s2amdMoverResult> results(3);
		prime();
		answered(s2amd_world_move_shapes(solver, movers.p, 3, results.p, nullptr));
		printf("-- move_shapes count 3 iterations 2, 7, 2: results %s\n", results.state());
	}
}

int main()
{
	traceOff();
	EXPECT(s2amd_create(0, &solver), S2AMD_OK);
	traceOn();
	if (!solver)
	{
		return 1;
	}
	printf("== no resident world\n");
	refusals();
	ask(3, 4, true);
	ask(0, 4, false);

	World empty = makeWorld(3);
	empty.shapes.clear();
	place("a world without shape slots", empty);
	ask(0, 4, true);
	ask(0, 4, false);
	{
		printf("-- move_shapes count 0 with null arrays\n");
		answered(s2amd_world_move_shapes(solver, nullptr, 0, nullptr, nullptr));
	}
	ask(3, 4, true);
	ask(3, 4, false);

	const World two = makeWorld(300);
	bodySlots = (int)two.bodies.size();
	place("a world of two shape tiles", two);
	refusals();
	for (const Rule& rule : rules)
	{
		ask(5, 4, true, &rule, 0);
		ask(5, 4, false, &rule, 4);
	}
	{
		// the largest body slot is taken
		Movers movers(2, 4);
		movers.p[1].ignoreBody = bodySlots - 1;
		Filled<s2amdMoverResult> results(2);
		prime();
		answered(s2amd_world_move_shapes(solver, movers.p, 2, results.p, nullptr));
		printf("-- move_shapes count 2, ignoreBody the last body slot: results %s\n", results.state());
	}
	batches(false);
	printf("== the same world, the batch limit\n");
	{
		printf("-- move_shapes count %d\n", 65535 * 256 + 1);
		Movers movers(1, 4);
		Filled<s2amdMoverResult> results(1);
		answered(s2amd_world_move_shapes(solver, movers.p, 65535 * 256 + 1, results.p, nullptr));
		printf("OUT results %s\n", results.state());
	}

	const World small = makeWorld(40);
	bodySlots = (int)small.bodies.size();
	place("a smaller world, in the block the larger one left", small);
	batches(true);
	ask(5, 4, true, &rules[16], 4); // (ignoreBody is measured against this world's body slots)

	traceOff();
	s2amd_destroy(solver);
	if (failures == 0)
	{
		printf("MOVER MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
