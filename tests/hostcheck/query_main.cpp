// TEST INFRASTRUCTURE.  The host side of the eight queries on the resident world (solver2d_amd/csrc: scene_query.hip, proximity_query.hip,
// contact_query.hip, shape_cast.hip) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan
// and linked against _build/libs2amd_hostcheck.so: every argument refusal and the calls without a world -> a world without shape slots,
// count == 0 and count 3 -> a world of two shape tiles: one invalid record first and last, 1, 256, 257 and 600 queries with ample room,
// 257 with a capacity of 0 and of 1, totals beyond the capacity, the batch limits -> queries x slots beyond 2^31 on a wide world ->
// calls on a smaller world, in the device block the larger ones left -> destroy.  Every caller
// buffer is a heap block of exactly the size passed, filled with 0xf9 bytes (a total with -7), and after every call the program prints
// "RC <code> <s2amd_last_error() when the code is not 0>" and one line that names the call and what became of its outputs.  Kernels never run here and the program zeroes
// the queries' device block before a call, so every total is 0 (one section fills it with ones instead, for S2AMD_E_CAPACITY): what is
// checked is that the host side touches only memory it owns, the return codes with their texts, the size of the device block, and --
// with S2_HOSTCHECK_TRACE_CALLS set -- the launches, copies, memsets and waits of every call, which hip_stub.cpp prints between the lines
// of this program.  tests/hostcheck/query_transcript.txt is that output; tests/test_query_host.py builds and runs the
// program and compares.  (Uploads, create and destroy run with the trace off: the transcript is the queries' alone.)
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

// Kernels do not run, so what a call copies back is what its device block held: all zero (every total 0, the usual case here), or every
// byte 1 (every total 16,843,009: more than any capacity, so the list calls answer S2AMD_E_CAPACITY)
static int blockByte = 0;

static void prime()
{
	if (solver->dQuery.p != nullptr)
	{
		memset(solver->dQuery.p, blockByte, solver->dQuery.bytes);
	}
}

// ... and the device block of the queries, whenever it has grown
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

// ---- one valid record of every kind, and what makes it invalid ----
static void makeRecord(int k, s2amdRay* r)
{
	*r = {};
	r->p1[0] = 0.5f * (float)(k % 40), r->p1[1] = 9.0f;
	r->p2[0] = r->p1[0] + 0.25f, r->p2[1] = -1.0f;
	r->maxFraction = 1.0f, r->maskBits = 0xffffffffu;
}
static void spoil(s2amdRay* r) { r->maxFraction = 100000.0f; }

static void makeRecord(int k, s2amdPointProbe* p)
{
	*p = {};
	p->p[0] = 0.5f * (float)(k % 40), p->p[1] = 1.0f, p->maskBits = 0xffffffffu;
}

static void makeRecord(int k, s2amdBoxQuery* b)
{
	*b = {};
	b->box[0] = 0.5f * (float)(k % 40), b->box[1] = 0.0f, b->box[2] = b->box[0] + 1.0f, b->box[3] = 4.0f, b->maskBits = 0xffffffffu;
}

// (point probes and box queries are not validated)
static void spoil(s2amdPointProbe*) {}
static void spoil(s2amdBoxQuery*) {}

static void makeRecord(int k, s2amdProximityQuery* q)
{
	*q = {};
	q->count = 1 + k % 8;
	for (int i = 0; i < q->count; ++i)
	{
		q->vertices[i][0] = 0.1f * (float)i, q->vertices[i][1] = 0.05f * (float)(i * i);
	}
	q->radius = 0.25f, q->maxDistance = k % 3 == 0 ? 0.0f : 2.0f;
	q->position[0] = 0.5f * (float)(k % 40), q->position[1] = 1.0f;
	q->rot[0] = 0.0f, q->rot[1] = 1.0f;
	q->maskBits = 0xffffffffu;
}
static void spoil(s2amdProximityQuery* q) { q->count = 9; }

static void makeRecord(int k, s2amdContactQuery* q)
{
	*q = {};
	const int types[4] = {S2AMD_SHAPE_CAPSULE, S2AMD_SHAPE_CIRCLE, S2AMD_SHAPE_POLYGON, S2AMD_SHAPE_SEGMENT};
	q->type = types[k % 4];
	q->count = q->type == S2AMD_SHAPE_POLYGON ? 4 : 0;
	const float v[4][2] = {{-0.5f, -0.25f}, {0.5f, -0.25f}, {0.5f, 0.25f}, {-0.5f, 0.25f}};
	const float n[4][2] = {{0.0f, -1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}};
	for (int i = 0; i < 4; ++i)
	{
		q->vertices[i][0] = v[i][0], q->vertices[i][1] = v[i][1];
		q->normals[i][0] = n[i][0], q->normals[i][1] = n[i][1];
	}
	q->radius = 0.125f;
	q->position[0] = 0.5f * (float)(k % 40), q->position[1] = 1.0f;
	q->rot[0] = 0.0f, q->rot[1] = 1.0f;
	q->maskBits = 0xffffffffu;
}
static void spoil(s2amdContactQuery* q) { q->type = S2AMD_SHAPE_FREE; }

static void makeRecord(int k, s2amdShapeCast* c)
{
	*c = {};
	c->count = 1 + k % 8;
	for (int i = 0; i < c->count; ++i)
	{
		c->vertices[i][0] = 0.1f * (float)i, c->vertices[i][1] = 0.05f * (float)(i * i);
	}
	c->radius = 0.25f;
	c->position[0] = 0.5f * (float)(k % 40), c->position[1] = 9.0f;
	c->rot[0] = 0.0f, c->rot[1] = 1.0f;
	c->translation[0] = 0.25f, c->translation[1] = -10.0f;
	c->maxFraction = 1.0f, c->maskBits = 0xffffffffu;
}
static void spoil(s2amdShapeCast* c) { c->radius = -1.0f; }

template <typename Q> struct Records : Exact<Q>
{
	explicit Records(int count) : Exact<Q>(count)
	{
		for (int k = 0; k < count; ++k)
		{
			makeRecord(k, this->p + k);
		}
	}
};

// ---- the two call shapes ----
// one answer per query
template <typename Q, typename H> struct BestCall
{
	const char* name;
	int (*fn)(s2amdSolver*, const Q*, int32_t, H*);

	void ask(int count, int bad = -1) const
	{
		Records<Q> records(count);
		if (bad >= 0)
		{
			spoil(records.p + bad);
		}
		Filled<H> hits(count);
		prime();
		answered(fn(solver, records.p, count, hits.p));
		printf("-- %s count %d%s: hits %s\n", name, count, bad < 0 ? "" : bad == 0 ? ", record 0 invalid" : ", the last record invalid", hits.state());
	}

	void refusals() const
	{
		printf("-- %s: a null solver, a negative count, null records, null hits\n", name);
		Records<Q> records(3);
		Filled<H> hits(3);
		answered(fn(nullptr, records.p, 3, hits.p));
		answered(fn(solver, records.p, -1, hits.p));
		answered(fn(solver, nullptr, 3, hits.p));
		answered(fn(solver, records.p, 3, nullptr));
		printf("OUT hits %s\n", hits.state());
	}

	// more records than a call takes: refused before a record is read (the one buffer that is not of the size passed)
	void tooMany() const
	{
		printf("-- %s count %d\n", name, 65535 * 256 + 1);
		Records<Q> records(1);
		Filled<H> hits(1);
		answered(fn(solver, records.p, 65535 * 256 + 1, hits.p));
		printf("OUT hits %s\n", hits.state());
	}
};

// a list per query: offsets[count + 1], `capacity` payload entries (shapes in range: and, when asked for, as many distances), the total
template <typename Q, typename P> struct ListCall
{
	const char* name;
	int (*plain)(s2amdSolver*, const Q*, int32_t, int32_t*, P*, int32_t, int32_t*);
	int (*parallel)(s2amdSolver*, const Q*, int32_t, int32_t*, P*, float*, int32_t, int32_t*);
	bool distances;

	int call(s2amdSolver* s, const Q* records, int32_t count, int32_t* offsets, P* payload, float* beside, int32_t capacity, int32_t* total) const
	{
		return plain != nullptr ? plain(s, records, count, offsets, payload, capacity, total) : parallel(s, records, count, offsets, payload, beside, capacity, total);
	}

	void ask(int count, int capacity, int bad = -1) const
	{
		Records<Q> records(count);
		if (bad >= 0)
		{
			spoil(records.p + bad);
		}
		Filled<int32_t> offsets(count > 0 ? count + 1 : 0);
		Filled<P> payload(capacity);
		Filled<float> beside(distances ? capacity : 0);
		int32_t total = -7;
		prime();
		answered(call(solver, records.p, count, offsets.p, payload.p, beside.p, capacity, &total));
		printf("-- %s count %d capacity %d%s: offsets %s payload %s distances %s total %d\n", name, count, capacity,
			   bad < 0 ? "" : bad == 0 ? ", record 0 invalid" : ", the last record invalid", offsets.state(), payload.state(), beside.state(), total);
	}

	void refusals() const
	{
		printf("-- %s: a null solver, a negative count, null records, null offsets, a negative capacity, a null total, a null payload\n", name);
		Records<Q> records(3);
		Filled<int32_t> offsets(4);
		Filled<P> payload(5);
		Filled<float> beside(distances ? 5 : 0);
		int32_t total = -7;
		answered(call(nullptr, records.p, 3, offsets.p, payload.p, beside.p, 5, &total));
		answered(call(solver, records.p, -1, offsets.p, payload.p, beside.p, 5, &total));
		answered(call(solver, nullptr, 3, offsets.p, payload.p, beside.p, 5, &total));
		answered(call(solver, records.p, 3, nullptr, payload.p, beside.p, 5, &total));
		answered(call(solver, records.p, 3, offsets.p, payload.p, beside.p, -1, &total));
		answered(call(solver, records.p, 3, offsets.p, payload.p, beside.p, 5, nullptr));
		answered(call(solver, records.p, 3, offsets.p, nullptr, beside.p, 5, &total));
		printf("OUT offsets %s payload %s distances %s total %d\n", offsets.state(), payload.state(), beside.state(), total);
	}

	// more records than a call takes: refused before a record is read (the one buffer that is not of the size passed)
	void tooMany() const
	{
		printf("-- %s count %d\n", name, 65535 * 256 + 1);
		Records<Q> records(1);
		Filled<int32_t> offsets(1);
		int32_t total = -7;
		answered(call(solver, records.p, 65535 * 256 + 1, offsets.p, nullptr, nullptr, 0, &total));
		printf("OUT offsets %s total %d\n", offsets.state(), total);
	}
};

static const BestCall<s2amdRay, s2amdRayHit> rayCast = {"ray_cast", s2amd_world_ray_cast};
static const BestCall<s2amdProximityQuery, s2amdProximityHit> closestShape = {"closest_shape", s2amd_world_closest_shape};
static const BestCall<s2amdContactQuery, s2amdContactHit> deepestContact = {"deepest_contact", s2amd_world_deepest_contact};
static const BestCall<s2amdShapeCast, s2amdShapeCastHit> castShape = {"cast_shape", s2amd_world_cast_shape};
static const ListCall<s2amdPointProbe, int32_t> pointProbe = {"point_probe", s2amd_world_point_probe, nullptr, false};
static const ListCall<s2amdBoxQuery, int32_t> queryBoxes = {"query_boxes", s2amd_world_query_boxes, nullptr, false};
static const ListCall<s2amdProximityQuery, int32_t> shapesInRange = {"shapes_in_range", nullptr, s2amd_world_shapes_in_range, false};
static const ListCall<s2amdProximityQuery, int32_t> shapesInRangeDistances = {"shapes_in_range with distances", nullptr, s2amd_world_shapes_in_range, true};
static const ListCall<s2amdContactQuery, s2amdContactHit> collideShape = {"collide_shape", s2amd_world_collide_shape, nullptr, false};
static const ListCall<s2amdShapeCast, s2amdShapeCastHit> castShapeAll = {"cast_shape_all", s2amd_world_cast_shape_all, nullptr, false};

static void refusals()
{
	rayCast.refusals(), closestShape.refusals(), deepestContact.refusals(), castShape.refusals();
	pointProbe.refusals(), queryBoxes.refusals(), shapesInRange.refusals(), shapesInRangeDistances.refusals(), collideShape.refusals(), castShapeAll.refusals();
}

static void askBest(int count)
{
	rayCast.ask(count), closestShape.ask(count), deepestContact.ask(count), castShape.ask(count);
}

static void askLists(int count, int capacity)
{
	pointProbe.ask(count, capacity), queryBoxes.ask(count, capacity), shapesInRange.ask(count, capacity), shapesInRangeDistances.ask(count, capacity);
	collideShape.ask(count, capacity), castShapeAll.ask(count, capacity);
}

static void askAll(int count, int capacity)
{
	askBest(count);
	askLists(count, capacity);
}

// the four validated kinds, through both of their calls
static void invalidRecords(int count)
{
	for (int bad = 0; bad < count; bad += std::max(count - 1, 1))
	{
		rayCast.ask(count, bad), closestShape.ask(count, bad), deepestContact.ask(count, bad), castShape.ask(count, bad);
		shapesInRange.ask(count, 8, bad), shapesInRangeDistances.ask(count, 8, bad), collideShape.ask(count, 8, bad), castShapeAll.ask(count, 8, bad);
	}
}

// 1 query, a full chunk, one more, and three chunks (`few`: the last alone), each with room that is more than 1 x shape slots
// but less than 256 x shape slots -- both sides of the `entries` clamp; then (not with `few`) no room and room for one entry
static void batches(bool few)
{
	const int counts[4] = {1, 256, 257, 600};
	for (int count : counts)
	{
		if (!few || count == 600)
		{
			askBest(count);
			askLists(count, 1000);
		}
	}
	if (!few)
	{
		askLists(257, 0);
		askLists(257, 1);
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
	askAll(3, 4);

	World empty = makeWorld(3);
	empty.shapes.clear();
	place("a world without shape slots", empty);
	askAll(0, 4);
	askAll(3, 4);

	const World two = makeWorld(300);
	place("a world of two shape tiles", two);
	invalidRecords(5);
	batches(false);
	printf("== the same world, totals beyond every capacity\n");
	blockByte = 1;
	askLists(257, 1000);
	blockByte = 0;
	printf("== the same world, the batch limit\n");
	rayCast.tooMany(), closestShape.tooMany(), deepestContact.tooMany(), castShape.tooMany();
	pointProbe.tooMany(), queryBoxes.tooMany(), shapesInRange.tooMany(), collideShape.tooMany(), castShapeAll.tooMany();

	// queries x shape slots beyond 2^31, with records that are all there: 70,001 slots x 30,679 queries
	const World wide = makeWorld(60000);
	place("a world of 274 shape tiles", wide);
	const int beyond = (int)(((size_t)1 << 31) / wide.shapes.size()) + 1;
	pointProbe.ask(beyond, 0), queryBoxes.ask(beyond, 0), shapesInRange.ask(beyond, 0), shapesInRangeDistances.ask(beyond, 0);
	collideShape.ask(beyond, 0), castShapeAll.ask(beyond, 0);
	castShapeAll.ask(beyond - 1, 0); // (the largest batch it takes)

	const World small = makeWorld(40);
	place("a smaller world, in the block the larger ones left", small);
	batches(true);

	traceOff();
	s2amd_destroy(solver);
	if (failures == 0)
	{
		printf("QUERY MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
