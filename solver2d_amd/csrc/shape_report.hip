// Shape report of the resident world (include/solver2d_amd.h: s2amd_world_set_shape_report, s2amd_world_set_shape_view and the three
// getters): what s2World_Draw's shape pass (src/world.c:373-410, s2DrawShape :308-367) and its AABB pass (:427-460) read -- world-space
// vertices, the body's class, the boxes -- for the shapes a view box overlaps, compacted on the device behind stage 4 of
// s2amd_world_step and behind the joint report, instead of derived on the host from a download of shapes, bodies and origins.  The
// shape is joint_report.hip's:
//
//   shapeCountKernel   one pass over the shape slots in tiles of 256.  "In view now" (live, and no view set or s2AABB_Overlaps(view, aabb))
//                      against bit 0 of the report's own state byte gives `entered` and `left`.  Per-tile counts by wave ballots, and one
//                      partial per tile for s2amdShapeSummary: live / per-type / bad-body counts and the two boxes.  The pass reads the
//                      state byte and only then writes it back as {bit 0: in view now, bit 1: in view before the step}: the write pass
//                      finds both in it.
//   shapeWriteKernel   the same tiles.  Every tile adds up the counts of the tiles before it (report_common.h: tileCountsBefore) and
//                      writes its entries at their ranks: three ascending lists without a sort or an atomic.  A draw record is two full
//                      64-byte lines; a lane that stored its own record would write 16 bytes at a stride of 128 and leave every line to
//                      be merged from eight partial writes.  So each lane builds its record -- from 132 bytes of the 196-byte shape, read
//                      as eight 16-byte loads and one dword, never the normals -- into the tile's LDS image at its rank, 16-byte chunks
//                      XOR-swizzled by the rank so that neither side has a bank conflict, and after one barrier each wave stores the
//                      image 1 KiB per instruction: lane l the l-th 16-byte chunk, whole lines only.  The fourth wave of the last tile
//                      reduces the tiles' partials to the summary.
//
// Minimum and maximum of the boxes follow "x < cur ? x : cur" / "x > cur ? x : cur" from {+INF, +INF, -INF, -INF}; the reductions keep
// the slots in ascending order (of two equal values the one of the lower slot stays, as in a loop over the slots), so that even -0
// against +0 comes out as that loop leaves it.  The state bytes are the report's own and the passes are enqueued once per step, behind
// the attempt that stands: a repeated step reports once.  All device memory is one block sized by shapeReportPrepare; a step allocates
// nothing and waits for nothing -- the getters do.
#include "report_common.h"

#include <cmath>

namespace
{

#define S2_SHAPE_DWORDS 49	   // sizeof(s2amdShape) / 4
#define S2_SHAPE_READ_DWORDS 33 // header, radius, boxes and vertices: everything before the normals

static_assert(sizeof(s2amdShape) == 4 * S2_SHAPE_DWORDS && offsetof(s2amdShape, normals) == 4 * S2_SHAPE_READ_DWORDS, "the shape record as the write pass reads it");
static_assert(offsetof(s2amdShape, body) == 0 && offsetof(s2amdShape, type) == 4 && offsetof(s2amdShape, count) == 28 && offsetof(s2amdShape, radius) == 32 &&
				  offsetof(s2amdShape, aabb) == 36 && offsetof(s2amdShape, fatAABB) == 52 && offsetof(s2amdShape, vertices) == 68,
			  "the shape record as the write pass reads it");
static_assert(sizeof(s2amdShapeDraw) == 128 && sizeof(s2amdShapeSummary) == 64, "the report's records");

// 16 bytes at a 4-byte boundary: a shape record is 196 bytes, so only every fourth one starts on a 16-byte boundary
struct __attribute__((packed, aligned(4))) Chunk
{
	uint32_t x, y, z, w;
};

struct ShapeView
{
	float lx, ly, ux, uy;
	int set;
};

// what one tile of the count pass contributes to s2amdShapeSummary
struct ShapeTilePartial
{
	int32_t live, byType[4], bad, pad[2];
	float movable[4], view[4];
};
static_assert(sizeof(ShapeTilePartial) == 64, "one line per tile");

// the head of the report as the getters fetch it (solver_internal.h: hShapeReportHead)
struct ShapeReportHead
{
	int32_t counts[4]; // {in view, entered, left, 0}
	s2amdShapeSummary summary;
};

struct ShapeReportLayout
{
	size_t was, counts, partials, head, entered, left, records, total;
	int tiles;
};

ShapeReportLayout shapeReportLayout(int ns)
{
	ShapeReportLayout l{};
	size_t at = 0;
	l.tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	l.was = reportTake(at, (size_t)ns);
	l.counts = reportTake(at, (size_t)3 * l.tiles * sizeof(int));
	l.partials = reportTake(at, (size_t)l.tiles * sizeof(ShapeTilePartial));
	l.head = reportTake(at, sizeof(ShapeReportHead));
	l.entered = reportTake(at, (size_t)ns * sizeof(int32_t));
	l.left = reportTake(at, (size_t)ns * sizeof(int32_t));
	l.records = reportTake(at, (size_t)ns * sizeof(s2amdShapeDraw));
	l.total = at;
	return l;
}

// s2AABB_Overlaps(view, box), include/solver2d/aabb.h:111-123: false only when one of the four differences is > 0
S2_DEV bool viewOverlaps(const ShapeView& v, float lx, float ly, float ux, float uy)
{
	const float d1x = lx - v.ux, d1y = ly - v.uy;
	const float d2x = v.lx - ux, d2y = v.ly - uy;
	if (d1x > 0.0f || d1y > 0.0f)
	{
		return false;
	}
	if (d2x > 0.0f || d2y > 0.0f)
	{
		return false;
	}
	return true;
}

// src/world.c:389-405: a dynamic body without mass before anything else
S2_DEV int bodyClassOf(int type, float mass)
{
	if (type == S2AMD_BODY_DYNAMIC && mass == 0.0f)
	{
		return 3;
	}
	return type == S2AMD_BODY_STATIC ? 0 : type == S2AMD_BODY_KINEMATIC ? 1 : 2;
}

struct SlotFacts
{
	bool live, inView, movable, bad;
	int type;
	float box[4];
};

// what both passes need of slot i: 24 bytes of the shape (body, type, aabb) and 8 of its body (mass, type)
S2_DEV SlotFacts slotFacts(const uint32_t* shapeWords, int i, const s2amdBody* bodies, int nb, const ShapeView& view)
{
	SlotFacts f;
	const uint32_t* w = shapeWords + (size_t)i * S2_SHAPE_DWORDS;
	const int body = (int)w[0];
	f.type = (int)w[1];
	f.live = f.type != S2AMD_SHAPE_FREE;
	f.inView = false, f.movable = false, f.bad = false;
	f.box[0] = f.box[1] = f.box[2] = f.box[3] = 0.0f;
	if (f.live)
	{
		f.box[0] = __uint_as_float(w[9]), f.box[1] = __uint_as_float(w[10]), f.box[2] = __uint_as_float(w[11]), f.box[3] = __uint_as_float(w[12]);
		f.inView = view.set == 0 || viewOverlaps(view, f.box[0], f.box[1], f.box[2], f.box[3]);
		if (body >= 0 && body < nb) // (s2amd_world_upload refuses a live shape on a body outside the array)
		{
			const int bodyType = bodies[body].type;
			f.movable = bodyType != S2AMD_BODY_FREE && bodyType != S2AMD_BODY_STATIC;
			f.bad = bodyClassOf(bodyType, bodies[body].mass) == 3;
		}
	}
	return f;
}

// {lower.x, lower.y, upper.x, upper.y}: cur = the box over lower slots, x = a box over higher ones
S2_DEV void boxAdd(float* cur, const float* x)
{
	cur[0] = x[0] < cur[0] ? x[0] : cur[0];
	cur[1] = x[1] < cur[1] ? x[1] : cur[1];
	cur[2] = x[2] > cur[2] ? x[2] : cur[2];
	cur[3] = x[3] > cur[3] ? x[3] : cur[3];
}

S2_DEV void boxEmpty(float* b)
{
	b[0] = b[1] = INFINITY;
	b[2] = b[3] = -INFINITY;
}

// The 64 lanes' boxes, lane 0's slots below lane 1's and so on, to one box in every lane: after the step of distance d a lane holds the
// box of the 2d consecutive lanes around it, and the half with the lower lanes is `cur` of boxAdd.
S2_DEV void boxOverWave(float* b, int lane)
{
	for (int d = 1; d < 64; d <<= 1)
	{
		float other[4];
		for (int k = 0; k < 4; ++k)
		{
			other[k] = __shfl_xor(b[k], d);
		}
		if ((lane & d) != 0)
		{
			// the partner holds the lower slots
			boxAdd(other, b);
			for (int k = 0; k < 4; ++k)
			{
				b[k] = other[k];
			}
		}
		else
		{
			boxAdd(b, other);
		}
	}
}

__global__ __launch_bounds__(S2_BLOCK) void shapeInitKernel(const uint32_t* shapeWords, int n, const s2amdBody* bodies, int nb, ShapeView view, uint8_t* was)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n)
	{
		was[i] = slotFacts(shapeWords, i, bodies, nb, view).inView ? 1 : 0;
	}
}

// counts[0..tiles) in view, [tiles..2 tiles) entered, [2 tiles..3 tiles) left; partials[tile]; was[i] = {bit 0 now, bit 1 before}
// Reads per slot 8 bytes of the shape and its state byte; per live slot also the 16-byte aabb and 8 bytes of its body.
__global__ __launch_bounds__(S2_BLOCK) void shapeCountKernel(const uint32_t* shapeWords, uint8_t* was, int n, int tiles, const s2amdBody* bodies, int nb, ShapeView view,
															 int* counts, ShapeTilePartial* partials)
{
	__shared__ int waves[9][S2_BLOCK / 64];
	__shared__ float waveBox[2][S2_BLOCK / 64][4];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	SlotFacts f;
	f.live = f.inView = f.movable = f.bad = false, f.type = S2AMD_SHAPE_FREE;
	bool before = false;
	if (i < n)
	{
		f = slotFacts(shapeWords, i, bodies, nb, view);
		before = (was[i] & 1) != 0;
		was[i] = (uint8_t)((f.inView ? 1 : 0) | (before ? 2 : 0));
	}
	float movable[4], seen[4];
	boxEmpty(movable), boxEmpty(seen);
	if (f.live && f.movable)
	{
		boxAdd(movable, f.box);
	}
	if (f.inView)
	{
		boxAdd(seen, f.box);
	}
	boxOverWave(movable, lane), boxOverWave(seen, lane);
	const int nView = __popcll(__ballot(f.inView));
	const int nEntered = __popcll(__ballot(f.inView && !before)), nLeft = __popcll(__ballot(before && !f.inView));
	const int nLive = __popcll(__ballot(f.live)), nBad = __popcll(__ballot(f.live && f.bad));
	int nType[4];
	for (int t = 0; t < 4; ++t)
	{
		nType[t] = __popcll(__ballot(f.live && f.type == t));
	}
	if (lane == 0)
	{
		waves[0][wave] = nView, waves[1][wave] = nEntered, waves[2][wave] = nLeft, waves[3][wave] = nLive;
		waves[4][wave] = nType[0], waves[5][wave] = nType[1], waves[6][wave] = nType[2], waves[7][wave] = nType[3];
		waves[8][wave] = nBad;
		for (int k = 0; k < 4; ++k)
		{
			waveBox[0][wave][k] = movable[k], waveBox[1][wave][k] = seen[k];
		}
	}
	__syncthreads();
	if (threadIdx.x < 9)
	{
		int total = 0;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			total += waves[threadIdx.x][w];
		}
		if (threadIdx.x < 3)
		{
			counts[(int)threadIdx.x * tiles + (int)blockIdx.x] = total;
		}
		else if (threadIdx.x == 3)
		{
			partials[blockIdx.x].live = total;
		}
		else if (threadIdx.x < 8)
		{
			partials[blockIdx.x].byType[threadIdx.x - 4] = total;
		}
		else
		{
			partials[blockIdx.x].bad = total;
		}
	}
	else if (threadIdx.x < 11)
	{
		// the tile's boxes: its waves in order
		const int which = (int)threadIdx.x - 9;
		float b[4];
		boxEmpty(b);
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			boxAdd(b, waveBox[which][w]);
		}
		float* out = which == 0 ? partials[blockIdx.x].movable : partials[blockIdx.x].view;
		out[0] = b[0], out[1] = b[1], out[2] = b[2], out[3] = b[3];
	}
	else if (threadIdx.x == 11)
	{
		partials[blockIdx.x].pad[0] = 0, partials[blockIdx.x].pad[1] = 0;
	}
}

// One record into the tile's LDS image at rank r: chunk c (16 bytes) of the record is slot r * 8 + (c ^ (r & 7)) of the image, so the
// eight lanes one ds_write_b128 cycle serves hit eight different 16-byte slots of the 32 banks, and the 64 consecutive slots a wave
// reads back are a permutation of eight whole rows.
S2_DEV void stageChunk(float4* image, int r, int c, float4 v)
{
	image[r * 8 + (c ^ (r & 7))] = v;
}

// head->counts = {in view, entered, left} of the step, head->summary; `flags`: which lists are wanted.
// Reads per slot what the count pass read; under DRAW per shape in view 132 bytes of the shape and 16 of its body (origin, rot), and
// writes two full 64-byte lines; 4 bytes per event.
__global__ __launch_bounds__(S2_BLOCK) void shapeWriteKernel(const uint32_t* shapeWords, const uint8_t* was, int n, int tiles, const int* counts,
															 const ShapeTilePartial* partials, const s2amdBody* bodies, const float2* origins, int nb, int flags,
															 ShapeReportHead* head, int32_t* enteredOut, int32_t* leftOut, float4* records)
{
	__shared__ float4 image[S2_BLOCK * 8]; // 256 records of 128 bytes
	__shared__ int waves[3][S2_BLOCK / 64];
	__shared__ int base[3];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	bool now = false, before = false;
	if (i < n)
	{
		const int state = was[i];
		now = (state & 1) != 0, before = (state & 2) != 0;
	}
	const bool entered = now && !before, left = before && !now;
	const unsigned long long viewMask = __ballot(now), enteredMask = __ballot(entered), leftMask = __ballot(left);
	if (lane == 0)
	{
		waves[0][wave] = __popcll(viewMask), waves[1][wave] = __popcll(enteredMask), waves[2][wave] = __popcll(leftMask);
	}
	if (wave < 3)
	{
		// the tiles before this one: wave w adds up list w's counts
		int partial = tileCountsBefore(counts, tiles, wave, (int)blockIdx.x, lane);
		for (int d = 32; d > 0; d >>= 1)
		{
			partial += __shfl_xor(partial, d);
		}
		if (lane == 0)
		{
			base[wave] = partial;
		}
	}
	else if ((int)blockIdx.x == tiles - 1)
	{
		// the summary: the idle wave of the last tile adds up the tiles' partials, each lane a run of consecutive tiles
		const int run = (tiles + 63) / 64;
		int nView = 0, nLive = 0, nBad = 0, nType[4] = {0, 0, 0, 0};
		float movable[4], seen[4];
		boxEmpty(movable), boxEmpty(seen);
		for (int b = lane * run; b < (lane + 1) * run && b < tiles; ++b)
		{
			const ShapeTilePartial p = partials[b];
			nView += counts[b];
			nLive += p.live, nBad += p.bad;
			nType[0] += p.byType[0], nType[1] += p.byType[1], nType[2] += p.byType[2], nType[3] += p.byType[3];
			boxAdd(movable, p.movable), boxAdd(seen, p.view);
		}
		for (int d = 32; d > 0; d >>= 1)
		{
			nView += __shfl_xor(nView, d), nLive += __shfl_xor(nLive, d), nBad += __shfl_xor(nBad, d);
			nType[0] += __shfl_xor(nType[0], d), nType[1] += __shfl_xor(nType[1], d);
			nType[2] += __shfl_xor(nType[2], d), nType[3] += __shfl_xor(nType[3], d);
		}
		boxOverWave(movable, lane), boxOverWave(seen, lane);
		if (lane == 0)
		{
			s2amdShapeSummary s{};
			s.liveShapes = nLive, s.inView = nView, s.badBodyShapes = nBad;
			for (int k = 0; k < 4; ++k)
			{
				s.byType[k] = nType[k];
				s.movableBounds[k] = movable[k], s.viewBounds[k] = seen[k];
			}
			head->summary = s;
		}
	}
	__syncthreads();
	int at[3] = {base[0], base[1], base[2]};
	int tileRank = 0; // of this lane's record among the tile's
	for (int w = 0; w < wave; ++w)
	{
		tileRank += waves[0][w], at[1] += waves[1][w], at[2] += waves[2][w];
	}
	const int tileRecords = waves[0][0] + waves[0][1] + waves[0][2] + waves[0][3];
	const unsigned long long lower = (1ull << lane) - 1ull;
	tileRank += __popcll(viewMask & lower);
	at[1] += __popcll(enteredMask & lower);
	at[2] += __popcll(leftMask & lower);
	if ((int)blockIdx.x == tiles - 1 && threadIdx.x == blockDim.x - 1)
	{
		head->counts[0] = at[0] + tileRank + (now ? 1 : 0);
		head->counts[1] = at[1] + (entered ? 1 : 0);
		head->counts[2] = at[2] + (left ? 1 : 0);
		head->counts[3] = 0;
	}
	if ((flags & S2AMD_SHAPE_REPORT_VIEW) != 0)
	{
		if (entered)
		{
			enteredOut[at[1]] = i;
		}
		if (left)
		{
			leftOut[at[2]] = i;
		}
	}
	if ((flags & S2AMD_SHAPE_REPORT_DRAW) == 0)
	{
		return; // (the whole block: `flags` is the launch's)
	}
	if (now)
	{
		// (`now` implies i < n and a live slot)
		const Chunk* src = (const Chunk*)(shapeWords + (size_t)i * S2_SHAPE_DWORDS);
		uint32_t d[S2_SHAPE_READ_DWORDS];
#pragma unroll
		for (int c = 0; c < 8; ++c)
		{
			const Chunk q = src[c];
			d[4 * c] = q.x, d[4 * c + 1] = q.y, d[4 * c + 2] = q.z, d[4 * c + 3] = q.w;
		}
		d[32] = shapeWords[(size_t)i * S2_SHAPE_DWORDS + 32];
		const int body = (int)d[0], type = (int)d[1];
		float2 origin = make_float2(0.0f, 0.0f), rot = make_float2(0.0f, 1.0f);
		int bodyType = S2AMD_BODY_STATIC;
		float mass = 0.0f;
		if (body >= 0 && body < nb)
		{
			origin = origins[body];
			rot = make_float2(bodies[body].rot[0], bodies[body].rot[1]);
			bodyType = bodies[body].type, mass = bodies[body].mass;
		}
		int vertexCount = 0;
		if (type == S2AMD_SHAPE_POLYGON)
		{
			const int count = (int)d[7];
			vertexCount = count < 0 ? 0 : count > 8 ? 8 : count;
		}
		else if (type == S2AMD_SHAPE_CAPSULE || type == S2AMD_SHAPE_SEGMENT)
		{
			vertexCount = 2;
		}
		else if (type == S2AMD_SHAPE_CIRCLE)
		{
			vertexCount = 1;
		}
		// s2RotateVector(rot, {1, 0}), include/solver2d/math.h:330-341
		const float axisX = rot.y * 1.0f - rot.x * 0.0f, axisY = rot.x * 1.0f + rot.y * 0.0f;
		stageChunk(image, tileRank, 0, make_float4(__int_as_float(i), __int_as_float(body), __int_as_float(type), __int_as_float(vertexCount)));
		stageChunk(image, tileRank, 1, make_float4(__int_as_float(bodyClassOf(bodyType, mass)), __uint_as_float(d[8]), axisX, axisY));
#pragma unroll
		for (int c = 0; c < 4; ++c)
		{
			float2 a = make_float2(0.0f, 0.0f), b = make_float2(0.0f, 0.0f);
			if (2 * c < vertexCount)
			{
				a = transformPoint(origin, rot, make_float2(__uint_as_float(d[17 + 4 * c]), __uint_as_float(d[18 + 4 * c])));
			}
			if (2 * c + 1 < vertexCount)
			{
				b = transformPoint(origin, rot, make_float2(__uint_as_float(d[19 + 4 * c]), __uint_as_float(d[20 + 4 * c])));
			}
			stageChunk(image, tileRank, 2 + c, make_float4(a.x, a.y, b.x, b.y));
		}
		stageChunk(image, tileRank, 6, make_float4(__uint_as_float(d[9]), __uint_as_float(d[10]), __uint_as_float(d[11]), __uint_as_float(d[12])));
		stageChunk(image, tileRank, 7, make_float4(__uint_as_float(d[13]), __uint_as_float(d[14]), __uint_as_float(d[15]), __uint_as_float(d[16])));
	}
	__syncthreads();
	// the tile's records are consecutive in the list: chunk g of the image goes to chunk g behind the tile's first record
	float4* out = records + (size_t)at[0] * 8;
	for (int g = (int)threadIdx.x; g < tileRecords * 8; g += S2_BLOCK)
	{
		const int r = g >> 3, c = g & 7;
		out[g] = image[r * 8 + (c ^ (r & 7))];
	}
}

ShapeReportLayout layoutOf(const s2amdSolver* s)
{
	return shapeReportLayout(s->shapeCapacity);
}

ShapeView viewOf(const s2amdSolver* s)
{
	ShapeView v;
	v.lx = s->shapeView[0], v.ly = s->shapeView[1], v.ux = s->shapeView[2], v.uy = s->shapeView[3];
	v.set = s->shapeViewSet ? 1 : 0;
	return v;
}

ReportRef ref(s2amdSolver* s)
{
	static_assert(sizeof(s->hShapeReportHead) == sizeof(ShapeReportHead), "the host copy of the report's head");
	return s ? ReportRef{s, &s->shapeReport, &s->hShapeReportHead, sizeof(s->hShapeReportHead), "shape-report", "s2amd_world_set_shape_report"} : ReportRef{};
}

// where a piece of the block lies, for a getter (0 for the null solver it will refuse)
size_t at(const s2amdSolver* s, size_t ShapeReportLayout::*piece)
{
	return s ? layoutOf(s).*piece : 0;
}

// "before" := in view as the resident shapes stand now, under the view as it is now
int shapeReportRestate(s2amdSolver* s)
{
	const int ns = s->shapeCapacity;
	const ShapeReportLayout l = layoutOf(s);
	if (ns <= 0 || s->shapeReport.block.p == nullptr || s->shapeReport.block.bytes < l.total)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	shapeInitKernel<<<gridFor((size_t)ns), dim3(S2_BLOCK), 0, s->stream>>>((const uint32_t*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, s->bodyCapacity, viewOf(s),
																		   (uint8_t*)((char*)s->shapeReport.block.p + l.was));
	HIP_TRY(hipGetLastError());
	return S2AMD_OK;
}

} // namespace

int shapeReportPrepare(s2amdSolver* s)
{
	if (!reportPrepareBegin(s, s->shapeReport))
	{
		return S2AMD_OK;
	}
	const ShapeReportLayout l = layoutOf(s);
	const int rc = reportPrepareBlock(s->shapeReport, l.total, l.head);
	return rc ? rc : shapeReportRestate(s);
}

int shapeReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->shapeReport;
	const int flags = r.flags;
	const int ns = s->shapeCapacity;
	const ShapeReportLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "shape"))
	{
		return rc;
	}
	if (ns > 0)
	{
		hipStream_t st = s->stream;
		char* base = (char*)r.block.p;
		const uint32_t* shapeWords = (const uint32_t*)s->dShapes.p;
		const s2amdBody* bodies = (const s2amdBody*)s->dBodies.p;
		shapeCountKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(shapeWords, (uint8_t*)(base + l.was), ns, l.tiles, bodies, s->bodyCapacity, viewOf(s),
																			 (int*)(base + l.counts), (ShapeTilePartial*)(base + l.partials));
		shapeWriteKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(shapeWords, (const uint8_t*)(base + l.was), ns, l.tiles, (const int*)(base + l.counts),
																			 (const ShapeTilePartial*)(base + l.partials), bodies, (const float2*)s->dOrigins.p, s->bodyCapacity,
																			 flags, (ShapeReportHead*)(base + l.head), (int32_t*)(base + l.entered), (int32_t*)(base + l.left),
																			 (float4*)(base + l.records));
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (a world without shape slots launches no tile: its head is known here)
		s->hShapeReportHead = {};
		s->hShapeReportHead.summary.movableBounds[0] = s->hShapeReportHead.summary.movableBounds[1] = INFINITY;
		s->hShapeReportHead.summary.movableBounds[2] = s->hShapeReportHead.summary.movableBounds[3] = -INFINITY;
		s->hShapeReportHead.summary.viewBounds[0] = s->hShapeReportHead.summary.viewBounds[1] = INFINITY;
		s->hShapeReportHead.summary.viewBounds[2] = s->hShapeReportHead.summary.viewBounds[3] = -INFINITY;
	}
	r.stepFlags = flags;
	r.headKnown = ns <= 0;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_shape_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2AMD_SHAPE_REPORT_DRAW | S2AMD_SHAPE_REPORT_VIEW | S2AMD_SHAPE_REPORT_BOUNDS, shapeReportPrepare);
}

int s2amd_world_set_shape_view(s2amdSolver* s, const float* box)
{
	if (!s)
	{
		return fail(S2AMD_E_INVALID, "null solver");
	}
	if (box)
	{
		// (written so that a NaN fails it)
		if (!(box[0] <= box[2]) || !(box[1] <= box[3]))
		{
			return fail(S2AMD_E_INVALID, "shape view: lower > upper, or a NaN");
		}
		s->shapeView[0] = box[0], s->shapeView[1] = box[1], s->shapeView[2] = box[2], s->shapeView[3] = box[3];
	}
	s->shapeViewSet = box != nullptr;
	if (s->shapeReport.flags != 0 && s->worldResident)
	{
		// "before" of the next step is taken under the new view: the change itself is no event
		return shapeReportRestate(s);
	}
	return S2AMD_OK;
}

int s2amd_world_shape_draws(s2amdSolver* s, s2amdShapeDraw* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_SHAPE_REPORT_DRAW, "s2amd_world_shape_draws", "shape-draw buffer too small", 0, at(s, &ShapeReportLayout::records), sizeof(*out), out, capacity,
						 count);
}

int s2amd_world_shape_view_events(s2amdSolver* s, int32_t* entered, int32_t enteredCapacity, int32_t* enteredCount, int32_t* left, int32_t leftCapacity, int32_t* leftCount)
{
	return reportGetEvents(ref(s), S2AMD_SHAPE_REPORT_VIEW, "s2amd_world_shape_view_events", "shape view event buffer too small", 1, at(s, &ShapeReportLayout::entered),
						   at(s, &ShapeReportLayout::left), entered, enteredCapacity, enteredCount, left, leftCapacity, leftCount);
}

int s2amd_world_shape_summary(s2amdSolver* s, s2amdShapeSummary* out)
{
	const int rc = out ? reportHeadFor(ref(s), 0, "s2amd_world_shape_summary") : fail(S2AMD_E_INVALID, "bad argument");
	if (rc == S2AMD_OK)
	{
		*out = s->hShapeReportHead.summary;
	}
	return rc;
}

} // extern "C"
#pragma GCC visibility pop
