// Grid report of the resident world (include/solver2d_amd.h: s2amd_world_set_grid_sensors, s2amd_world_set_grid_report and the five
// getters): a list of up to 1,024 occupancy grids, fixed in the world or mounted on bodies, rasterised behind every s2amd_world_step --
// what a caller otherwise composes per step from a pose download, width x height cell centres computed on the host, one
// s2amd_world_point_probe call and a fold of its CSR list into an image.  A cell is that call's statement (scene_query.hip) for the
// cell's centre, folded with OR (categories) and min (lowest slot), with two further exclusions from the candidates: the shapes of the
// grid's own body, and with SKIP_STATIC the shapes on static bodies.  The passes are enqueued behind stage 4 of s2amd_world_step and
// behind the other seven reports, once per step (a repeated step reports once); the report keeps nothing from step to step.
//
//   gridPoseKernel        one lane per grid: active and the frame G (mount_ops.h: the mount rule), the
//                         box of the four corner cells' centres, staged as one 64-byte record; the state with occupied = 0 and
//                         lowestShape = -1, which the raster pass counts into.
//   gridCandidatesKernel  the sensor report's mask idea: a workgroup holds one tile of 256 shape slots -- 28 bytes of the slot (body,
//                         type, category, fat box) and its body's type in registers -- and walks one chunk of up to 256 posed grids
//                         staged in LDS (8 KiB), every grid a broadcast read.  The ballot of a wave is one word of the
//                         grids x (tiles * 4) mask.  No atomic; every word is written.
//   gridRasterKernel      a wave owns one tile of 64 cells of one grid (the table of tiles is built on the host when the list is set, so
//                         no tile straddles two grids): an 8 x 8 block of cells (64 consecutive cells of a row measured slower, DESIGN.md
//                         section 6a).  A lane computes its own cell centre P once; the wave walks its grid's mask words and, inside a
//                         word, the set bits -- both loops wave-uniform -- reads the candidate's record at a uniform address, and every
//                         lane tests its own P against the fat box first and the geometry second.  A polygon some lane has to test is
//                         staged by lanes 0..7, one vertex each as two floats, into the wave's 64 bytes of LDS and read from there at
//                         stride 1.  The OR and the minimum stay in registers; each requested array takes one 4-byte store per lane;
//                         occupied is a wave popcount and one integer atomic add, lowestShape one integer atomic min (as unsigned: -1
//                         is the largest value, so "none" needs no second pass); the wave with a grid's first tile writes candidates,
//                         the popcount of the grid's mask.
//
// No float atomics, no scratch.  The point tests are query_ops.h's and gjk_ops.h's, in scene_query.hip's sequence (s2Shape_TestPoint;
// that file's kernels stay as they were, instruction for instruction).  All arithmetic is fp32 in the reference's operation order; this file is compiled without
// contraction in both libraries (Makefile).  All device memory is one block sized by gridReportPrepare; a step allocates nothing and
// waits for nothing -- the getters do.
#include "report_common.h"

#define S2_NP_BLOCK 1 // a polygon is the wave's eight staged vertices (stride 1); the probed point is a one-vertex proxy of the lane's own
#define S2_NP_MAX_VERTS 8
#include "query_ops.h"
#include "mount_ops.h"

#include <cmath>
#include <cstring>

namespace
{

static_assert(sizeof(s2amdGridSensor) == 64 && sizeof(s2amdGridState) == 64, "the report's records");
static_assert(sizeof(s2amdShape) == 196, "the shape record");

#define S2_GRID_SENSOR_KNOWN_FLAGS (S2AMD_GRID_SENSOR_DISABLED | S2AMD_GRID_SENSOR_SKIP_STATIC)
#define S2_GRID_REPORT_KNOWN (S2AMD_GRID_REPORT_CATEGORIES | S2AMD_GRID_REPORT_SHAPES | S2AMD_GRID_REPORT_OCCUPANCY | S2AMD_GRID_REPORT_STATES)
#define S2_GRID_CHUNK S2_BLOCK // grids a workgroup of the candidates pass stages: one per lane

// a grid as the candidates and the raster pass read it: the frame, the rule's fields, the extent, the candidate box
struct alignas(16) PosedGrid
{
	float px, py, s, c;
	float cellSize;
	uint32_t mask;
	int32_t body; // the grid's own (< 0: fixed in the world, nothing excluded)
	int32_t bits; // 1: active, 2: SKIP_STATIC
	int32_t width, height, firstCell, pad;
	float lx, ly, ux, uy;
};
static_assert(sizeof(PosedGrid) == 64, "four 16-byte words per staged grid");

// a tile of 64 cells of one grid: the 8 x 8 block whose first cell is (a, b)
struct alignas(16) GridTile
{
	int32_t grid, a, b, first; // first != 0: the grid's first tile (its wave writes `candidates`)
};

struct GridLayout
{
	size_t grids, posed, states, masks, tiles, head, categories, shapes, occupancy, total;
	size_t words; // mask words per grid
	int shapeTiles;
};

GridLayout gridLayout(int count, size_t cells, size_t cellTiles, int ns)
{
	GridLayout l{};
	size_t at = 0;
	l.shapeTiles = (std::max(ns, 0) + S2_BLOCK - 1) / S2_BLOCK;
	l.words = (size_t)l.shapeTiles * 4;
	l.grids = reportTake(at, (size_t)count * sizeof(s2amdGridSensor));
	l.posed = reportTake(at, (size_t)count * sizeof(PosedGrid));
	l.states = reportTake(at, (size_t)count * sizeof(s2amdGridState));
	l.masks = reportTake(at, (size_t)count * l.words * sizeof(unsigned long long));
	l.tiles = reportTake(at, cellTiles * sizeof(GridTile));
	l.head = reportTake(at, 4 * sizeof(int32_t));
	l.categories = reportTake(at, cells * sizeof(uint32_t));
	l.shapes = reportTake(at, cells * sizeof(int32_t));
	l.occupancy = reportTake(at, cells * sizeof(float));
	l.total = at;
	return l;
}

// the centre of cell (i, j) in the grid's own frame: everything in front of the one multiply is exact
S2_DEV V2 cellLocal(int i, int j, int width, int height, float cellSize)
{
	const float x = (((float)i + 0.5f) - 0.5f * (float)width) * cellSize;
	const float y = (((float)j + 0.5f) - 0.5f * (float)height) * cellSize;
	return v2(x, y);
}

// posed[g] and states[g] (occupied = candidates = 0, lowestShape = -1: the raster pass's)
__global__ __launch_bounds__(S2_BLOCK) void gridPoseKernel(const s2amdGridSensor* grids, int count, const s2amdBody* bodies, const float2* origins, int nb, PosedGrid* posed,
															s2amdGridState* states)
{
	const int g = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (g >= count)
	{
		return;
	}
	const s2amdGridSensor* q = grids + g;
	const int body = q->body, flags = q->flags, width = q->width, height = q->height;
	const int firstCell = q->pad[0]; // (the prefix sum the setter left there)
	const float cellSize = q->cellSize;
	// mount_ops.h's mountFrame, spelt out: called here, the compiler pairs this kernel's loads and multiplies differently, and the kernel is to stay as it was
	bool active = (flags & S2AMD_GRID_SENSOR_DISABLED) == 0;
	Xf xf;
	xf.p = v2(q->position[0], q->position[1]);
	xf.q.s = q->rot[0], xf.q.c = q->rot[1];
	if (active && body >= 0)
	{
		active = liveBody(bodies, nb, body);
		if (active)
		{
			const float2 o = origins[body];
			const float bs = bodies[body].rot[0], bc = bodies[body].rot[1];
			const float s = bs * xf.q.c + bc * xf.q.s;
			const float c = bc * xf.q.c - bs * xf.q.s;
			const float px = (bc * xf.p.x - bs * xf.p.y) + o.x;
			const float py = (bs * xf.p.x + bc * xf.p.y) + o.y;
			xf.p = v2(px, py);
			xf.q.s = s, xf.q.c = c;
		}
	}
	float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (active)
	{
		// the four corner cells, in the order (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)
		const V2 a = xfPoint(xf, cellLocal(0, 0, width, height, cellSize));
		const V2 b = xfPoint(xf, cellLocal(width - 1, 0, width, height, cellSize));
		const V2 c = xfPoint(xf, cellLocal(0, height - 1, width, height, cellSize));
		const V2 d = xfPoint(xf, cellLocal(width - 1, height - 1, width, height, cellSize));
		active = finiteBits(a.x) && finiteBits(a.y) && finiteBits(b.x) && finiteBits(b.y) && finiteBits(c.x) && finiteBits(c.y) && finiteBits(d.x) && finiteBits(d.y);
		if (active)
		{
			V2 lower = a, upper = a;
			lower = v2(S2_MINF(lower.x, b.x), S2_MINF(lower.y, b.y)), upper = v2(S2_MAXF(upper.x, b.x), S2_MAXF(upper.y, b.y));
			lower = v2(S2_MINF(lower.x, c.x), S2_MINF(lower.y, c.y)), upper = v2(S2_MAXF(upper.x, c.x), S2_MAXF(upper.y, c.y));
			lower = v2(S2_MINF(lower.x, d.x), S2_MINF(lower.y, d.y)), upper = v2(S2_MAXF(upper.x, d.x), S2_MAXF(upper.y, d.y));
			box = make_float4(lower.x, lower.y, upper.x, upper.y);
		}
	}
	if (!active) // (the corners of an active mount may still fail)
	{
		xf = noFrame();
	}
	float4* to = (float4*)(posed + g);
	to[0] = make_float4(xf.p.x, xf.p.y, xf.q.s, xf.q.c);
	to[1] = make_float4(cellSize, __uint_as_float(q->maskBits), __int_as_float(body),
						__int_as_float((active ? 1 : 0) | ((flags & S2AMD_GRID_SENSOR_SKIP_STATIC) != 0 ? 2 : 0)));
	to[2] = make_float4(__int_as_float(width), __int_as_float(height), __int_as_float(firstCell), __int_as_float(0));
	to[3] = box;
	float4* st = (float4*)(states + g);
	st[0] = make_float4(__int_as_float(g), __int_as_float(body), __int_as_float(active ? 1 : 0), __int_as_float(firstCell));
	st[1] = make_float4(__int_as_float(width * height), __int_as_float(0), __int_as_float(-1), __int_as_float(0));
	st[2] = make_float4(xf.p.x, xf.p.y, xf.q.s, xf.q.c);
	st[3] = box;
}

// masks[(grid * tiles + tile) * 4 + wave], bit = lane: the wave's candidates of the grid.  Every word is written.
__global__ __launch_bounds__(S2_BLOCK) void gridCandidatesKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, int nb, const PosedGrid* posed, int count,
																  unsigned long long* masks)
{
	__shared__ float4 staged[S2_GRID_CHUNK][2]; // {mask, body, bits, 0}, the box
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_GRID_CHUNK;
	const int chunk = count - first < S2_GRID_CHUNK ? count - first : S2_GRID_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		const float4* from = (const float4*)(posed + first + (int)threadIdx.x);
		const float4 rule = from[1];
		staged[threadIdx.x][0] = make_float4(rule.y, rule.z, rule.w, 0.0f);
		staged[threadIdx.x][1] = from[3];
	}
	bool live = false, onStatic = false;
	int body = -1;
	uint32_t category = 0u;
	float fat[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	if (slot < n)
	{
		const s2amdShape* w = shapes + slot;
		live = w->type != S2AMD_SHAPE_FREE;
		if (live)
		{
			body = w->body;
			category = w->categoryBits;
			fat[0] = w->fatAABB[0], fat[1] = w->fatAABB[1], fat[2] = w->fatAABB[2], fat[3] = w->fatAABB[3];
			onStatic = body >= 0 && body < nb && bodies[body].type == S2AMD_BODY_STATIC;
		}
	}
	__syncthreads();
	for (int k = 0; k < chunk; ++k)
	{
		const float4 rule = staged[k][0], box = staged[k][1];
		const uint32_t mask = __float_as_uint(rule.x);
		const int own = __float_as_int(rule.y), bits = __float_as_int(rule.z);
		const bool candidate = live && (bits & 1) != 0 && (category & mask) != 0u && !(own >= 0 && body == own) && !((bits & 2) != 0 && onStatic) &&
							   boxesOverlap(fat, box.x, box.y, box.z, box.w);
		const unsigned long long ballot = __ballot(candidate);
		if (lane == 0)
		{
			masks[((size_t)(first + k) * tiles + blockIdx.x) * 4 + wave] = ballot;
		}
	}
}

S2_DEV int uniform(int v)
{
	return __builtin_amdgcn_readfirstlane(v);
}

// orders the wave's own LDS traffic: lanes 0..7 stage a polygon that all 64 lanes read, with no other wave involved
S2_DEV void waveLdsSync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

// s2Shape_TestPoint (src/shape.c:110-137) of world point P on the shape record w (read at a uniform address), its fat box passed
S2_DEV bool cellHits(const s2amdShape* w, int type, const s2amdBody* bodies, const float2* origins, int nb, V2 P, float2* staged, const PolyRef& point)
{
	const int body = w->body;
	Xf xf;
	xf.p = v2(0.0f, 0.0f);
	xf.q.s = 0.0f, xf.q.c = 1.0f;
	if (body >= 0 && body < nb) // (s2amd_world_upload refuses a live shape on a body outside the array)
	{
		const float2 o = origins[body];
		xf.p = v2(o.x, o.y);
		xf.q.s = bodies[body].rot[0], xf.q.c = bodies[body].rot[1];
	}
	const V2 local = xfInvPoint(xf, P);
	const float radius = w->radius;
	switch (type)
	{
		case S2AMD_SHAPE_CAPSULE:
			return pointInCapsule(local, v2(w->vertices[0][0], w->vertices[0][1]), v2(w->vertices[1][0], w->vertices[1][1]), radius);
		case S2AMD_SHAPE_CIRCLE:
			return pointInCircle(local, v2(w->vertices[0][0], w->vertices[0][1]), radius);
		case S2AMD_SHAPE_POLYGON:
		{
			PolyRef polygon;
			const int count = w->count;
			polygon.verts = staged;
			polygon.norms = nullptr;
			polygon.count = count < 0 ? 0 : count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : count;
			polygon.radius = radius;
			point.verts[0] = make_float2(local.x, local.y);
			return pointInPolygon(polygon, point);
		}
		default:
			return false;
	}
}

// the cells of tile `blockIdx.x * 4 + wave`: categories / shapes / occupancy at the cell's index (each where `flags` asks), and the
// grid's occupied, lowestShape and candidates
__global__ __launch_bounds__(S2_BLOCK) void gridRasterKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const PosedGrid* posed,
															  const GridTile* tiles, int tileCount, const unsigned long long* masks, int words, int flags, uint32_t* categories,
															  int32_t* lowest, float* occupancy, s2amdGridState* states)
{
	__shared__ float2 probe[S2_BLOCK];
	__shared__ float2 polygons[(S2_BLOCK / 64) * S2_NP_MAX_VERTS];
	const int lane = (int)(threadIdx.x & 63);
	const int t = uniform((int)(blockIdx.x * (S2_BLOCK / 64) + (threadIdx.x >> 6)));
	if (t >= tileCount) // (whole waves; the kernel has no workgroup barrier)
	{
		return;
	}
	float2* staged = polygons + (threadIdx.x >> 6) * S2_NP_MAX_VERTS;
	const GridTile tile = tiles[t];
	const int g = uniform(tile.grid);
	const PosedGrid q = posed[g];
	const int width = uniform(q.width), height = uniform(q.height);
	const int i = tile.a + (lane & 7), j = tile.b + (lane >> 3);
	const bool cell = i < width && j < height;
	const bool active = uniform(q.bits & 1) != 0;
	Xf G;
	G.p = v2(q.px, q.py);
	G.q.s = q.s, G.q.c = q.c;
	const V2 P = xfPoint(G, cellLocal(i, j, width, height, q.cellSize));
	PolyRef point;
	point.verts = probe + threadIdx.x, point.norms = nullptr;
	point.count = 1, point.radius = 0.0f;
	uint32_t seen = 0u;
	int shape = -1;
	int candidates = 0;
	const unsigned long long* mine = masks + (size_t)g * words;
	if (active)
	{
		for (int w = 0; w < words; ++w)
		{
			const unsigned long long m = mine[w];
			uint32_t lo = (uint32_t)uniform((int)(uint32_t)(m & 0xffffffffull)), hi = (uint32_t)uniform((int)(uint32_t)(m >> 32));
			candidates += __popc(lo) + __popc(hi);
			for (int half = 0; half < 2; ++half)
			{
				uint32_t bits = half == 0 ? lo : hi;
				while (bits != 0u)
				{
					const int bit = __ffs((int)bits) - 1;
					bits &= bits - 1u;
					const int slot = w * 64 + half * 32 + bit;
					if (slot >= n) // (the mask pass sets no such bit)
					{
						continue;
					}
					const s2amdShape* record = shapes + slot;
					float fat[4];
					fat[0] = record->fatAABB[0], fat[1] = record->fatAABB[1], fat[2] = record->fatAABB[2], fat[3] = record->fatAABB[3];
					const bool inBox = cell && boxesOverlap(fat, P.x, P.y, P.x, P.y);
					if (__ballot(inBox) == 0ull) // (the whole wave: an 8 x 8 block is 2 m wide, most candidates end here)
					{
						continue;
					}
					const int type = uniform(record->type);
					if (type == S2AMD_SHAPE_POLYGON)
					{
						waveLdsSync(); // (the lanes' reads of the polygon before are done)
						if (lane < S2_NP_MAX_VERTS)
						{
							staged[lane] = make_float2(record->vertices[lane][0], record->vertices[lane][1]);
						}
						waveLdsSync();
					}
					if (inBox && cellHits(record, type, bodies, origins, nb, P, staged, point))
					{
						seen |= record->categoryBits;
						shape = shape < 0 ? slot : shape; // (the slots ascend: the first hit is the lowest)
					}
				}
			}
		}
	}
	if (cell)
	{
		const size_t at = (size_t)q.firstCell + (size_t)j * width + i;
		if ((flags & S2AMD_GRID_REPORT_CATEGORIES) != 0)
		{
			categories[at] = seen;
		}
		if ((flags & S2AMD_GRID_REPORT_SHAPES) != 0)
		{
			lowest[at] = shape;
		}
		if ((flags & S2AMD_GRID_REPORT_OCCUPANCY) != 0)
		{
			occupancy[at] = shape >= 0 ? 1.0f : 0.0f;
		}
	}
	// the grid's counts: -1 is the largest unsigned value, so the minimum over "none" stays -1
	const int occupied = __popcll(__ballot(shape >= 0));
	uint32_t least = (uint32_t)shape;
	for (int d = 32; d > 0; d >>= 1)
	{
		const uint32_t other = (uint32_t)__shfl_xor((int)least, d);
		least = other < least ? other : least;
	}
	if (lane == 0)
	{
		s2amdGridState* st = states + g;
		if (occupied > 0)
		{
			atomicAdd(&st->occupied, occupied);
			atomicMin((unsigned int*)&st->lowestShape, least);
		}
		if (tile.first != 0)
		{
			st->candidates = candidates;
		}
	}
}

int gridCountOf(const s2amdSolver* s)
{
	return (int)s->hGridSensors.size();
}

size_t gridCellsOf(const s2amdSolver* s)
{
	return s->gridCells;
}

GridLayout layoutOf(const s2amdSolver* s)
{
	return gridLayout(gridCountOf(s), gridCellsOf(s), s->hGridTiles.size() / 4, s->shapeCapacity);
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->gridReport, s->hGridReportHead, sizeof(s->hGridReportHead), "grid-report", "s2amd_world_set_grid_report"} : ReportRef{};
}

// the tiles of the list, no tile across two grids: 8 x 8 blocks, row by row of blocks
void buildTiles(const std::vector<s2amdGridSensor>& grids, std::vector<int32_t>& tiles)
{
	tiles.clear();
	for (size_t g = 0; g < grids.size(); ++g)
	{
		int first = 1;
		for (int b = 0; b < grids[g].height; b += 8)
		{
			for (int a = 0; a < grids[g].width; a += 8)
			{
				const int32_t tile[4] = {(int32_t)g, a, b, first};
				tiles.insert(tiles.end(), tile, tile + 4);
				first = 0;
			}
		}
	}
}

// the list and its tiles into the block (waited for: the caller's next s2amd_world_set_grid_sensors replaces the vectors these copies read)
int gridReportStage(s2amdSolver* s)
{
	const int count = gridCountOf(s);
	const GridLayout l = layoutOf(s);
	if (count <= 0 || s->gridReport.block.p == nullptr || s->gridReport.block.bytes < l.total)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	char* base = (char*)s->gridReport.block.p;
	HIP_TRY(hipMemcpyAsync(base + l.grids, s->hGridSensors.data(), (size_t)count * sizeof(s2amdGridSensor), hipMemcpyHostToDevice, s->stream));
	HIP_TRY(hipMemcpyAsync(base + l.tiles, s->hGridTiles.data(), s->hGridTiles.size() * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

bool validGridSensor(const s2amdGridSensor& q)
{
	const bool finite = std::isfinite(q.position[0]) && std::isfinite(q.position[1]) && std::isfinite(q.rot[0]) && std::isfinite(q.rot[1]) && std::isfinite(q.cellSize);
	return finite && q.cellSize > 0.0f && q.width >= 1 && q.width <= S2AMD_MAX_GRID_SIDE && q.height >= 1 && q.height <= S2AMD_MAX_GRID_SIDE &&
		   (q.flags & ~S2_GRID_SENSOR_KNOWN_FLAGS) == 0;
}

} // namespace

int gridReportPrepare(s2amdSolver* s)
{
	if (!reportPrepareBegin(s, s->gridReport))
	{
		return S2AMD_OK;
	}
	const GridLayout l = layoutOf(s);
	const int rc = reportPrepareBlock(s->gridReport, l.total, l.head);
	return rc ? rc : gridReportStage(s);
}

int gridReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->gridReport;
	const int flags = r.flags;
	const int count = gridCountOf(s);
	const GridLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "grid"))
	{
		return rc;
	}
	if (count > 0)
	{
		char* base = (char*)r.block.p;
		hipStream_t st = s->stream;
		const s2amdShape* shapes = (const s2amdShape*)s->dShapes.p;
		const s2amdBody* bodies = (const s2amdBody*)s->dBodies.p;
		const float2* origins = (const float2*)s->dOrigins.p;
		const int ns = std::max(s->shapeCapacity, 0);
		const int tileCount = (int)(s->hGridTiles.size() / 4);
		PosedGrid* posed = (PosedGrid*)(base + l.posed);
		s2amdGridState* states = (s2amdGridState*)(base + l.states);
		unsigned long long* masks = (unsigned long long*)(base + l.masks);
		gridPoseKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const s2amdGridSensor*)(base + l.grids), count, bodies, origins, s->bodyCapacity, posed, states);
		if (l.shapeTiles > 0)
		{
			const int chunks = (count + S2_GRID_CHUNK - 1) / S2_GRID_CHUNK;
			gridCandidatesKernel<<<dim3((unsigned)l.shapeTiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(shapes, ns, l.shapeTiles, bodies, s->bodyCapacity, posed, count, masks);
		}
		const dim3 grid((unsigned)((tileCount + S2_BLOCK / 64 - 1) / (S2_BLOCK / 64)));
		gridRasterKernel<<<grid, dim3(S2_BLOCK), 0, st>>>(shapes, ns, bodies, origins, s->bodyCapacity, posed, (const GridTile*)(base + l.tiles), tileCount, masks, (int)l.words,
														  flags, (uint32_t*)(base + l.categories), (int32_t*)(base + l.shapes), (float*)(base + l.occupancy), states);
		HIP_TRY(hipGetLastError());
	}
	// (the counts are the list's: the head is known here, no getter fetches one)
	s->hGridReportHead[0] = (int32_t)gridCellsOf(s), s->hGridReportHead[1] = count, s->hGridReportHead[2] = s->hGridReportHead[3] = 0;
	r.stepFlags = flags;
	r.headKnown = true;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_grid_sensors(s2amdSolver* s, const s2amdGridSensor* grids, int32_t count)
{
	if (int rc = listArgs(s, grids, count, S2AMD_MAX_GRID_SENSORS))
	{
		return rc;
	}
	size_t cells = 0;
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validGridSensor(grids[i]) || (s->worldResident && grids[i].body >= s->bodyCapacity))
		{
			return fail(S2AMD_E_INVALID, "grid sensor " + std::to_string(i) +
											 " is invalid (width or height outside 1..256, a NaN or infinite field, cellSize <= 0, unknown flag bits, a body outside the body array)");
		}
		cells += (size_t)grids[i].width * (size_t)grids[i].height;
	}
	if (cells > (size_t)S2AMD_MAX_GRID_CELLS)
	{
		return fail(S2AMD_E_INVALID, "grid sensors: more than S2AMD_MAX_GRID_CELLS cells over the list");
	}
	// the last step's report is void; firstCell rides in the list's own copy (pad[0])
	std::vector<s2amdGridSensor> next(grids, grids + count);
	int32_t firstCell = 0;
	for (s2amdGridSensor& q : next)
	{
		memset(q.pad, 0, sizeof(q.pad));
		q.pad[0] = firstCell;
		firstCell += q.width * q.height;
	}
	std::vector<int32_t> nextTiles;
	buildTiles(next, nextTiles);
	const auto exchange = [&] {
		next.swap(s->hGridSensors);
		nextTiles.swap(s->hGridTiles);
		std::swap(cells, s->gridCells);
	};
	return listSwapIn(s, exchange, gridReportPrepare);
}

int s2amd_world_set_grid_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2_GRID_REPORT_KNOWN, gridReportPrepare);
}

int s2amd_world_grid_categories(s2amdSolver* s, uint32_t* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_GRID_REPORT_CATEGORIES, "s2amd_world_grid_categories", "grid category buffer too small", 0, s ? layoutOf(s).categories : 0,
						 sizeof(uint32_t), out, capacity, count);
}

int s2amd_world_grid_shapes(s2amdSolver* s, int32_t* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_GRID_REPORT_SHAPES, "s2amd_world_grid_shapes", "grid shape buffer too small", 0, s ? layoutOf(s).shapes : 0, sizeof(int32_t), out,
						 capacity, count);
}

int s2amd_world_grid_occupancy(s2amdSolver* s, float* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_GRID_REPORT_OCCUPANCY, "s2amd_world_grid_occupancy", "grid occupancy buffer too small", 0, s ? layoutOf(s).occupancy : 0, sizeof(float),
						 out, capacity, count);
}

int s2amd_world_export_grid_occupancy(s2amdSolver* s, void* deviceCells, int32_t capacity)
{
	if (!s || capacity < 0 || (capacity > 0 && !deviceCells))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	const int rc = reportHeadFor(ref(s), S2AMD_GRID_REPORT_OCCUPANCY, "s2amd_world_export_grid_occupancy");
	if (rc)
	{
		return rc;
	}
	const int32_t cells = s->hGridReportHead[0];
	if (cells > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "device occupancy buffer too small");
	}
	return reportCopyOut(s, deviceCells, s->gridReport.block, layoutOf(s).occupancy, cells, sizeof(float), hipMemcpyDeviceToDevice);
}

int s2amd_world_grid_states(s2amdSolver* s, s2amdGridState* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_GRID_REPORT_STATES, "s2amd_world_grid_states", "grid state buffer too small", 1, s ? layoutOf(s).states : 0, sizeof(s2amdGridState), out,
						 capacity, count);
}

} // extern "C"
#pragma GCC visibility pop
