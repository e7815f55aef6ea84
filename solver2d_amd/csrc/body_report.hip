// Body report of the resident world (include/solver2d_amd.h: s2amd_world_set_body_report, s2amd_world_set_rest_thresholds and the four
// getters): velocities, which poses changed, which bodies came to rest or woke up, and the islands of the world as it stands -- compacted
// on the device behind stage 4 of s2amd_world_step and behind the shape report, instead of derived on the host from a download of bodies,
// origins, contacts and joints.  The reference has no sleeping: the report says who is at rest, the solve skips nobody.  The shape is
// shape_report.hip's, with a union-find in the manner of structure.hip between the two passes:
//
//   bodyCountKernel        one pass over the body slots in tiles of 256.  Compares {origin, rot} with the report's copy from before the
//                          step and refreshes the copy; advances the body's rest timer; leaves {at rest now, at rest before, moved,
//                          reported} in the report's own state byte; per-tile counts of the three lists by wave ballots and one partial
//                          per tile for s2amdBodySummary.  Under ISLANDS it also makes every slot its own union-find root and clears the
//                          slot's island sums.
//   bodyHookKernel         (ISLANDS) one lane per contact / joint slot: a touching contact or a revolute joint between two movable bodies
//                          hooks the higher root under the lower by CAS, so a component's root is its lowest slot whatever the
//                          interleaving: the labels are a pure function of the arrays.
//   bodyIslandSumKernel    (ISLANDS) body tiles: label[i] = root, the tile's count of roots, and the island's sums -- bodies, bodies at
//                          rest (integer adds), the minimum timer (a non-negative float: its bits compared as uint32) and the fastest
//                          body as max of (speedSquared bits << 32) | (0xFFFFFFFF - slot); edge tiles: the contact and joint counts.
//                          Nothing here depends on the order of execution and there is no floating-point atomic.  Inside a wave, runs
//                          of consecutive lanes with the same label are combined first and only a run's first lane goes to memory:
//                          neighbouring slots usually share an island (at base 200 all 20,000 bodies do), so a wave issues one set of
//                          atomics, not 64.
//   bodyIslandWriteKernel  (ISLANDS) the same body tiles: a root's index is the number of roots below it (tileCountsBefore + ballot
//                          rank), its s2amdIslandState goes to that place, and the tile leaves a partial for the summary.
//   bodyWriteKernel        the same tiles: every tile adds up the counts of the tiles before it and writes its entries at their ranks:
//                          three ascending lists without a sort or an atomic.  A record is one 64-byte line, built in the tile's LDS
//                          image at its rank (16-byte chunks XOR-swizzled by the rank) and stored 1 KiB per wave instruction, whole
//                          lines only.  The fourth wave of the last tile reduces the partials to the summary.
//
// "At rest before the step" is the timer as it stood before the step against `seconds` as it is now: what a pass that re-evaluated stored
// bits after s2amd_world_set_rest_thresholds would leave, without the stored bits and without the pass.  The state is the report's own and
// the passes are enqueued once per step, behind the attempt that stands: a repeated step reports once.  All device memory is one block
// sized by bodyReportPrepare; a step allocates nothing and waits for nothing -- the getters do.
#include "report_common.h"

#include <cmath>

namespace
{

#define S2_BODY_NOW 1	   // state byte: at rest after this step
#define S2_BODY_BEFORE 2   // ... before it
#define S2_BODY_MOVED 4	   // the pose differs from the copy
#define S2_BODY_REPORTED 8 // neither free nor static

static_assert(sizeof(s2amdBodyState) == 64 && sizeof(s2amdIslandState) == 32 && sizeof(s2amdBodySummary) == 64, "the report's records");
static_assert(S2AMD_BODY_STATE_AT_REST == 2 * S2_BODY_NOW && S2AMD_BODY_STATE_MOVED == 1, "the record's flags");

typedef unsigned long long u64;

struct RestRule
{
	float lin2, ang2, seconds, dt;
};

// what one tile of the count pass contributes to s2amdBodySummary
struct BodyTilePartial
{
	int32_t reported, dynamic, kinematic, moved, resting, pad;
	u64 fastest;
};
static_assert(sizeof(BodyTilePartial) == 32, "two per line");

// ... and one tile of the island write pass
struct IslandTilePartial
{
	int32_t resting, pad;
	u64 largest; // (bodyCount << 32) | (0xFFFFFFFF - index); 0: no island
};
static_assert(sizeof(IslandTilePartial) == 16, "four per line");

// the sums of the island whose root is this slot
struct IslandSums
{
	int32_t bodies, resting, contacts, joints;
	uint32_t minRest; // bits of the minimum timer
	int32_t pad;
	u64 fastest; // (speedSquared bits << 32) | (0xFFFFFFFF - slot); 0: every speed a NaN
};
static_assert(sizeof(IslandSums) == 32, "two 16-byte stores clear it");

// the head of the report as the getters fetch it (solver_internal.h: hBodyReportHead)
struct BodyReportHead
{
	int32_t counts[4]; // {records, rested, woke, islands}
	s2amdBodySummary summary;
};

struct BodyReportLayout
{
	size_t pose, timer, state, parent, label, islandIndex, sums, counts, partials, islandPartials, head, rested, woke, records, islands, total;
	int tiles;
};

BodyReportLayout bodyReportLayout(int nb)
{
	BodyReportLayout l{};
	size_t at = 0;
	l.tiles = (nb + S2_BLOCK - 1) / S2_BLOCK;
	l.pose = reportTake(at, (size_t)nb * sizeof(uint4));
	l.timer = reportTake(at, (size_t)nb * sizeof(float));
	l.state = reportTake(at, (size_t)nb);
	l.parent = reportTake(at, (size_t)nb * sizeof(int));
	l.label = reportTake(at, (size_t)nb * sizeof(int));
	l.islandIndex = reportTake(at, (size_t)nb * sizeof(int));
	l.sums = reportTake(at, (size_t)nb * sizeof(IslandSums));
	l.counts = reportTake(at, (size_t)4 * l.tiles * sizeof(int));
	l.partials = reportTake(at, (size_t)l.tiles * sizeof(BodyTilePartial));
	l.islandPartials = reportTake(at, (size_t)l.tiles * sizeof(IslandTilePartial));
	l.head = reportTake(at, sizeof(BodyReportHead));
	l.rested = reportTake(at, (size_t)nb * sizeof(int32_t));
	l.woke = reportTake(at, (size_t)nb * sizeof(int32_t));
	l.records = reportTake(at, (size_t)nb * sizeof(s2amdBodyState));
	l.islands = reportTake(at, (size_t)nb * sizeof(s2amdIslandState));
	l.total = at;
	return l;
}

S2_DEV bool reportedType(int type) { return type != S2AMD_BODY_FREE && type != S2AMD_BODY_STATIC; }

// the key of "fastest": larger speed first, of equal speeds the lower slot; 0 for a NaN, which never wins (speedSquared is never negative)
S2_DEV u64 fastestKey(float speedSquared, int slot)
{
	if (!(speedSquared == speedSquared))
	{
		return 0ull;
	}
	return ((u64)__float_as_uint(speedSquared) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)slot);
}

S2_DEV u64 maxOverWave(u64 v)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const u64 other = __shfl_xor(v, d);
		v = other > v ? other : v;
	}
	return v;
}

S2_DEV uint4 poseOf(const s2amdBody& b, float2 origin)
{
	return make_uint4(__float_as_uint(origin.x), __float_as_uint(origin.y), __float_as_uint(b.rot[0]), __float_as_uint(b.rot[1]));
}

// the copy of the poses as the bodies stand, every timer at +0
__global__ __launch_bounds__(S2_BLOCK) void bodyInitKernel(const s2amdBody* bodies, const float2* origins, int n, uint4* pose, float* timer, uint8_t* state)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n)
	{
		pose[i] = poseOf(bodies[i], origins[i]);
		timer[i] = 0.0f;
		state[i] = 0;
	}
}

// counts[0..tiles) reported (or moved, under MOVED_ONLY), [tiles..2 tiles) rested, [2 tiles..3 tiles) woke, [3 tiles..4 tiles) zero here
// (the island pass fills it); partials[tile]; state[i]; pose[i] and timer[i] advanced.
// Reads per slot 44 bytes of the body, its origin, its pose copy and its timer.
__global__ __launch_bounds__(S2_BLOCK) void bodyCountKernel(const s2amdBody* bodies, const float2* origins, int n, int tiles, RestRule rule, int flags, uint4* pose,
															float* timer, uint8_t* state, int* counts, BodyTilePartial* partials, int* parent, IslandSums* sums)
{
	__shared__ int waves[8][S2_BLOCK / 64];
	__shared__ u64 waveFastest[S2_BLOCK / 64];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	bool reported = false, moved = false, now = false, before = false;
	int type = S2AMD_BODY_FREE;
	u64 key = 0ull;
	if (i < n)
	{
		const s2amdBody& b = bodies[i];
		type = b.type;
		reported = reportedType(type);
		const uint4 cur = poseOf(b, origins[i]);
		const uint4 old = pose[i];
		pose[i] = cur;
		if (reported)
		{
			moved = cur.x != old.x || cur.y != old.y || cur.z != old.z || cur.w != old.w;
			const float vx = b.linearVelocity[0], vy = b.linearVelocity[1], w = b.angularVelocity;
			const float speedSquared = vx * vx + vy * vy;
			const float ww = w * w;
			const bool candidate = speedSquared <= rule.lin2 && ww <= rule.ang2;
			const float t = timer[i];
			before = t >= rule.seconds;
			const float next = candidate ? t + rule.dt : 0.0f;
			timer[i] = next;
			now = next >= rule.seconds;
			key = fastestKey(speedSquared, i);
		}
		state[i] = (uint8_t)((now ? S2_BODY_NOW : 0) | (before ? S2_BODY_BEFORE : 0) | (moved ? S2_BODY_MOVED : 0) | (reported ? S2_BODY_REPORTED : 0));
		if ((flags & S2AMD_BODY_REPORT_ISLANDS) != 0)
		{
			parent[i] = i;
			uint4* clear = (uint4*)(sums + i);
			clear[0] = make_uint4(0u, 0u, 0u, 0u);
			clear[1] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
		}
	}
	const bool listed = reported && ((flags & S2AMD_BODY_REPORT_MOVED_ONLY) == 0 || moved);
	const int nListed = __popcll(__ballot(listed));
	const int nRested = __popcll(__ballot(now && !before)), nWoke = __popcll(__ballot(before && !now));
	const int nReported = __popcll(__ballot(reported)), nMoved = __popcll(__ballot(moved)), nResting = __popcll(__ballot(now));
	const int nDynamic = __popcll(__ballot(type == S2AMD_BODY_DYNAMIC)), nKinematic = __popcll(__ballot(type == S2AMD_BODY_KINEMATIC));
	key = maxOverWave(key);
	if (lane == 0)
	{
		waves[0][wave] = nListed, waves[1][wave] = nRested, waves[2][wave] = nWoke, waves[3][wave] = nReported;
		waves[4][wave] = nDynamic, waves[5][wave] = nKinematic, waves[6][wave] = nMoved, waves[7][wave] = nResting;
		waveFastest[wave] = key;
	}
	__syncthreads();
	if (threadIdx.x < 7)
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
			partials[blockIdx.x].reported = total;
		}
		else if (threadIdx.x == 4)
		{
			partials[blockIdx.x].dynamic = total;
		}
		else if (threadIdx.x == 5)
		{
			partials[blockIdx.x].kinematic = total;
		}
		else
		{
			partials[blockIdx.x].moved = total;
		}
	}
	else if (threadIdx.x == 7)
	{
		int total = 0;
		u64 best = 0ull;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			total += waves[7][w];
			best = waveFastest[w] > best ? waveFastest[w] : best;
		}
		partials[blockIdx.x].resting = total;
		partials[blockIdx.x].pad = 0;
		partials[blockIdx.x].fastest = best;
		counts[3 * tiles + (int)blockIdx.x] = 0;
	}
}

// ---- islands: structure.hip's lock-free union-find on the resident arrays ----
// Reads go through agent-scope atomics: another CU's hook must become visible inside this launch, and a CU's vector L1 is never refreshed
// by other CUs' stores.
S2_DEV int loadParent(int* parent, int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

S2_DEV int findRoot(int* parent, int i)
{
	int p = loadParent(parent, i);
	while (p != i)
	{
		const int gp = loadParent(parent, p);
		if (gp != p)
		{
			// path halving: a benign race, every value written is an ancestor of i
			__hip_atomic_store(parent + i, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		i = p;
		p = gp;
	}
	return i;
}

S2_DEV void hook(int* parent, int a, int b)
{
	for (;;)
	{
		const int ra = findRoot(parent, a), rb = findRoot(parent, b);
		if (ra == rb)
		{
			return;
		}
		const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
		// hi is a root only while parent[hi] == hi
		if (atomicCAS(&parent[hi], hi, lo) == hi)
		{
			return;
		}
	}
}

// a reported body the solve can move; a slot outside the array is none
S2_DEV bool movableSlot(const s2amdBody* bodies, int nb, int slot)
{
	if (slot < 0 || slot >= nb)
	{
		return false;
	}
	const s2amdBody& b = bodies[slot];
	return reportedType(b.type) && (b.invMass != 0.0f || b.invI != 0.0f);
}

__global__ __launch_bounds__(S2_BLOCK) void bodyHookKernel(const s2amdBody* bodies, int nb, const s2amdContact* contacts, int nc, const s2amdJoint* joints, int nj,
														   int* parent)
{
	const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	int a = -1, b = -1;
	if (e < nc)
	{
		if (contacts[e].pointCount > 0)
		{
			a = contacts[e].bodyA, b = contacts[e].bodyB;
		}
	}
	else if (e < nc + nj)
	{
		const s2amdJoint& j = joints[e - nc];
		if (j.type == S2AMD_JOINT_REVOLUTE)
		{
			a = j.bodyA, b = j.bodyB;
		}
	}
	if (movableSlot(bodies, nb, a) && movableSlot(bodies, nb, b))
	{
		hook(parent, a, b);
	}
}

// The runs of consecutive lanes with the same label: `run` numbers them along the wave, `first` marks a run's first lane.
struct WaveRuns
{
	int run;
	bool first;
};

S2_DEV WaveRuns waveRuns(int label, int lane)
{
	const int below = __shfl_up(label, 1);
	WaveRuns r;
	r.first = lane == 0 || below != label;
	r.run = __popcll(__ballot(r.first) & ((2ull << lane) - 1ull));
	return r;
}

// after the loop a run's first lane holds the run's sum / minimum / maximum: a lane takes what the lane d above it holds while that lane
// is of its own run (runs are consecutive, so everything between is as well)
S2_DEV int runSum(int v, int run, int lane)
{
	for (int d = 1; d < 64; d <<= 1)
	{
		const int other = __shfl_down(v, d), otherRun = __shfl_down(run, d);
		if (lane + d < 64 && otherRun == run)
		{
			v += other;
		}
	}
	return v;
}

S2_DEV uint32_t runMin(uint32_t v, int run, int lane)
{
	for (int d = 1; d < 64; d <<= 1)
	{
		const uint32_t other = __shfl_down(v, d);
		const int otherRun = __shfl_down(run, d);
		if (lane + d < 64 && otherRun == run)
		{
			v = other < v ? other : v;
		}
	}
	return v;
}

S2_DEV u64 runMax(u64 v, int run, int lane)
{
	for (int d = 1; d < 64; d <<= 1)
	{
		const u64 other = __shfl_down(v, d);
		const int otherRun = __shfl_down(run, d);
		if (lane + d < 64 && otherRun == run)
		{
			v = other > v ? other : v;
		}
	}
	return v;
}

// Blocks [0, tiles): the body slots.  label[i] = the root of a reported body, -1 otherwise; counts[3 tiles + tile] = the tile's roots;
// sums[root] += the body.  Blocks [tiles, ...): the contact and joint slots, sums[root].contacts / .joints.
__global__ __launch_bounds__(S2_BLOCK) void bodyIslandSumKernel(const s2amdBody* bodies, int nb, int tiles, const s2amdContact* contacts, int nc, const s2amdJoint* joints,
																int nj, const uint8_t* state, const float* timer, int* parent, int* label, int* counts, IslandSums* sums)
{
	__shared__ int waveRoots[S2_BLOCK / 64];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	if ((int)blockIdx.x < tiles)
	{
		const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
		int root = -1, resting = 0;
		uint32_t rest = 0xFFFFFFFFu;
		u64 key = 0ull;
		if (i < nb)
		{
			const int st = state[i];
			if ((st & S2_BODY_REPORTED) != 0)
			{
				root = findRoot(parent, i);
				resting = (st & S2_BODY_NOW) != 0 ? 1 : 0;
				rest = __float_as_uint(timer[i]);
				const float vx = bodies[i].linearVelocity[0], vy = bodies[i].linearVelocity[1];
				key = fastestKey(vx * vx + vy * vy, i);
			}
			label[i] = root;
		}
		const int nRoots = __popcll(__ballot(root >= 0 && root == i));
		if (lane == 0)
		{
			waveRoots[wave] = nRoots;
		}
		const WaveRuns r = waveRuns(root, lane);
		const int nBodies = runSum(root >= 0 ? 1 : 0, r.run, lane), nResting = runSum(resting, r.run, lane);
		rest = runMin(rest, r.run, lane);
		key = runMax(key, r.run, lane);
		if (r.first && root >= 0)
		{
			IslandSums* s = sums + root;
			atomicAdd(&s->bodies, nBodies);
			if (nResting != 0)
			{
				atomicAdd(&s->resting, nResting);
			}
			atomicMin(&s->minRest, rest);
			if (key != 0ull)
			{
				atomicMax(&s->fastest, key);
			}
		}
		__syncthreads();
		if (threadIdx.x == 0)
		{
			counts[3 * tiles + (int)blockIdx.x] = waveRoots[0] + waveRoots[1] + waveRoots[2] + waveRoots[3];
		}
		return;
	}
	const int e = (int)(((int)blockIdx.x - tiles) * (int)blockDim.x + (int)threadIdx.x);
	int owner = -1, isContact = 0, isJoint = 0;
	if (e < nc)
	{
		if (contacts[e].pointCount > 0)
		{
			const int a = contacts[e].bodyA, b = contacts[e].bodyB;
			owner = movableSlot(bodies, nb, a) ? a : movableSlot(bodies, nb, b) ? b : -1;
			isContact = 1;
		}
	}
	else if (e < nc + nj)
	{
		const s2amdJoint& j = joints[e - nc];
		if (j.type != S2AMD_JOINT_FREE)
		{
			const int a = j.type == S2AMD_JOINT_REVOLUTE ? j.bodyA : -1, b = j.bodyB;
			owner = movableSlot(bodies, nb, a) ? a : movableSlot(bodies, nb, b) ? b : -1;
			isJoint = 1;
		}
	}
	const int root = owner >= 0 ? findRoot(parent, owner) : -1;
	const WaveRuns r = waveRuns(root, lane);
	const int nContacts = runSum(root >= 0 ? isContact : 0, r.run, lane), nJoints = runSum(root >= 0 ? isJoint : 0, r.run, lane);
	if (r.first && root >= 0)
	{
		if (nContacts != 0)
		{
			atomicAdd(&sums[root].contacts, nContacts);
		}
		if (nJoints != 0)
		{
			atomicAdd(&sums[root].joints, nJoints);
		}
	}
}

S2_DEV s2amdIslandState islandOf(int root, const IslandSums& s)
{
	s2amdIslandState r;
	r.firstBody = root, r.bodyCount = s.bodies, r.contactCount = s.contacts, r.jointCount = s.joints, r.restingBodies = s.resting;
	r.fastestBody = s.fastest != 0ull ? (int)(0xFFFFFFFFu - (uint32_t)s.fastest) : -1;
	r.maxSpeedSquared = s.fastest != 0ull ? __uint_as_float((uint32_t)(s.fastest >> 32)) : -1.0f;
	r.minRestTime = __uint_as_float(s.minRest);
	return r;
}

// islandIndex[root] = its place in the list; islands[place]; islandPartials[tile]
__global__ __launch_bounds__(S2_BLOCK) void bodyIslandWriteKernel(const int* label, int nb, int tiles, const int* counts, const IslandSums* sums, int* islandIndex,
																  s2amdIslandState* islands, IslandTilePartial* islandPartials)
{
	__shared__ int waveRoots[S2_BLOCK / 64], waveResting[S2_BLOCK / 64];
	__shared__ u64 waveLargest[S2_BLOCK / 64];
	__shared__ int base;
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const bool isRoot = i < nb && label[i] == i;
	const unsigned long long rootMask = __ballot(isRoot);
	IslandSums s{};
	if (isRoot)
	{
		s = sums[i];
	}
	const bool resting = isRoot && s.resting == s.bodies;
	const int nResting = __popcll(__ballot(resting));
	if (lane == 0)
	{
		waveRoots[wave] = __popcll(rootMask), waveResting[wave] = nResting;
	}
	if (wave == 0)
	{
		int partial = tileCountsBefore(counts, tiles, 3, (int)blockIdx.x, lane);
		for (int d = 32; d > 0; d >>= 1)
		{
			partial += __shfl_xor(partial, d);
		}
		if (lane == 0)
		{
			base = partial;
		}
	}
	__syncthreads();
	int index = base;
	for (int w = 0; w < wave; ++w)
	{
		index += waveRoots[w];
	}
	index += __popcll(rootMask & ((1ull << lane) - 1ull));
	u64 largest = 0ull;
	if (isRoot)
	{
		islandIndex[i] = index;
		const s2amdIslandState r = islandOf(i, s);
		uint4* out = (uint4*)(islands + index);
		out[0] = make_uint4((uint32_t)r.firstBody, (uint32_t)r.bodyCount, (uint32_t)r.contactCount, (uint32_t)r.jointCount);
		out[1] = make_uint4((uint32_t)r.restingBodies, (uint32_t)r.fastestBody, __float_as_uint(r.maxSpeedSquared), __float_as_uint(r.minRestTime));
		largest = ((u64)(uint32_t)s.bodies << 32) | (u64)(0xFFFFFFFFu - (uint32_t)index);
	}
	largest = maxOverWave(largest);
	if (lane == 0)
	{
		waveLargest[wave] = largest;
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		IslandTilePartial p;
		p.resting = waveResting[0] + waveResting[1] + waveResting[2] + waveResting[3], p.pad = 0;
		p.largest = 0ull;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			p.largest = waveLargest[w] > p.largest ? waveLargest[w] : p.largest;
		}
		islandPartials[blockIdx.x] = p;
	}
}

// One record into the tile's LDS image at rank r: chunk c (16 bytes) of the record is slot r * 4 + (c ^ (r & 3)) of the image
S2_DEV void stageChunk(float4* image, int r, int c, float4 v)
{
	image[r * 4 + (c ^ (r & 3))] = v;
}

// head->counts = {records, rested, woke, islands} of the step, head->summary; `flags`: which lists are wanted.
// Reads per slot its state byte; under STATES per listed body 28 bytes of the body, its origin and timer (and under ISLANDS its label, the
// root's index and 8 bytes of the root's sums), and writes one full 64-byte line; 4 bytes per event.
__global__ __launch_bounds__(S2_BLOCK) void bodyWriteKernel(const s2amdBody* bodies, const float2* origins, int n, int tiles, const uint8_t* state, const float* timer,
															const int* counts, const BodyTilePartial* partials, const IslandTilePartial* islandPartials, const int* label,
															const int* islandIndex, const IslandSums* sums, int flags, BodyReportHead* head, int32_t* restedOut,
															int32_t* wokeOut, float4* records)
{
	__shared__ float4 image[S2_BLOCK * 4]; // 256 records of 64 bytes
	__shared__ int waves[3][S2_BLOCK / 64];
	__shared__ int base[3];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	int st = 0;
	if (i < n)
	{
		st = state[i];
	}
	const bool now = (st & S2_BODY_NOW) != 0, before = (st & S2_BODY_BEFORE) != 0, moved = (st & S2_BODY_MOVED) != 0;
	const bool listed = (st & S2_BODY_REPORTED) != 0 && ((flags & S2AMD_BODY_REPORT_MOVED_ONLY) == 0 || moved);
	const bool rested = now && !before, woke = before && !now;
	const unsigned long long listedMask = __ballot(listed), restedMask = __ballot(rested), wokeMask = __ballot(woke);
	if (lane == 0)
	{
		waves[0][wave] = __popcll(listedMask), waves[1][wave] = __popcll(restedMask), waves[2][wave] = __popcll(wokeMask);
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
		const bool withIslands = (flags & S2AMD_BODY_REPORT_ISLANDS) != 0;
		const int run = (tiles + 63) / 64;
		int nReported = 0, nDynamic = 0, nKinematic = 0, nMoved = 0, nResting = 0, nIslands = 0, nRestingIslands = 0;
		u64 fastest = 0ull, largest = 0ull;
		for (int b = lane * run; b < (lane + 1) * run && b < tiles; ++b)
		{
			const BodyTilePartial p = partials[b];
			nReported += p.reported, nDynamic += p.dynamic, nKinematic += p.kinematic, nMoved += p.moved, nResting += p.resting;
			fastest = p.fastest > fastest ? p.fastest : fastest;
			if (withIslands)
			{
				const IslandTilePartial q = islandPartials[b];
				nIslands += counts[3 * tiles + b];
				nRestingIslands += q.resting;
				largest = q.largest > largest ? q.largest : largest;
			}
		}
		for (int d = 32; d > 0; d >>= 1)
		{
			nReported += __shfl_xor(nReported, d), nDynamic += __shfl_xor(nDynamic, d), nKinematic += __shfl_xor(nKinematic, d);
			nMoved += __shfl_xor(nMoved, d), nResting += __shfl_xor(nResting, d);
			nIslands += __shfl_xor(nIslands, d), nRestingIslands += __shfl_xor(nRestingIslands, d);
		}
		fastest = maxOverWave(fastest), largest = maxOverWave(largest);
		if (lane == 0)
		{
			s2amdBodySummary s{};
			s.bodies = nReported, s.dynamicBodies = nDynamic, s.kinematicBodies = nKinematic, s.movedBodies = nMoved, s.restingBodies = nResting;
			s.islands = nIslands, s.restingIslands = nRestingIslands;
			s.largestIsland = largest != 0ull ? (int)(0xFFFFFFFFu - (uint32_t)largest) : -1;
			s.largestIslandBodies = (int)(uint32_t)(largest >> 32);
			s.fastestBody = fastest != 0ull ? (int)(0xFFFFFFFFu - (uint32_t)fastest) : -1;
			s.maxSpeedSquared = fastest != 0ull ? __uint_as_float((uint32_t)(fastest >> 32)) : -1.0f;
			head->summary = s;
			head->counts[3] = nIslands;
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
	tileRank += __popcll(listedMask & lower);
	at[1] += __popcll(restedMask & lower);
	at[2] += __popcll(wokeMask & lower);
	if ((int)blockIdx.x == tiles - 1 && threadIdx.x == blockDim.x - 1)
	{
		head->counts[0] = at[0] + tileRank + (listed ? 1 : 0);
		head->counts[1] = at[1] + (rested ? 1 : 0);
		head->counts[2] = at[2] + (woke ? 1 : 0);
	}
	if ((flags & S2AMD_BODY_REPORT_REST) != 0)
	{
		if (rested)
		{
			restedOut[at[1]] = i;
		}
		if (woke)
		{
			wokeOut[at[2]] = i;
		}
	}
	if ((flags & S2AMD_BODY_REPORT_STATES) == 0)
	{
		return; // (the whole block: `flags` is the launch's)
	}
	if (listed)
	{
		// (`listed` implies i < n)
		const s2amdBody& b = bodies[i];
		const float2 origin = origins[i];
		const float vx = b.linearVelocity[0], vy = b.linearVelocity[1];
		const float speedSquared = vx * vx + vy * vy;
		int island = -1, recordFlags = (moved ? S2AMD_BODY_STATE_MOVED : 0) | (now ? S2AMD_BODY_STATE_AT_REST : 0);
		if ((flags & S2AMD_BODY_REPORT_ISLANDS) != 0)
		{
			const int root = label[i]; // (a reported body has one, inside the array)
			island = islandIndex[root];
			recordFlags |= sums[root].resting == sums[root].bodies ? S2AMD_BODY_STATE_ISLAND_AT_REST : 0;
		}
		stageChunk(image, tileRank, 0, make_float4(__int_as_float(i), __int_as_float(b.type), __int_as_float(island), __int_as_float(recordFlags)));
		stageChunk(image, tileRank, 1, make_float4(origin.x, origin.y, b.position[0], b.position[1]));
		stageChunk(image, tileRank, 2, make_float4(b.rot[0], b.rot[1], s2_atan2f(b.rot[0], b.rot[1]), b.angularVelocity));
		stageChunk(image, tileRank, 3, make_float4(vx, vy, timer[i], speedSquared));
	}
	__syncthreads();
	// the tile's records are consecutive in the list: chunk g of the image goes to chunk g behind the tile's first record
	float4* out = records + (size_t)at[0] * 4;
	for (int g = (int)threadIdx.x; g < tileRecords * 4; g += S2_BLOCK)
	{
		const int r = g >> 2, c = g & 3;
		out[g] = image[r * 4 + (c ^ (r & 3))];
	}
}

BodyReportLayout layoutOf(const s2amdSolver* s)
{
	return bodyReportLayout(s->bodyCapacity);
}

ReportRef ref(s2amdSolver* s)
{
	static_assert(sizeof(s->hBodyReportHead) == sizeof(BodyReportHead), "the host copy of the report's head");
	return s ? ReportRef{s, &s->bodyReport, &s->hBodyReportHead, sizeof(s->hBodyReportHead), "body-report", "s2amd_world_set_body_report"} : ReportRef{};
}

// where a piece of the block lies, for a getter (0 for the null solver it will refuse)
size_t at(const s2amdSolver* s, size_t BodyReportLayout::*piece)
{
	return s ? layoutOf(s).*piece : 0;
}

} // namespace

int bodyReportPrepare(s2amdSolver* s)
{
	ReportState& r = s->bodyReport;
	if (!reportPrepareBegin(s, r))
	{
		return S2AMD_OK;
	}
	const int nb = s->bodyCapacity;
	const BodyReportLayout l = layoutOf(s);
	int rc = reportPrepareBlock(r, l.total, l.head);
	if (rc)
	{
		return rc;
	}
	if (nb > 0)
	{
		HIP_TRY(hipSetDevice(s->device));
		char* base = (char*)r.block.p;
		bodyInitKernel<<<gridFor((size_t)nb), dim3(S2_BLOCK), 0, s->stream>>>((const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, nb, (uint4*)(base + l.pose),
																			  (float*)(base + l.timer), (uint8_t*)(base + l.state));
		HIP_TRY(hipGetLastError());
	}
	return S2AMD_OK;
}

int bodyReportEnqueue(s2amdSolver* s, const s2amdStepParams* params)
{
	ReportState& r = s->bodyReport;
	const int flags = r.flags;
	const int nb = s->bodyCapacity;
	const BodyReportLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "body"))
	{
		return rc;
	}
	if (nb > 0)
	{
		hipStream_t st = s->stream;
		char* base = (char*)r.block.p;
		const s2amdBody* bodies = (const s2amdBody*)s->dBodies.p;
		const float2* origins = (const float2*)s->dOrigins.p;
		const s2amdContact* contacts = (const s2amdContact*)s->dContacts.p;
		const s2amdJoint* joints = (const s2amdJoint*)s->dJoints.p;
		const int nc = s->contactCapacity, nj = s->jointCapacity;
		RestRule rule;
		rule.lin2 = s->restLinearSpeed * s->restLinearSpeed, rule.ang2 = s->restAngularSpeed * s->restAngularSpeed;
		rule.seconds = s->restSeconds, rule.dt = params->dt;
		uint8_t* state = (uint8_t*)(base + l.state);
		float* timer = (float*)(base + l.timer);
		int* counts = (int*)(base + l.counts);
		int* parent = (int*)(base + l.parent);
		int* label = (int*)(base + l.label);
		int* islandIndex = (int*)(base + l.islandIndex);
		IslandSums* sums = (IslandSums*)(base + l.sums);
		const dim3 tiles((unsigned)l.tiles), block(S2_BLOCK);
		bodyCountKernel<<<tiles, block, 0, st>>>(bodies, origins, nb, l.tiles, rule, flags, (uint4*)(base + l.pose), timer, state, counts,
												 (BodyTilePartial*)(base + l.partials), parent, sums);
		if ((flags & S2AMD_BODY_REPORT_ISLANDS) != 0)
		{
			const size_t edges = (size_t)nc + (size_t)nj;
			if (edges > 0)
			{
				bodyHookKernel<<<gridFor(edges), block, 0, st>>>(bodies, nb, contacts, nc, joints, nj, parent);
			}
			bodyIslandSumKernel<<<dim3((unsigned)l.tiles + gridFor(edges).x), block, 0, st>>>(bodies, nb, l.tiles, contacts, nc, joints, nj, state, timer, parent, label,
																							  counts, sums);
			bodyIslandWriteKernel<<<tiles, block, 0, st>>>(label, nb, l.tiles, counts, sums, islandIndex, (s2amdIslandState*)(base + l.islands),
														   (IslandTilePartial*)(base + l.islandPartials));
		}
		bodyWriteKernel<<<tiles, block, 0, st>>>(bodies, origins, nb, l.tiles, state, timer, counts, (const BodyTilePartial*)(base + l.partials),
												 (const IslandTilePartial*)(base + l.islandPartials), label, islandIndex, sums, flags, (BodyReportHead*)(base + l.head),
												 (int32_t*)(base + l.rested), (int32_t*)(base + l.woke), (float4*)(base + l.records));
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (a world without body slots launches no tile: its head is known here)
		s->hBodyReportHead = {};
		s->hBodyReportHead.summary.largestIsland = -1, s->hBodyReportHead.summary.fastestBody = -1;
		s->hBodyReportHead.summary.maxSpeedSquared = -1.0f;
	}
	r.stepFlags = flags;
	r.headKnown = nb <= 0;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_body_report(s2amdSolver* s, int32_t flags)
{
	// (the pose copy is of the bodies as they stand, the timers start at +0)
	return reportSet(ref(s), flags, S2AMD_BODY_REPORT_STATES | S2AMD_BODY_REPORT_REST | S2AMD_BODY_REPORT_ISLANDS | S2AMD_BODY_REPORT_MOVED_ONLY, bodyReportPrepare);
}

int s2amd_world_set_rest_thresholds(s2amdSolver* s, float linearSpeed, float angularSpeed, float seconds)
{
	if (!s)
	{
		return fail(S2AMD_E_INVALID, "null solver");
	}
	// (written so that a NaN fails it)
	if (!(linearSpeed >= 0.0f) || !(angularSpeed >= 0.0f) || !(seconds >= 0.0f))
	{
		return fail(S2AMD_E_INVALID, "rest thresholds: a negative value or a NaN");
	}
	// "at rest before" of the next step is the kept timers against these values (bodyCountKernel): the change itself is no event
	s->restLinearSpeed = linearSpeed, s->restAngularSpeed = angularSpeed, s->restSeconds = seconds;
	return S2AMD_OK;
}

int s2amd_world_body_states(s2amdSolver* s, s2amdBodyState* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_BODY_REPORT_STATES, "s2amd_world_body_states", "body-state buffer too small", 0, at(s, &BodyReportLayout::records), sizeof(*out), out, capacity,
						 count);
}

int s2amd_world_body_rest_events(s2amdSolver* s, int32_t* rested, int32_t restedCapacity, int32_t* restedCount, int32_t* woke, int32_t wokeCapacity, int32_t* wokeCount)
{
	return reportGetEvents(ref(s), S2AMD_BODY_REPORT_REST, "s2amd_world_body_rest_events", "body rest event buffer too small", 1, at(s, &BodyReportLayout::rested),
						   at(s, &BodyReportLayout::woke), rested, restedCapacity, restedCount, woke, wokeCapacity, wokeCount);
}

int s2amd_world_islands(s2amdSolver* s, s2amdIslandState* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_BODY_REPORT_ISLANDS, "s2amd_world_islands", "island buffer too small", 3, at(s, &BodyReportLayout::islands), sizeof(*out), out, capacity, count);
}

int s2amd_world_body_summary(s2amdSolver* s, s2amdBodySummary* out)
{
	const int rc = out ? reportHeadFor(ref(s), 0, "s2amd_world_body_summary") : fail(S2AMD_E_INVALID, "bad argument");
	if (rc == S2AMD_OK)
	{
		*out = s->hBodyReportHead.summary;
	}
	return rc;
}

} // extern "C"
#pragma GCC visibility pop
