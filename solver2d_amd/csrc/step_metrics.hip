// Step metrics of the resident world (include/solver2d_amd.h: s2amd_world_set_metrics, s2amd_world_metrics, s2amd_world_metrics_history):
// how deep the contacts still sit, how fast bodies still approach, the energy, momentum and spin of the bodies and how far the revolute
// joints have pulled apart -- the world as it stands after stage 4 of s2amd_world_step reduced to ONE 128-byte s2amdStepMetrics on the
// device, behind the body report, and kept in a ring in device memory, instead of a download of the whole world every step and the
// arithmetic on the host.  Two launches per step:
//
//   metricsGatherKernel   one launch over the three domains in tiles of 256 slots: blocks [0, contactTiles) the contact slots,
//                         [contactTiles, contactTiles + bodyTiles) the body slots, the rest the joint slots (a section whose flag is off
//                         has no tiles).  A lane computes its slot's terms; counts go through wave sums, the arg-min / arg-max through
//                         compare-and-keep over (value, slot), and every float sum through PSUM's in-tile shape: a 64-lane xor butterfly
//                         with masks 1, 2, 4, 8, 16, 32 -- lane 0 then holds levels 0..5 of the pairwise tree -- and the four wave sums
//                         as (w0 + w1) + (w2 + w3), levels 6 and 7.  A lane outside the array or without a term contributes +0.0f.  Each
//                         tile leaves its counts in a partial record and its float sums in per-sum arrays.
//                         The 152-byte contact records are read by the lanes of touching slots alone, straight from memory: neighbouring
//                         lanes read neighbouring records, so every line a wave fetches is used by it, a tile without a touching slot
//                         fetches 12 bytes per slot, and the tile needs no LDS image (38 KiB for 256 records), which would cap the
//                         blocks per CU for the body gathers behind it.
//   metricsFinishKernel   one workgroup: lanes 0..7 of its first wave add the tiles' float sums left to right from +0.0f (addInOrder,
//                         one sum per lane), all lanes add up the counts and resolve arg-min and arg-max over the tiles, and lane 0
//                         writes the record with eight 16-byte stores into the ring position the host passes.
//
// The order of every float operation is fixed and there is no floating-point atomic: a record is a pure function of the arrays.  The
// kernels are enqueued once per step behind the attempt that stands: a repeated step records once.  A step allocates nothing and waits
// for nothing -- the getters do.
#include "report_common.h"

namespace
{

static_assert(sizeof(s2amdStepMetrics) == 128, "one record: eight 16-byte stores");
static_assert(S2_BLOCK == 256, "PSUM's tile");

#define S2_METRICS_ALL (S2AMD_METRICS_CONTACTS | S2AMD_METRICS_BODIES | S2AMD_METRICS_JOINTS)
#define S2_METRICS_SLOP 0.005f // s2_linearSlop (src/core.h)

// what one contact tile leaves besides its two float sums
struct ContactTilePartial
{
	int32_t contacts, points, penetrating, approaching;
	float minGap;
	int32_t minGapSlot; // -1: no point whose gap is a number
	float maxApproach;
	int32_t maxApproachSlot; // -1: no approaching point
};
static_assert(sizeof(ContactTilePartial) == 32, "two 16-byte stores");

struct JointTilePartial
{
	int32_t revolute, maxGapSlot;
	float maxGap;
	int32_t pad;
};
static_assert(sizeof(JointTilePartial) == 16, "one 16-byte store");

// float sums: the index of a sum's per-tile array
enum
{
	S2_SUM_PENETRATION,
	S2_SUM_NORMAL_IMPULSE,
	S2_SUM_KINETIC,
	S2_SUM_POTENTIAL,
	S2_SUM_MOMENTUM_X,
	S2_SUM_MOMENTUM_Y,
	S2_SUM_SPIN,
	S2_SUM_JOINT_GAP,
	S2_SUM_COUNT
};

struct MetricsLayout
{
	size_t contactPartials, bodyCounts, jointPartials, sums, total;
	int contactTiles, bodyTiles, jointTiles; // of the whole capacities, whatever the flags
	int sumStride;							 // floats between the per-tile arrays of two sums: a multiple of 64, so every array starts on a line
};

MetricsLayout metricsLayout(int nc, int nb, int nj)
{
	MetricsLayout l{};
	size_t at = 0;
	l.contactTiles = (nc + S2_BLOCK - 1) / S2_BLOCK, l.bodyTiles = (nb + S2_BLOCK - 1) / S2_BLOCK, l.jointTiles = (nj + S2_BLOCK - 1) / S2_BLOCK;
	l.contactPartials = reportTake(at, (size_t)l.contactTiles * sizeof(ContactTilePartial));
	l.bodyCounts = reportTake(at, (size_t)l.bodyTiles * sizeof(int32_t));
	l.jointPartials = reportTake(at, (size_t)l.jointTiles * sizeof(JointTilePartial));
	l.sumStride = (std::max(std::max(l.contactTiles, l.bodyTiles), std::max(l.jointTiles, 1)) + 63) & ~63;
	l.sums = reportTake(at, (size_t)S2_SUM_COUNT * l.sumStride * sizeof(float));
	l.total = at;
	return l;
}

// what the kernels are told about the step
struct MetricsStep
{
	int32_t step, flags, solverType;
	float dt, gx, gy;
	int32_t contactTiles, bodyTiles, jointTiles; // of this launch: 0 for a section whose flag is off
};

struct MetricsBuffers
{
	ContactTilePartial* contactPartials;
	int32_t* bodyCounts;
	JointTilePartial* jointPartials;
	float* sums; // sum k's per-tile array starts at sums + k * sumStride
	int32_t sumStride;
};

S2_DEV int waveSum(int v)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		v += __shfl_xor(v, d);
	}
	return v;
}

// PSUM levels 0..5: after mask m every lane holds the sum of its aligned group of 2m lanes, combined as the pairwise tree combines them
// (t[i] + t[i + m] for the group's lower half: the addition commutes, so the upper half holds the same bits)
S2_DEV float waveTreeSum(float v)
{
	for (int m = 1; m < 64; m <<= 1)
	{
		v = v + __shfl_xor(v, m);
	}
	return v;
}

// "smaller value, then lower slot"; slot -1: nothing yet
S2_DEV void keepMin(float& v, int& slot, float otherV, int otherSlot)
{
	if (otherSlot >= 0 && (slot < 0 || otherV < v || (otherV == v && otherSlot < slot)))
	{
		v = otherV, slot = otherSlot;
	}
}

// "larger value, then lower slot"; slot -1: nothing yet
S2_DEV void keepMax(float& v, int& slot, float otherV, int otherSlot)
{
	if (otherSlot >= 0 && (slot < 0 || otherV > v || (otherV == v && otherSlot < slot)))
	{
		v = otherV, slot = otherSlot;
	}
}

S2_DEV void minOverWave(float& v, int& slot)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const float otherV = __shfl_xor(v, d);
		const int otherSlot = __shfl_xor(slot, d);
		keepMin(v, slot, otherV, otherSlot);
	}
}

S2_DEV void maxOverWave(float& v, int& slot)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const float otherV = __shfl_xor(v, d);
		const int otherSlot = __shfl_xor(slot, d);
		keepMax(v, slot, otherV, otherSlot);
	}
}

// the velocity of body `b`'s material point at local anchor `anchor` (relative to the body origin)
S2_DEV float2 pointVelocity(const s2amdBody& b, float2 anchor)
{
	const float ax = anchor.x - b.localCenter[0], ay = anchor.y - b.localCenter[1];
	const float s = b.rot[0], c = b.rot[1];
	const float rx = c * ax - s * ay, ry = s * ax + c * ay;
	const float w = b.angularVelocity;
	return make_float2(b.linearVelocity[0] - w * ry, b.linearVelocity[1] + w * rx);
}

// One contact slot's terms
struct ContactTerms
{
	int points, penetrating, approaching;
	float minGap;
	int minGapSlot;
	float maxApproach;
	int maxApproachSlot;
	float penetration, normalImpulse;
};

S2_DEV ContactTerms contactTerms(const s2amdContact* contacts, const s2amdPairState* pairs, const s2amdBody* bodies, const float2* origins, int nc, int nb, int i)
{
	ContactTerms t;
	t.points = 0, t.penetrating = 0, t.approaching = 0;
	t.minGap = 0.0f, t.minGapSlot = -1, t.maxApproach = 0.0f, t.maxApproachSlot = -1;
	t.penetration = 0.0f, t.normalImpulse = 0.0f;
	if (i >= nc || pairs[i].shapeA < 0)
	{
		return t;
	}
	const s2amdContact& c = contacts[i];
	const int pointCount = c.pointCount, a = c.bodyA, b = c.bodyB;
	if (pointCount <= 0 || a < 0 || a >= nb || b < 0 || b >= nb)
	{
		return t;
	}
	t.points = pointCount < 2 ? 1 : 2;
	const s2amdBody& bodyA = bodies[a];
	const s2amdBody& bodyB = bodies[b];
	const float2 oA = origins[a], oB = origins[b];
	const float2 qA = make_float2(bodyA.rot[0], bodyA.rot[1]), qB = make_float2(bodyB.rot[0], bodyB.rot[1]);
	const float nx = c.normal[0], ny = c.normal[1];
	float pen[2] = {0.0f, 0.0f}, imp[2] = {0.0f, 0.0f};
#pragma unroll
	for (int j = 0; j < 2; ++j)
	{
		if (j < t.points)
		{
			const s2amdManifoldPoint& p = c.points[j];
			const float2 lA = make_float2(p.localAnchorA[0], p.localAnchorA[1]), lB = make_float2(p.localAnchorB[0], p.localAnchorB[1]);
			const float2 pA = transformPoint(oA, qA, lA), pB = transformPoint(oB, qB, lB);
			const float dx = pB.x - pA.x, dy = pB.y - pA.y;
			const float gap = (dx * nx + dy * ny) + p.separation;
			const float2 uA = pointVelocity(bodyA, lA), uB = pointVelocity(bodyB, lB);
			const float ex = uB.x - uA.x, ey = uB.y - uA.y;
			const float vn = ex * nx + ey * ny;
			t.penetrating += gap < -S2_METRICS_SLOP ? 1 : 0;
			t.approaching += vn < 0.0f ? 1 : 0;
			// (a NaN never wins; the lower point keeps a tie inside the slot)
			if (gap == gap && (t.minGapSlot < 0 || gap < t.minGap))
			{
				t.minGap = gap, t.minGapSlot = i;
			}
			if (vn < 0.0f && (t.maxApproachSlot < 0 || -vn > t.maxApproach))
			{
				t.maxApproach = -vn, t.maxApproachSlot = i;
			}
			pen[j] = gap < 0.0f ? -gap : 0.0f;
			imp[j] = p.normalImpulse;
		}
	}
	t.penetration = t.points == 2 ? pen[0] + pen[1] : pen[0];
	t.normalImpulse = t.points == 2 ? imp[0] + imp[1] : imp[0];
	return t;
}

// squared anchor gap of a revolute joint (joint_report.hip: jointCountKernel); a body outside the array stands at the origin, unrotated
S2_DEV float jointGapSquared(const s2amdJoint& j, const s2amdBody* bodies, const float2* origins, int nb)
{
	float2 oA = make_float2(0.0f, 0.0f), qA = make_float2(0.0f, 1.0f), oB = oA, qB = qA;
	if (j.bodyA >= 0 && j.bodyA < nb)
	{
		oA = origins[j.bodyA], qA = make_float2(bodies[j.bodyA].rot[0], bodies[j.bodyA].rot[1]);
	}
	if (j.bodyB >= 0 && j.bodyB < nb)
	{
		oB = origins[j.bodyB], qB = make_float2(bodies[j.bodyB].rot[0], bodies[j.bodyB].rot[1]);
	}
	const float2 pa = transformPoint(oA, qA, make_float2(j.localOriginAnchorA[0], j.localOriginAnchorA[1]));
	const float2 pb = transformPoint(oB, qB, make_float2(j.localOriginAnchorB[0], j.localOriginAnchorB[1]));
	const float dx = pb.x - pa.x, dy = pb.y - pa.y;
	return dx * dx + dy * dy;
}

// PSUM levels 6 and 7 over the wave sums lane 0 of every wave left in `waveSums[k][wave]`
S2_DEV float tileSum(const float (*waveSums)[S2_BLOCK / 64], int k)
{
	return (waveSums[k][0] + waveSums[k][1]) + (waveSums[k][2] + waveSums[k][3]);
}

__global__ __launch_bounds__(S2_BLOCK) void metricsGatherKernel(const s2amdContact* contacts, const s2amdPairState* pairs, int nc, const s2amdBody* bodies,
																const float2* origins, int nb, const s2amdJoint* joints, int nj, MetricsStep step, MetricsBuffers out)
{
	__shared__ float waveSums[5][S2_BLOCK / 64];
	__shared__ int waveCounts[4][S2_BLOCK / 64];
	__shared__ float waveBest[2][S2_BLOCK / 64];
	__shared__ int waveBestSlot[2][S2_BLOCK / 64];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	int tile = (int)blockIdx.x;
	if (tile < step.contactTiles)
	{
		const int i = tile * S2_BLOCK + (int)threadIdx.x;
		ContactTerms t = contactTerms(contacts, pairs, bodies, origins, nc, nb, i);
		const int nContacts = waveSum(t.points > 0 ? 1 : 0), nPoints = waveSum(t.points);
		const int nPenetrating = waveSum(t.penetrating), nApproaching = waveSum(t.approaching);
		minOverWave(t.minGap, t.minGapSlot);
		maxOverWave(t.maxApproach, t.maxApproachSlot);
		const float penetration = waveTreeSum(t.penetration), normalImpulse = waveTreeSum(t.normalImpulse);
		if (lane == 0)
		{
			waveCounts[0][wave] = nContacts, waveCounts[1][wave] = nPoints, waveCounts[2][wave] = nPenetrating, waveCounts[3][wave] = nApproaching;
			waveBest[0][wave] = t.minGap, waveBestSlot[0][wave] = t.minGapSlot;
			waveBest[1][wave] = t.maxApproach, waveBestSlot[1][wave] = t.maxApproachSlot;
			waveSums[0][wave] = penetration, waveSums[1][wave] = normalImpulse;
		}
		__syncthreads();
		if (threadIdx.x == 0)
		{
			ContactTilePartial p;
			p.contacts = waveCounts[0][0] + waveCounts[0][1] + waveCounts[0][2] + waveCounts[0][3];
			p.points = waveCounts[1][0] + waveCounts[1][1] + waveCounts[1][2] + waveCounts[1][3];
			p.penetrating = waveCounts[2][0] + waveCounts[2][1] + waveCounts[2][2] + waveCounts[2][3];
			p.approaching = waveCounts[3][0] + waveCounts[3][1] + waveCounts[3][2] + waveCounts[3][3];
			p.minGap = 0.0f, p.minGapSlot = -1, p.maxApproach = 0.0f, p.maxApproachSlot = -1;
			for (int w = 0; w < S2_BLOCK / 64; ++w)
			{
				keepMin(p.minGap, p.minGapSlot, waveBest[0][w], waveBestSlot[0][w]);
				keepMax(p.maxApproach, p.maxApproachSlot, waveBest[1][w], waveBestSlot[1][w]);
			}
			uint4* dst = (uint4*)(out.contactPartials + tile);
			dst[0] = make_uint4((uint32_t)p.contacts, (uint32_t)p.points, (uint32_t)p.penetrating, (uint32_t)p.approaching);
			dst[1] = make_uint4(__float_as_uint(p.minGap), (uint32_t)p.minGapSlot, __float_as_uint(p.maxApproach), (uint32_t)p.maxApproachSlot);
			out.sums[S2_SUM_PENETRATION * out.sumStride + tile] = tileSum(waveSums, 0);
			out.sums[S2_SUM_NORMAL_IMPULSE * out.sumStride + tile] = tileSum(waveSums, 1);
		}
		return;
	}
	tile -= step.contactTiles;
	if (tile < step.bodyTiles)
	{
		const int i = tile * S2_BLOCK + (int)threadIdx.x;
		bool counted = false;
		float kinetic = 0.0f, potential = 0.0f, px = 0.0f, py = 0.0f, spin = 0.0f;
		if (i < nb)
		{
			const s2amdBody& b = bodies[i];
			counted = b.type != S2AMD_BODY_FREE && b.type != S2AMD_BODY_STATIC;
			if (counted)
			{
				const float vx = b.linearVelocity[0], vy = b.linearVelocity[1], w = b.angularVelocity;
				kinetic = ((0.5f * b.mass) * (vx * vx + vy * vy)) + ((0.5f * b.I) * (w * w));
				potential = -((b.mass * b.gravityScale) * (step.gx * b.position[0] + step.gy * b.position[1]));
				px = b.mass * vx, py = b.mass * vy;
				spin = b.I * w;
			}
		}
		const int nCounted = waveSum(counted ? 1 : 0);
		kinetic = waveTreeSum(kinetic), potential = waveTreeSum(potential), px = waveTreeSum(px), py = waveTreeSum(py), spin = waveTreeSum(spin);
		if (lane == 0)
		{
			waveCounts[0][wave] = nCounted;
			waveSums[0][wave] = kinetic, waveSums[1][wave] = potential, waveSums[2][wave] = px, waveSums[3][wave] = py, waveSums[4][wave] = spin;
		}
		__syncthreads();
		if (threadIdx.x == 0)
		{
			out.bodyCounts[tile] = waveCounts[0][0] + waveCounts[0][1] + waveCounts[0][2] + waveCounts[0][3];
		}
		if (threadIdx.x < 5)
		{
			// (S2_SUM_KINETIC .. S2_SUM_SPIN in the order of waveSums' rows)
			out.sums[(S2_SUM_KINETIC + (int)threadIdx.x) * out.sumStride + tile] = tileSum(waveSums, (int)threadIdx.x);
		}
		return;
	}
	tile -= step.bodyTiles;
	{
		const int i = tile * S2_BLOCK + (int)threadIdx.x;
		bool revolute = false;
		float term = 0.0f, g = -1.0f;
		int gSlot = -1;
		if (i < nj)
		{
			const s2amdJoint& j = joints[i];
			revolute = j.type == S2AMD_JOINT_REVOLUTE;
			if (revolute)
			{
				term = jointGapSquared(j, bodies, origins, nb);
				if (term >= 0.0f) // (a NaN never wins)
				{
					g = term, gSlot = i;
				}
			}
		}
		const int nRevolute = waveSum(revolute ? 1 : 0);
		maxOverWave(g, gSlot);
		term = waveTreeSum(term);
		if (lane == 0)
		{
			waveCounts[0][wave] = nRevolute;
			waveBest[0][wave] = g, waveBestSlot[0][wave] = gSlot;
			waveSums[0][wave] = term;
		}
		__syncthreads();
		if (threadIdx.x == 0)
		{
			float tg = -1.0f;
			int ts = -1;
			for (int w = 0; w < S2_BLOCK / 64; ++w)
			{
				keepMax(tg, ts, waveBest[0][w], waveBestSlot[0][w]);
			}
			const int total = waveCounts[0][0] + waveCounts[0][1] + waveCounts[0][2] + waveCounts[0][3];
			*(uint4*)(out.jointPartials + tile) = make_uint4((uint32_t)total, (uint32_t)ts, __float_as_uint(tg), 0u);
			out.sums[S2_SUM_JOINT_GAP * out.sumStride + tile] = tileSum(waveSums, 0);
		}
	}
}

// One workgroup.  record: the ring position of this step.
__global__ __launch_bounds__(S2_BLOCK) void metricsFinishKernel(MetricsStep step, MetricsBuffers in, uint4* record)
{
	__shared__ float sums[S2_SUM_COUNT];
	__shared__ int waveCounts[6][S2_BLOCK / 64];
	__shared__ float waveBest[3][S2_BLOCK / 64];
	__shared__ int waveBestSlot[3][S2_BLOCK / 64];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	if (threadIdx.x < S2_SUM_COUNT)
	{
		// the tile sums left to right from +0.0f: one sum per lane, each lane its own array (and its own trip count)
		const int k = (int)threadIdx.x;
		const int tiles = k <= S2_SUM_NORMAL_IMPULSE ? step.contactTiles : k <= S2_SUM_SPIN ? step.bodyTiles : step.jointTiles;
		sums[k] = addInOrder(0.0f, in.sums + k * in.sumStride, tiles);
	}
	int contacts = 0, points = 0, penetrating = 0, approaching = 0, energyBodies = 0, revolute = 0;
	float minGap = 0.0f, maxApproach = 0.0f, maxJointGap = -1.0f;
	int minGapSlot = -1, maxApproachSlot = -1, maxJointGapSlot = -1;
	// (ascending tiles per lane and a total order: the result does not depend on who holds which tile)
	for (int b = (int)threadIdx.x; b < step.contactTiles; b += S2_BLOCK)
	{
		const ContactTilePartial p = in.contactPartials[b];
		contacts += p.contacts, points += p.points, penetrating += p.penetrating, approaching += p.approaching;
		keepMin(minGap, minGapSlot, p.minGap, p.minGapSlot);
		keepMax(maxApproach, maxApproachSlot, p.maxApproach, p.maxApproachSlot);
	}
	for (int b = (int)threadIdx.x; b < step.bodyTiles; b += S2_BLOCK)
	{
		energyBodies += in.bodyCounts[b];
	}
	for (int b = (int)threadIdx.x; b < step.jointTiles; b += S2_BLOCK)
	{
		const JointTilePartial p = in.jointPartials[b];
		revolute += p.revolute;
		keepMax(maxJointGap, maxJointGapSlot, p.maxGap, p.maxGapSlot);
	}
	contacts = waveSum(contacts), points = waveSum(points), penetrating = waveSum(penetrating), approaching = waveSum(approaching);
	energyBodies = waveSum(energyBodies), revolute = waveSum(revolute);
	minOverWave(minGap, minGapSlot);
	maxOverWave(maxApproach, maxApproachSlot);
	maxOverWave(maxJointGap, maxJointGapSlot);
	if (lane == 0)
	{
		waveCounts[0][wave] = contacts, waveCounts[1][wave] = points, waveCounts[2][wave] = penetrating, waveCounts[3][wave] = approaching;
		waveCounts[4][wave] = energyBodies, waveCounts[5][wave] = revolute;
		waveBest[0][wave] = minGap, waveBestSlot[0][wave] = minGapSlot;
		waveBest[1][wave] = maxApproach, waveBestSlot[1][wave] = maxApproachSlot;
		waveBest[2][wave] = maxJointGap, waveBestSlot[2][wave] = maxJointGapSlot;
	}
	__syncthreads();
	if (threadIdx.x != 0)
	{
		return;
	}
	int total[6];
	for (int k = 0; k < 6; ++k)
	{
		total[k] = waveCounts[k][0] + waveCounts[k][1] + waveCounts[k][2] + waveCounts[k][3];
	}
	minGap = 0.0f, minGapSlot = -1, maxApproach = 0.0f, maxApproachSlot = -1, maxJointGap = -1.0f, maxJointGapSlot = -1;
	for (int w = 0; w < S2_BLOCK / 64; ++w)
	{
		keepMin(minGap, minGapSlot, waveBest[0][w], waveBestSlot[0][w]);
		keepMax(maxApproach, maxApproachSlot, waveBest[1][w], waveBestSlot[1][w]);
		keepMax(maxJointGap, maxJointGapSlot, waveBest[2][w], waveBestSlot[2][w]);
	}
	const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
	uint4 chunk[8];
	chunk[0] = make_uint4((uint32_t)step.step, (uint32_t)step.flags, (uint32_t)step.solverType, __float_as_uint(step.dt));
	chunk[1] = zero, chunk[2] = zero, chunk[3] = zero, chunk[4] = zero, chunk[5] = zero, chunk[6] = zero, chunk[7] = zero;
	if ((step.flags & S2AMD_METRICS_CONTACTS) != 0)
	{
		chunk[1] = make_uint4((uint32_t)total[0], (uint32_t)total[1], (uint32_t)total[2], (uint32_t)total[3]);
		chunk[2] = make_uint4(__float_as_uint(minGap), (uint32_t)minGapSlot, __float_as_uint(maxApproach), (uint32_t)maxApproachSlot);
		chunk[3].x = __float_as_uint(sums[S2_SUM_PENETRATION]), chunk[3].y = __float_as_uint(sums[S2_SUM_NORMAL_IMPULSE]);
	}
	if ((step.flags & S2AMD_METRICS_BODIES) != 0)
	{
		chunk[3].z = (uint32_t)total[4], chunk[3].w = __float_as_uint(sums[S2_SUM_KINETIC]);
		chunk[4] = make_uint4(__float_as_uint(sums[S2_SUM_POTENTIAL]), __float_as_uint(sums[S2_SUM_MOMENTUM_X]), __float_as_uint(sums[S2_SUM_MOMENTUM_Y]),
							  __float_as_uint(sums[S2_SUM_SPIN]));
	}
	if ((step.flags & S2AMD_METRICS_JOINTS) != 0)
	{
		chunk[5] = make_uint4((uint32_t)total[5], (uint32_t)maxJointGapSlot, __float_as_uint(maxJointGap), __float_as_uint(sums[S2_SUM_JOINT_GAP]));
	}
#pragma unroll
	for (int k = 0; k < 8; ++k)
	{
		record[k] = chunk[k];
	}
}

// the record's chunks above are the struct's fields in order
static_assert(offsetof(s2amdStepMetrics, touchingContacts) == 16 && offsetof(s2amdStepMetrics, minGap) == 32 && offsetof(s2amdStepMetrics, sumPenetration) == 48 &&
				  offsetof(s2amdStepMetrics, energyBodies) == 56 && offsetof(s2amdStepMetrics, potentialEnergy) == 64 && offsetof(s2amdStepMetrics, revoluteJoints) == 80 &&
				  offsetof(s2amdStepMetrics, sumJointGapSquared) == 92 && offsetof(s2amdStepMetrics, pad) == 96,
			  "the record as metricsFinishKernel stores it");

int metricsGetterState(const s2amdSolver* s)
{
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	return S2AMD_OK;
}

// records [first, first + count) of the ring, in order
int metricsFetch(s2amdSolver* s, s2amdStepMetrics* out, int first, int count)
{
	if (count > 0)
	{
		HIP_TRY(hipSetDevice(s->device));
		HIP_TRY(hipMemcpyAsync(out, (const s2amdStepMetrics*)s->dMetricsRing.p + first, (size_t)count * sizeof(s2amdStepMetrics), hipMemcpyDeviceToHost, s->stream));
	}
	return S2AMD_OK;
}

} // namespace

int metricsPrepare(s2amdSolver* s)
{
	s->metricsWritten = 0;
	if (!reportPrepareBegin(s, s->metrics))
	{
		return S2AMD_OK;
	}
	return reportPrepareBlock(s->metrics, metricsLayout(s->contactCapacity, s->bodyCapacity, s->jointCapacity).total, 0);
}

int metricsEnqueue(s2amdSolver* s, const s2amdStepParams* params)
{
	const int flags = s->metrics.flags;
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	const int nc = s->contactCapacity, nb = s->bodyCapacity, nj = s->jointCapacity;
	const MetricsLayout l = metricsLayout(nc, nb, nj);
	if (s->metricsLength < 1 || s->dMetricsRing.p == nullptr || s->dMetricsRing.bytes < (size_t)s->metricsLength * sizeof(s2amdStepMetrics) ||
		s->metrics.block.p == nullptr || s->metrics.block.bytes < l.total)
	{
		return fail(S2AMD_E_STATE, "internal: the step metrics' device blocks were not prepared");
	}
	char* base = (char*)s->metrics.block.p;
	MetricsBuffers buffers;
	buffers.contactPartials = (ContactTilePartial*)(base + l.contactPartials);
	buffers.bodyCounts = (int32_t*)(base + l.bodyCounts);
	buffers.jointPartials = (JointTilePartial*)(base + l.jointPartials);
	buffers.sums = (float*)(base + l.sums), buffers.sumStride = l.sumStride;
	MetricsStep step;
	step.step = (int32_t)s->metricsWritten, step.flags = flags, step.solverType = params->solverType;
	step.dt = params->dt, step.gx = params->gravity[0], step.gy = params->gravity[1];
	step.contactTiles = (flags & S2AMD_METRICS_CONTACTS) != 0 ? l.contactTiles : 0;
	step.bodyTiles = (flags & S2AMD_METRICS_BODIES) != 0 ? l.bodyTiles : 0;
	step.jointTiles = (flags & S2AMD_METRICS_JOINTS) != 0 ? l.jointTiles : 0;
	const int tiles = step.contactTiles + step.bodyTiles + step.jointTiles;
	hipStream_t st = s->stream;
	if (tiles > 0)
	{
		metricsGatherKernel<<<dim3((unsigned)tiles), dim3(S2_BLOCK), 0, st>>>((const s2amdContact*)s->dContacts.p, (const s2amdPairState*)s->dPairs.p, nc,
																			  (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, nb, (const s2amdJoint*)s->dJoints.p, nj,
																			  step, buffers);
	}
	const size_t position = (size_t)(s->metricsWritten % (long long)s->metricsLength);
	metricsFinishKernel<<<dim3(1), dim3(S2_BLOCK), 0, st>>>(step, buffers, (uint4*)((s2amdStepMetrics*)s->dMetricsRing.p + position));
	HIP_TRY(hipGetLastError());
	s->metricsWritten += 1;
	s->metrics.stepFlags = flags;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_metrics(s2amdSolver* s, int32_t flags, int32_t historyLength)
{
	if (!s)
	{
		return fail(S2AMD_E_INVALID, "null solver");
	}
	if ((flags & ~S2_METRICS_ALL) != 0)
	{
		return fail(S2AMD_E_INVALID, "unknown step-metrics flag bits");
	}
	if (flags != 0 && (historyLength < 1 || historyLength > S2AMD_METRICS_MAX_HISTORY))
	{
		return fail(S2AMD_E_INVALID, "step metrics: the history length must be 1.." + std::to_string(S2AMD_METRICS_MAX_HISTORY));
	}
	if (flags != 0)
	{
		const size_t need = (size_t)historyLength * sizeof(s2amdStepMetrics);
		if (need > s->dMetricsRing.bytes && s->dMetricsRing.p != nullptr)
		{
			// (a step enqueued earlier may still be writing into the ring that is about to be given back)
			HIP_TRY(hipSetDevice(s->device));
			HIP_TRY(hipStreamSynchronize(s->stream));
		}
		const int rc = s->dMetricsRing.ensure(need);
		if (rc)
		{
			return rc;
		}
		s->metricsLength = historyLength;
	}
	s->metrics.flags = flags;
	return metricsPrepare(s);
}

int s2amd_world_metrics(s2amdSolver* s, s2amdStepMetrics* out)
{
	if (!s || !out)
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	int rc = metricsGetterState(s);
	if (rc)
	{
		return rc;
	}
	if (s->metrics.stepFlags == 0 || s->metricsWritten < 1)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_metrics: the last s2amd_world_step recorded nothing (s2amd_world_set_metrics, then a step)");
	}
	if ((rc = metricsFetch(s, out, (int)((s->metricsWritten - 1) % (long long)s->metricsLength), 1)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

int s2amd_world_metrics_history(s2amdSolver* s, s2amdStepMetrics* out, int32_t capacity, int32_t* count)
{
	if (!s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	int rc = metricsGetterState(s);
	if (rc)
	{
		return rc;
	}
	if (s->metrics.flags == 0)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_metrics_history: the recorder is off (s2amd_world_set_metrics)");
	}
	const long long length = (long long)s->metricsLength;
	const int n = (int)std::min(s->metricsWritten, length);
	*count = n;
	if (n > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "step-metrics history buffer too small");
	}
	if (n == 0)
	{
		return S2AMD_OK;
	}
	// the oldest record's position, and the two runs of the ring behind it: [start, length) and, wrapped, [0, ...)
	const int start = (int)((s->metricsWritten - n) % length);
	const int head = std::min(n, (int)length - start);
	if ((rc = metricsFetch(s, out, start, head)) != 0 || (rc = metricsFetch(s, out + head, 0, n - head)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop
