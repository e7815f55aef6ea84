// Resets on the resident world (include/solver2d_amd.h: s2amd_world_set_resets, s2amd_world_set_reset_report, s2amd_world_reset_agents,
// s2amd_world_reset_states, s2amd_world_reset_counts): a persistent list of body records and joint records over agents; the bodies and
// joints of a triggered agent go back to the start state of their records, and the boxes, contacts and pair states that the teleport
// invalidates are put right -- stage 4's box arithmetic (refit_ops.h), s2BroadPhase_MoveProxy's unconditional fat box with the shape in
// the move buffer, s2CreateContact's empty manifold.  The eleventh entry of report_host.cpp's table, behind the episodes whose flags word
// is the trigger of a step, and the first that writes the world; s2amd_world_reset_agents is the same pass between steps.
//
// A pass is two launches:
//   resetRecordsKernel  one lane per body record, per joint record and per agent, each range in workgroups of its own.  A record lane
//                       reads its agent's trigger and the agent's `resets` counter of the set this pass reads, writes its target, the
//                       body's origin and mark[body] = 1 or 0 -- every pass, each record owns its byte (the host has refused a slot
//                       named twice), so nothing clears the marks.  An agent lane writes its record of the OTHER set: the record lanes
//                       of this launch read counters that nobody writes.  countsNow[1], the bodies applied, is the marked-body word.
//   resetWorldKernel    one lane per shape slot and per contact slot.  Every wave first reads the marked-body word at a uniform address
//                       and leaves if it is 0: a step in which nobody finished pays two near-empty launches.  A shape lane reads
//                       mark[shape.body], a contact lane mark[bodyA] | mark[bodyB]; the contact record is emptied with 16-byte stores.
// The counts are the episodes' (two sets, ping-pong; one ballot and one integer atomic per wave and code).  No float atomics, no sort,
// no scratch, no LDS, no memset and no host wait in a pass.  The arithmetic is fp32 one operation at a time; this file is compiled
// without contraction in both libraries (Makefile), because the result is stated bit for bit.
#include "solver_internal.h"

#include "refit_ops.h"
#include "report_common.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdResetBody) == 64 && sizeof(s2amdResetJoint) == 32 && sizeof(s2amdResetState) == 16, "the resets' records");
static_assert(sizeof(s2amdBody) == 88 && sizeof(s2amdJoint) == 92 && sizeof(s2amdContact) == 152 && sizeof(s2amdPairState) == 28 && sizeof(s2amdShape) == 196,
			  "the wire records the pass stores into by word");

#define S2_RESET_KNOWN (S2AMD_RESET_ON_EPISODE_END | S2AMD_RESET_REPORT_STATES)

// the device block of a list
struct ResetLayout
{
	size_t counts, bodies, joints, states, trigger, total;
};

ResetLayout resetLayout(int bodies, int joints, int agents)
{
	ResetLayout l{};
	size_t at = 0;
	l.counts = reportTake(at, 16 * sizeof(int));
	l.bodies = reportTake(at, (size_t)bodies * sizeof(s2amdResetBody));
	l.joints = reportTake(at, (size_t)joints * sizeof(s2amdResetJoint));
	l.states = reportTake(at, 2 * (size_t)agents * sizeof(s2amdResetState));
	l.trigger = reportTake(at, (size_t)agents * sizeof(int));
	l.total = at;
	return l;
}

ResetLayout layoutOf(const s2amdSolver* s)
{
	return resetLayout((int)s->hResetBodies.size(), (int)s->hResetJoints.size(), s->resetAgents);
}

// MurmurHash3's finaliser (graph_coloring.cpp, structure.hip)
S2_DEV unsigned int fmix32(unsigned int k)
{
	k ^= k >> 16;
	k *= 0x85ebca6bu;
	k ^= k >> 13;
	k *= 0xc2b2ae35u;
	k ^= k >> 16;
	return k;
}

// component c of record k at the agent's n-th reset: base + t * jitter with t in [-1, 1), or base's bits with no jitter
S2_DEV float jittered(float base, float jitter, unsigned int seed, unsigned int k, unsigned int c, unsigned int n)
{
	if (jitter == 0.0f)
	{
		return base;
	}
	unsigned int h = fmix32(seed + 0x9e3779b9u * (8u * k + c));
	h = fmix32(h ^ n);
	const float u = (float)(h >> 8) * 0x1p-24f;
	const float t = 2.0f * u - 1.0f;
	const float d = t * jitter;
	return base + d;
}

// trigger: one word per agent below triggerAgents (nullptr: nobody), tested against mask; all: everybody
S2_DEV bool triggered(int agent, const int* trigger, int triggerAgents, int mask, int all)
{
	if (all != 0)
	{
		return true;
	}
	return trigger != nullptr && agent >= 0 && agent < triggerAgents && (trigger[agent] & mask) != 0;
}

// Workgroups [0, bodyBlocks): body records; [bodyBlocks, bodyBlocks + jointBlocks): joint records; behind them: agents.  The host has
// checked every record; the comparisons against the capacities keep a lane inside the arrays whatever a record names.
__global__ __launch_bounds__(S2_BLOCK) void resetRecordsKernel(const s2amdResetBody* bodyRecords, int bodyCount, int bodyBlocks, const s2amdResetJoint* jointRecords, int jointCount,
																   int jointBlocks, int agents, const int* trigger, int triggerAgents, int mask, int all, unsigned int seed,
																   const s2amdResetState* statesNow, s2amdResetState* statesNext, s2amdBody* bodies, int nb, float2* origins,
																   unsigned char* mark, s2amdJoint* joints, int nj, int* countsNow, int* countsNext)
{
	const int block = (int)blockIdx.x;
	if (block == 0 && threadIdx.x == 0)
	{
		// (the set the pass behind this one counts into)
		((int4*)countsNext)[0] = make_int4(0, 0, 0, 0);
		((int4*)countsNext)[1] = make_int4(0, 0, 0, 0);
	}
	// 0: nothing to count; else the index of the count + 1
	int code = 0;
	if (block < bodyBlocks)
	{
		const int k = block * S2_BLOCK + (int)threadIdx.x;
		if (k < bodyCount)
		{
			const int4 head = ((const int4*)bodyRecords)[4 * (size_t)k];		// agent, body, flags, position.x
			const float4 pose = ((const float4*)bodyRecords)[4 * (size_t)k + 1]; // position.y, rot.s, rot.c, linearVelocity.x
			const float4 rest = ((const float4*)bodyRecords)[4 * (size_t)k + 2]; // linearVelocity.y, angularVelocity, positionJitter
			const float4 tail = ((const float4*)bodyRecords)[4 * (size_t)k + 3]; // velocityJitter, angularJitter, reserved
			const int agent = head.x, body = head.y, flags = head.z;
			const bool on = (flags & S2AMD_RESET_DISABLED) == 0 && agent >= 0 && agent < agents && triggered(agent, trigger, triggerAgents, mask, all);
			const bool inside = body >= 0 && body < nb;
			bool apply = false;
			if (on)
			{
				const int type = inside ? bodies[body].type : S2AMD_BODY_FREE;
				apply = type != S2AMD_BODY_FREE && type != S2AMD_BODY_STATIC;
				code = apply ? 2 : 3;
			}
			if (apply)
			{
				const unsigned int n = (unsigned int)statesNow[agent].resets;
				const float px = jittered(__int_as_float(head.w), rest.z, seed, (unsigned int)k, 0u, n);
				const float py = jittered(pose.x, rest.w, seed, (unsigned int)k, 1u, n);
				const float vx = jittered(pose.w, tail.x, seed, (unsigned int)k, 2u, n);
				const float vy = jittered(rest.x, tail.y, seed, (unsigned int)k, 3u, n);
				const float w = jittered(rest.y, tail.z, seed, (unsigned int)k, 4u, n);
				float* b = (float*)(bodies + body); // 22 words, 8-byte aligned
				const float2 lc = make_float2(b[9], b[10]); // (localCenter lies at an odd word)
				*(float2*)(b + 0) = make_float2(px, py);
				*(float2*)(b + 2) = make_float2(pose.y, pose.z);
				*(float2*)(b + 4) = make_float2(vx, vy);
				*(float2*)(b + 6) = make_float2(w, 0.0f); // angularVelocity, deltaPosition.x
				b[8] = 0.0f;							  // deltaPosition.y
				b[11] = 0.0f;							  // force.x
				*(float2*)(b + 12) = make_float2(0.0f, 0.0f); // force.y, torque
				// (stage4BodyOne's operation order)
				Rot q;
				q.s = pose.y, q.c = pose.z;
				const V2 o = sub(v2(px, py), rotate(q, v2(lc.x, lc.y)));
				origins[body] = make_float2(o.x, o.y);
			}
			if (inside)
			{
				mark[body] = apply ? 1 : 0;
			}
		}
	}
	else if (block < bodyBlocks + jointBlocks)
	{
		const int k = (block - bodyBlocks) * S2_BLOCK + (int)threadIdx.x;
		if (k < jointCount)
		{
			const int4 head = ((const int4*)jointRecords)[2 * (size_t)k];	  // agent, joint, flags, enableMotor
			const int4 tail = ((const int4*)jointRecords)[2 * (size_t)k + 1]; // enableLimit, motorSpeed, targetA
			const int agent = head.x, joint = head.y, flags = head.z;
			const bool on = (flags & S2AMD_RESET_DISABLED) == 0 && agent >= 0 && agent < agents && triggered(agent, trigger, triggerAgents, mask, all);
			if (on)
			{
				const int type = joint >= 0 && joint < nj ? joints[joint].type : S2AMD_JOINT_FREE;
				const bool apply = type != S2AMD_JOINT_FREE;
				code = apply ? 4 : 5;
				if (apply)
				{
					int* j = (int*)(joints + joint); // 23 words, 4-byte aligned
					j[9] = 0, j[10] = 0, j[11] = 0, j[12] = 0, j[13] = 0; // impulse, motorImpulse, lowerImpulse, upperImpulse: +0
					if ((flags & S2AMD_RESET_JOINT_SETTINGS) != 0)
					{
						if (type == S2AMD_JOINT_REVOLUTE)
						{
							j[3] = head.w, j[4] = tail.x, j[15] = tail.y;
						}
						else if (type == S2AMD_JOINT_MOUSE)
						{
							j[21] = tail.z, j[22] = tail.w;
						}
					}
				}
			}
		}
	}
	else
	{
		const int a = (block - bodyBlocks - jointBlocks) * S2_BLOCK + (int)threadIdx.x;
		if (a < agents)
		{
			const bool on = triggered(a, trigger, triggerAgents, mask, all);
			const int resets = statesNow[a].resets + (on ? 1 : 0);
			*(int4*)(statesNext + a) = make_int4(resets, on ? 1 : 0, 0, 0);
			code = on ? 1 : 0;
		}
	}
	// agents reset, bodies applied, bodies skipped, joints applied, joints skipped
	for (int c = 1; c <= 5; ++c)
	{
		const unsigned long long m = __ballot(code == c);
		if (m != 0ull && (threadIdx.x & 63) == 0)
		{
			atomicAdd(countsNow + (c - 1), __popcll(m));
		}
	}
}

// the contact record of slot i as s2CreateContact leaves it: bodyA, bodyB, friction and constraintIndex kept, everything else zero.
// 38 words at an 8-byte aligned address that is 16-byte aligned for an even slot: 16-byte stores with one 8-byte store at the odd end.
S2_DEV void emptyContact(s2amdContact* contacts, int i)
{
	int* c = (int*)(contacts + i);
	const int2 ab = *(const int2*)(c + 0);
	const int2 fi = *(const int2*)(c + 6);
	const int4 zero = make_int4(0, 0, 0, 0);
	if ((i & 1) == 0)
	{
		*(int4*)(c + 0) = make_int4(ab.x, ab.y, 0, 0);
		*(int4*)(c + 4) = make_int4(0, 0, fi.x, fi.y);
		for (int w = 8; w < 36; w += 4)
		{
			*(int4*)(c + w) = zero;
		}
		*(int2*)(c + 36) = make_int2(0, 0);
	}
	else
	{
		*(int2*)(c + 0) = ab;
		*(int4*)(c + 2) = zero;
		*(int4*)(c + 6) = make_int4(fi.x, fi.y, 0, 0);
		for (int w = 10; w < 38; w += 4)
		{
			*(int4*)(c + w) = zero;
		}
	}
}

// Workgroups [0, shapeBlocks): shape slots; behind them: contact slots.
__global__ __launch_bounds__(S2_BLOCK) void resetWorldKernel(const int* markedBodies, const unsigned char* mark, const s2amdBody* bodies, int nb, const float2* origins,
																 s2amdShape* shapes, int ns, int shapeBlocks, s2amdContact* contacts, s2amdPairState* pairs, int nc, int* countsNow)
{
	if (*markedBodies == 0)
	{
		return; // (uniform: the whole grid leaves)
	}
	const int block = (int)blockIdx.x;
	bool moved = false, emptied = false;
	if (block < shapeBlocks)
	{
		const int i = block * S2_BLOCK + (int)threadIdx.x;
		if (i < ns)
		{
			s2amdShape* sh = shapes + i;
			const int body = sh->body, type = sh->type; // (196-byte records: 4-byte aligned, word loads)
			if (type != S2AMD_SHAPE_FREE && body >= 0 && body < nb && mark[body] != 0)
			{
				const float2 o = origins[body];
				Rot q;
				q.s = bodies[body].rot[0], q.c = bodies[body].rot[1];
				(void)refitShapeOne(q, sh, v2(o.x, o.y));
				// s2BroadPhase_MoveProxy: a new fat box whatever the old one held, and into the move buffer
				const float a0 = sh->aabb[0], a1 = sh->aabb[1], a2 = sh->aabb[2], a3 = sh->aabb[3];
				sh->fatAABB[0] = a0 - S2_AABB_MARGIN;
				sh->fatAABB[1] = a1 - S2_AABB_MARGIN;
				sh->fatAABB[2] = a2 + S2_AABB_MARGIN;
				sh->fatAABB[3] = a3 + S2_AABB_MARGIN;
				sh->enlarged = 1;
				moved = true;
			}
		}
	}
	else
	{
		const int i = (block - shapeBlocks) * S2_BLOCK + (int)threadIdx.x;
		if (i < nc)
		{
			int* p = (int*)(pairs + i); // 7 words, 4-byte aligned
			if (p[0] >= 0)
			{
				const int2 ab = *(const int2*)(contacts + i);
				const bool a = ab.x >= 0 && ab.x < nb && mark[ab.x] != 0;
				const bool b = ab.y >= 0 && ab.y < nb && mark[ab.y] != 0;
				if (a || b)
				{
					emptyContact(contacts, i);
					p[2] = 0, p[3] = 0, p[4] = 0, p[5] = 0, p[6] = 0; // the cache, the ids, the persisted flags
					emptied = true;
				}
			}
		}
	}
	const unsigned long long m = __ballot(moved), e = __ballot(emptied);
	if ((threadIdx.x & 63) == 0)
	{
		if (m != 0ull)
		{
			atomicAdd(countsNow + 5, __popcll(m));
		}
		if (e != 0ull)
		{
			atomicAdd(countsNow + 6, __popcll(e));
		}
	}
}

bool finite2(const float v[2])
{
	return std::isfinite(v[0]) && std::isfinite(v[1]);
}

bool validBody(const s2amdResetBody& r, int32_t agents)
{
	if (r.agent < 0 || r.agent >= agents || r.body < 0 || (r.flags & ~S2AMD_RESET_DISABLED) != 0 || r.reserved != 0)
	{
		return false;
	}
	if (!finite2(r.position) || !finite2(r.rot) || !finite2(r.linearVelocity) || !std::isfinite(r.angularVelocity) || !finite2(r.positionJitter) ||
		!finite2(r.velocityJitter) || !std::isfinite(r.angularJitter))
	{
		return false;
	}
	return r.positionJitter[0] >= 0.0f && r.positionJitter[1] >= 0.0f && r.velocityJitter[0] >= 0.0f && r.velocityJitter[1] >= 0.0f && r.angularJitter >= 0.0f;
}

bool validJoint(const s2amdResetJoint& r, int32_t agents)
{
	return r.agent >= 0 && r.agent < agents && r.joint >= 0 && (r.flags & ~(S2AMD_RESET_DISABLED | S2AMD_RESET_JOINT_SETTINGS)) == 0 && std::isfinite(r.motorSpeed) &&
		   finite2(r.targetA);
}

// the index of the first entry whose slot an earlier entry names, -1: none
int firstRepeat(std::vector<std::pair<int32_t, int32_t>>& slotAndIndex)
{
	std::sort(slotAndIndex.begin(), slotAndIndex.end());
	int first = -1;
	for (size_t i = 1; i < slotAndIndex.size(); ++i)
	{
		if (slotAndIndex[i].first == slotAndIndex[i - 1].first && (first < 0 || slotAndIndex[i].second < first))
		{
			first = slotAndIndex[i].second;
		}
	}
	return first;
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->resetReport, nullptr, 0, "reset-report", "s2amd_world_set_reset_report"} : ReportRef{};
}

int flagsTurnedOn(s2amdSolver*)
{
	return S2AMD_OK; // (nothing is re-based by the flags: the counters are the list's and the world's)
}

// the counters, both sets of counts and the marks to zero (enqueued): at an upload and when a list goes in
int zeroCounters(s2amdSolver* s, char* base, const ResetLayout& l, int agents)
{
	HIP_TRY(hipMemsetAsync(base + l.counts, 0, 16 * sizeof(int), s->stream));
	HIP_TRY(hipMemsetAsync(base + l.states, 0, 2 * (size_t)agents * sizeof(s2amdResetState), s->stream));
	if (s->worldResident && s->bodyCapacity > 0)
	{
		if (int rc = s->dResetMark.ensure((size_t)s->bodyCapacity))
		{
			return rc;
		}
		HIP_TRY(hipMemsetAsync(s->dResetMark.p, 0, (size_t)s->bodyCapacity, s->stream));
	}
	return S2AMD_OK;
}

// One pass, enqueued on the solver's stream.  trigger: device words, one per agent below triggerAgents; all: every agent.
int enqueuePass(s2amdSolver* s, const int* trigger, int triggerAgents, int mask, int all)
{
	const int agents = s->resetAgents, nrb = (int)s->hResetBodies.size(), nrj = (int)s->hResetJoints.size();
	const int nb = s->bodyCapacity, nj = s->jointCapacity, ns = s->shapeCapacity, nc = s->contactCapacity;
	const ResetLayout l = layoutOf(s);
	if (s->dResets.p == nullptr || s->dResets.bytes < l.total || (nb > 0 && (s->dResetMark.p == nullptr || s->dResetMark.bytes < (size_t)nb)))
	{
		return fail(S2AMD_E_STATE, "internal: the reset list's device block was not prepared");
	}
	char* base = (char*)s->dResets.p;
	int* counts = (int*)(base + l.counts);
	int* now = counts + 8 * (int)(s->resetPasses & 1);
	int* next = counts + 8 * (int)((s->resetPasses + 1) & 1);
	s2amdResetState* states = (s2amdResetState*)(base + l.states);
	const s2amdResetState* statesNow = states + (size_t)agents * (size_t)(s->resetPasses & 1);
	s2amdResetState* statesNext = states + (size_t)agents * (size_t)((s->resetPasses + 1) & 1);
	const int bodyBlocks = (nrb + S2_BLOCK - 1) / S2_BLOCK, jointBlocks = (nrj + S2_BLOCK - 1) / S2_BLOCK, agentBlocks = (agents + S2_BLOCK - 1) / S2_BLOCK;
	resetRecordsKernel<<<dim3((unsigned)(bodyBlocks + jointBlocks + agentBlocks)), dim3(S2_BLOCK), 0, s->stream>>>(
		(const s2amdResetBody*)(base + l.bodies), nrb, bodyBlocks, (const s2amdResetJoint*)(base + l.joints), nrj, jointBlocks, agents, trigger, triggerAgents, mask, all, s->resetSeed,
		statesNow, statesNext, (s2amdBody*)s->dBodies.p, nb, (float2*)s->dOrigins.p, (unsigned char*)s->dResetMark.p, (s2amdJoint*)s->dJoints.p, nj, now, next);
	HIP_TRY(hipGetLastError());
	const int shapeBlocks = (ns + S2_BLOCK - 1) / S2_BLOCK, contactBlocks = (nc + S2_BLOCK - 1) / S2_BLOCK;
	if (nrb > 0 && shapeBlocks + contactBlocks > 0)
	{
		resetWorldKernel<<<dim3((unsigned)(shapeBlocks + contactBlocks)), dim3(S2_BLOCK), 0, s->stream>>>(now + 1, (const unsigned char*)s->dResetMark.p, (const s2amdBody*)s->dBodies.p, nb,
																										  (const float2*)s->dOrigins.p, (s2amdShape*)s->dShapes.p, ns, shapeBlocks,
																										  (s2amdContact*)s->dContacts.p, (s2amdPairState*)s->dPairs.p, nc, now);
		HIP_TRY(hipGetLastError());
	}
	s->resetPasses += 1;
	s->resetCountsKnown = true;
	s->resetSourceOff = false;
	// What the host believed of the world the pass writes: the pair query that rode behind stage 4 ran before it (s2amd_world_find_pairs
	// now runs on the flags as they stand, the resets' included), the per-slot bytes and the step's read-back are of the state before.
	s->pairCacheValid = false;
	s->slotBytesFresh = false;
	s->stepBackValid = false;
	return S2AMD_OK;
}

} // namespace

// (at s2amd_world_upload: the marks are the new world's, the counters go to zero; the list and its block are the setter's and stay)
int resetPrepare(s2amdSolver* s)
{
	(void)reportPrepareBegin(s, s->resetReport);
	s->resetCountsKnown = false;
	s->resetSourceOff = false;
	s->resetPasses = 0;
	if (s->resetAgents <= 0 || !s->worldResident || s->dResets.p == nullptr)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	return zeroCounters(s, (char*)s->dResets.p, layoutOf(s), s->resetAgents);
}

int resetEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->resetReport;
	if (r.flags == 0)
	{
		return S2AMD_OK;
	}
	if (s->resetAgents > 0 && (r.flags & S2AMD_RESET_ON_EPISODE_END) != 0)
	{
		int episodeAgents = 0;
		const int* flags = episodeStepFlags(s, &episodeAgents);
		if (flags == nullptr)
		{
			// (the episode pass did not run this step: nobody is triggered, nothing is enqueued, and the counts say so)
			s->resetCountsKnown = true;
			s->resetSourceOff = true;
		}
		else if (int rc = enqueuePass(s, flags, episodeAgents, 3, 0))
		{
			return rc;
		}
	}
	r.stepFlags = r.flags;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_resets(s2amdSolver* s, const s2amdResetBody* bodies, int32_t bodyCount, const s2amdResetJoint* joints, int32_t jointCount, int32_t agents, uint32_t seed)
{
	if (int rc = listArgs(s, bodies, bodyCount, S2AMD_MAX_RESET_BODIES))
	{
		return rc;
	}
	if (int rc = listArgs(s, joints, jointCount, S2AMD_MAX_RESET_JOINTS))
	{
		return rc;
	}
	if (agents < 0 || agents > S2AMD_MAX_RESET_AGENTS || ((bodyCount > 0 || jointCount > 0) && agents == 0))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	for (int32_t i = 0; i < bodyCount; ++i)
	{
		if (!validBody(bodies[i], agents))
		{
			return fail(S2AMD_E_INVALID, "reset body record " + std::to_string(i) +
											 " is invalid (an agent outside the agents, a negative body, unknown flag bits, reserved != 0, a NaN or infinite value, a "
											 "negative jitter): nothing was replaced");
		}
	}
	for (int32_t i = 0; i < jointCount; ++i)
	{
		if (!validJoint(joints[i], agents))
		{
			return fail(S2AMD_E_INVALID, "reset joint record " + std::to_string(i) +
											 " is invalid (an agent outside the agents, a negative joint, unknown flag bits, a NaN or infinite value): nothing was replaced");
		}
	}
	{
		std::vector<std::pair<int32_t, int32_t>> named((size_t)bodyCount);
		for (int32_t i = 0; i < bodyCount; ++i)
		{
			named[(size_t)i] = {bodies[i].body, i};
		}
		int twice = firstRepeat(named);
		if (twice >= 0)
		{
			return fail(S2AMD_E_INVALID, "reset body record " + std::to_string(twice) + " names a body slot an earlier record names: nothing was replaced");
		}
		named.resize((size_t)jointCount);
		for (int32_t i = 0; i < jointCount; ++i)
		{
			named[(size_t)i] = {joints[i].joint, i};
		}
		twice = firstRepeat(named);
		if (twice >= 0)
		{
			return fail(S2AMD_E_INVALID, "reset joint record " + std::to_string(twice) + " names a joint slot an earlier record names: nothing was replaced");
		}
	}
	if (agents == 0)
	{
		// (the block stays for the next list; a pass in flight still reads it)
		s->hResetBodies.clear();
		s->hResetJoints.clear();
		s->resetAgents = 0;
		s->resetReport.stepFlags = 0;
		s->resetCountsKnown = false, s->resetSourceOff = false;
		s->resetPasses = 0;
		return S2AMD_OK;
	}
	if (treesAnySet(s) || s->refitOrderCount > 0)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_set_resets: a reset list is not offered together with device trees (s2amd_world_set_tree) or a refit order "
								   "(s2amd_world_set_refit_order): nothing was replaced");
	}
	// The lists go to their device block now, so that a pass only launches: waited for, because the block of the list before may still be
	// read by a pass in flight and the copies read this call's memory.
	const ResetLayout l = resetLayout(bodyCount, jointCount, agents);
	const int rc = listUpload(s, s->dResets, l.total, [&](char* base) {
		if (bodyCount > 0)
		{
			HIP_TRY(hipMemcpyAsync(base + l.bodies, bodies, (size_t)bodyCount * sizeof(s2amdResetBody), hipMemcpyHostToDevice, s->stream));
		}
		if (jointCount > 0)
		{
			HIP_TRY(hipMemcpyAsync(base + l.joints, joints, (size_t)jointCount * sizeof(s2amdResetJoint), hipMemcpyHostToDevice, s->stream));
		}
		// (the marks of the list that left go with it: this is the one place that clears them)
		return zeroCounters(s, base, l, agents);
	});
	if (rc)
	{
		return rc; // (the old list stands: its host state is as it was)
	}
	s->hResetBodies.assign(bodies, bodies + bodyCount);
	s->hResetJoints.assign(joints, joints + jointCount);
	s->resetAgents = agents;
	s->resetSeed = seed;
	s->resetPasses = 0;
	s->resetCountsKnown = false, s->resetSourceOff = false;
	s->resetReport.stepFlags = 0; // the last pass's answers were of the list that left
	return S2AMD_OK;
}

int s2amd_world_set_reset_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2_RESET_KNOWN, flagsTurnedOn);
}

int s2amd_world_reset_agents(s2amdSolver* s, const int32_t* agents, int32_t count)
{
	const bool everybody = agents == nullptr && count == S2AMD_RESET_ALL;
	if (!s || (!everybody && (count < 0 || count > S2AMD_MAX_RESET_AGENTS || (count > 0 && !agents))))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (s->resetAgents <= 0)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_reset_agents: no reset list is set (s2amd_world_set_resets)");
	}
	for (int32_t i = 0; !everybody && i < count; ++i)
	{
		if (agents[i] < 0 || agents[i] >= s->resetAgents)
		{
			return fail(S2AMD_E_INVALID, "s2amd_world_reset_agents: entry " + std::to_string(i) + " is outside the list's agents: nothing was reset");
		}
	}
	if (!everybody && count == 0)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	const int* trigger = nullptr;
	if (!everybody)
	{
		// the pinned stage, one word per agent: written here, copied asynchronously.  The copy of the call before may still be reading it:
		// its event is waited for first (the edits' discipline, world_edit.hip).
		const size_t bytes = (size_t)s->resetAgents * sizeof(int32_t);
		if (int rc = s->resetStage.begin(bytes, (size_t)S2AMD_MAX_RESET_AGENTS * sizeof(int32_t)))
		{
			return rc;
		}
		int32_t* stage = (int32_t*)s->resetStage.buf.p;
		memset(stage, 0, bytes);
		for (int32_t i = 0; i < count; ++i)
		{
			stage[agents[i]] = 1;
		}
		char* at = (char*)s->dResets.p + layoutOf(s).trigger;
		HIP_TRY(hipMemcpyAsync(at, stage, bytes, hipMemcpyHostToDevice, s->stream));
		HIP_TRY(s->resetStage.record(s->stream));
		trigger = (const int*)at;
	}
	if (int rc = enqueuePass(s, trigger, s->resetAgents, ~0, everybody ? 1 : 0))
	{
		return rc;
	}
	s->resetReport.stepFlags = s->resetReport.flags; // the getters answer for this pass
	return S2AMD_OK;
}

int s2amd_world_reset_states(s2amdSolver* s, s2amdResetState* out, int32_t capacity, int32_t* count)
{
	const int rc = reportGetPerItem(ref(s), S2AMD_RESET_REPORT_STATES, "s2amd_world_reset_states", "s2amd_world_reset_states: buffer too small", out, capacity, count,
									s ? s->resetAgents : 0, true);
	if (rc || *count == 0)
	{
		return rc;
	}
	// (the set the last pass wrote; before any pass, set 0, which the setter zeroed)
	const size_t offset = layoutOf(s).states + (size_t)s->resetAgents * (size_t)(s->resetPasses & 1) * sizeof(s2amdResetState);
	return reportCopyOut(s, out, s->dResets, offset, *count, sizeof(s2amdResetState), hipMemcpyDeviceToHost);
}

int s2amd_world_reset_counts(s2amdSolver* s, int32_t counts[8])
{
	if (!s || !counts)
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	for (int k = 0; k < 8; ++k)
	{
		counts[k] = 0;
	}
	if (s->resetAgents <= 0)
	{
		return S2AMD_OK;
	}
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (!s->resetCountsKnown)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_reset_counts: no reset pass has run since the list was set and since the last upload (s2amd_world_set_reset_report, then a "
								   "step; or s2amd_world_reset_agents)");
	}
	if (s->resetSourceOff)
	{
		counts[7] = 1;
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	const int* set = (const int*)((const char*)s->dResets.p + layoutOf(s).counts) + 8 * (int)((s->resetPasses - 1) & 1);
	HIP_TRY(hipMemcpyAsync(counts, set, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop
