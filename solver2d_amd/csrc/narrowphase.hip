// Narrow phase, behind the same C-ABI:
//   s2amd_update_contacts == Stage 3 of s2World_Step, "update contacts" (src/world.c:132-168): per live contact
//   whose fat AABBs still overlap, s2UpdateContact (src/contact.c:296-358) -- the manifold function of the
//   shape-type pair, then the feature-id matching that carries impulses and the sticky-friction cache over.
//
// One thread per contact slot; the reference walks the pool on one core.  The two polygons of a pair (B
// already moved into A's frame, as s2CollidePolygons does) live in LDS because GJK addresses their vertices by
// computed index; everything else is registers.  All arithmetic is fp32 in the reference's operation order
// (-ffp-contract=off), so manifolds, feature ids and simplex caches are bit-identical to the reference's
// (tests/test_gpu_narrowphase.py against captures of the unmodified reference and the oracle).
//
// The manifold functions themselves are manifold_ops.h (shared with contact_query.hip); GJK with its simplex
// cache is gjk_ops.h.

#include "launch.h"
#include "s2_device.h"

#include "solver2d_amd.h"

#include <cfloat>
#include <cstring>
#include <string>

#define S2_NP_BLOCK 128
#define S2_NP_SPECULATIVE (4.0f * S2_LINEAR_SLOP) // constants.h:8
#define S2_NP_MAX_VERTS 8

#include "manifold_ops.h"

int s2amdFail(int code, const std::string& msg);
hipStream_t s2amdStream(s2amdSolver* s);
int s2amdDevice(s2amdSolver* s);
void s2amdRecordDeviceMs(s2amdSolver* s, float ms);

namespace
{

// one contact slot of stage 3; returns S2AMD_PAIR_*.  lds: the block's 4 * S2_NP_MAX_VERTS * S2_NP_BLOCK float2 staging area
S2_DEV int updateContactOne(const s2amdBody* bodies, const float2* origins, const s2amdShape* shapes, s2amdPairState* ps, s2amdContact* ct, float2* lds)
{
	if (ps->shapeA < 0 || ps->shapeB < 0)
	{
		return S2AMD_PAIR_FREE;
	}
	const s2amdShape* shapeA = shapes + ps->shapeA;
	const s2amdShape* shapeB = shapes + ps->shapeB;
	{
		// s2AABB_Overlaps on the fat boxes: aabb.h:111-123, src/world.c:149-167
		float d1x = shapeB->fatAABB[0] - shapeA->fatAABB[2], d1y = shapeB->fatAABB[1] - shapeA->fatAABB[3];
		float d2x = shapeA->fatAABB[0] - shapeB->fatAABB[2], d2y = shapeA->fatAABB[1] - shapeB->fatAABB[3];
		if (d1x > 0.0f || d1y > 0.0f || d2x > 0.0f || d2y > 0.0f)
		{
			return S2AMD_PAIR_SEPARATED;
		}
	}
	const int bodyA = shapeA->body, bodyB = shapeB->body;
	Xf xfA, xfB;
	xfA.p = v2(origins[bodyA].x, origins[bodyA].y);
	xfA.q.s = bodies[bodyA].rot[0], xfA.q.c = bodies[bodyA].rot[1];
	xfB.p = v2(origins[bodyB].x, origins[bodyB].y);
	xfB.q.s = bodies[bodyB].rot[0], xfB.q.c = bodies[bodyB].rot[1];

	Cache cache;
	cache.metric = ps->cacheMetric;
	cache.count = ps->cacheCount;
	for (int k = 0; k < 3; ++k)
	{
		cache.indexA[k] = ps->cacheIndexA[k];
		cache.indexB[k] = ps->cacheIndexB[k];
	}

	// the manifold function of the ordered type pair (src/contact.c:139-151)
	const int ta = shapeA->type, tb = shapeB->type;
	Manifold m = emptyManifold();
	PolyRef pa, pb;
	pa.verts = lds + threadIdx.x;
	pa.norms = lds + S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	pb.verts = lds + 2 * S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	pb.norms = lds + 3 * S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	const V2 a0 = v2(shapeA->vertices[0][0], shapeA->vertices[0][1]), a1 = v2(shapeA->vertices[1][0], shapeA->vertices[1][1]);
	const V2 b0 = v2(shapeB->vertices[0][0], shapeB->vertices[0][1]);
	if (tb == S2AMD_SHAPE_CIRCLE)
	{
		if (ta == S2AMD_SHAPE_CIRCLE)
		{
			m = collideCircles(a0, shapeA->radius, xfA, b0, shapeB->radius, xfB);
		}
		else if (ta == S2AMD_SHAPE_CAPSULE || ta == S2AMD_SHAPE_SEGMENT)
		{
			m = collideCapsuleAndCircle(a0, a1, ta == S2AMD_SHAPE_CAPSULE ? shapeA->radius : 0.0f, xfA, b0, shapeB->radius, xfB);
		}
		else if (ta == S2AMD_SHAPE_POLYGON)
		{
			stagePolygon(shapeA, pa, false, xfA, &pa.radius, &pa.count);
			m = collidePolygonAndCircle(pa, xfA, b0, shapeB->radius, xfB);
		}
	}
	else if ((ta == S2AMD_SHAPE_CAPSULE && tb == S2AMD_SHAPE_CAPSULE) || (ta == S2AMD_SHAPE_POLYGON && tb == S2AMD_SHAPE_CAPSULE) ||
			 (ta == S2AMD_SHAPE_POLYGON && tb == S2AMD_SHAPE_POLYGON) || (ta == S2AMD_SHAPE_SEGMENT && tb == S2AMD_SHAPE_CAPSULE) ||
			 (ta == S2AMD_SHAPE_SEGMENT && tb == S2AMD_SHAPE_POLYGON))
	{
		Xf xf = xfInvMul(xfA, xfB);
		stagePolygon(shapeA, pa, false, xf, &pa.radius, &pa.count);
		stagePolygon(shapeB, pb, true, xf, &pb.radius, &pb.count);
		m = collidePolygons(pa, xfA, pb, xf, cache);
	}

	// s2UpdateContact: src/contact.c:296-358
	const int oldCount = ct->pointCount;
	const uint32_t oldId0 = ps->id[0], oldId1 = ps->id[1];
	s2amdManifoldPoint oldPoints[2] = {ct->points[0], ct->points[1]};
	int frictionPersisted = m.pointCount == oldCount ? 1 : 0;
	ct->pointCount = m.pointCount;
	ct->normal[0] = m.normal.x, ct->normal[1] = m.normal.y;
	for (int p = 0; p < 2; ++p)
	{
		s2amdManifoldPoint q;
		memset(&q, 0, sizeof(q));
		uint32_t id = 0u;
		int persisted = 0;
		if (p < m.pointCount)
		{
			const MPoint& mp = m.points[p];
			q.localAnchorA[0] = mp.localAnchorA.x, q.localAnchorA[1] = mp.localAnchorA.y;
			q.localAnchorB[0] = mp.localAnchorB.x, q.localAnchorB[1] = mp.localAnchorB.y;
			q.separation = mp.separation;
			id = mp.id;
			for (int j = 0; j < oldCount && j < 2; ++j)
			{
				if ((j == 0 ? oldId0 : oldId1) == id)
				{
					const s2amdManifoldPoint& o = oldPoints[j];
					q.frictionNormalA[0] = o.frictionNormalA[0], q.frictionNormalA[1] = o.frictionNormalA[1];
					q.frictionNormalB[0] = o.frictionNormalB[0], q.frictionNormalB[1] = o.frictionNormalB[1];
					q.frictionAnchorA[0] = o.frictionAnchorA[0], q.frictionAnchorA[1] = o.frictionAnchorA[1];
					q.frictionAnchorB[0] = o.frictionAnchorB[0], q.frictionAnchorB[1] = o.frictionAnchorB[1];
					q.normalImpulse = o.normalImpulse;
					q.tangentImpulse = o.tangentImpulse;
					persisted = 1;
					break;
				}
			}
			if (!persisted)
			{
				frictionPersisted = 0;
			}
		}
		ct->points[p] = q;
		ps->id[p] = (uint16_t)id;
		ps->persisted[p] = (uint8_t)persisted;
	}
	ct->frictionPersisted = frictionPersisted;
	ps->cacheMetric = cache.metric;
	ps->cacheCount = (uint16_t)cache.count;
	for (int k = 0; k < 3; ++k)
	{
		ps->cacheIndexA[k] = (uint8_t)cache.indexA[k];
		ps->cacheIndexB[k] = (uint8_t)cache.indexB[k];
	}
	return S2AMD_PAIR_UPDATED;
}

// SUMMARY (resident world, world.hip): a separated pair is destroyed the way src/world.c:149-167 destroys its contact (no
// manifold, free pair slot), the slot's point count is compared with the previous step's byte, and the step's counters
// {separated, active, flips, moves} are accumulated in summary[0..3].
template <bool SUMMARY>
__global__ __launch_bounds__(S2_NP_BLOCK) void updateContactsKernel(const s2amdBody* bodies, const float2* origins, const s2amdShape* shapes,
																	 s2amdPairState* pairs, s2amdContact* contacts, int contactCapacity, int32_t* status,
																	 uint8_t* pointBytes, int* summary, int* separatedSlots, const uint8_t* watched)
{
	__shared__ float2 lds[4 * S2_NP_MAX_VERTS * S2_NP_BLOCK]; // vertsA, normsA, vertsB, normsB: 32 KiB
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	int pc = 0;
	if (i < contactCapacity)
	{
		int st = updateContactOne(bodies, origins, shapes, pairs + i, contacts + i, lds);
		status[i] = st;
		if (SUMMARY)
		{
			if (st == S2AMD_PAIR_SEPARATED)
			{
				contacts[i].pointCount = 0;
				pairs[i].shapeA = -1;
				pairs[i].shapeB = -1;
				separatedSlots[atomicAdd(summary + 0, 1)] = i; // the caller's s2DestroyContact list (s2amd_world_separated)
			}
			else
			{
				pc = contacts[i].pointCount;
				pc = pc > 0 ? pc : 0;
			}
			int old = pointBytes[i];
			if (old != pc)
			{
				pointBytes[i] = (uint8_t)pc;
				atomicAdd(summary + 3, 1);
				if ((old > 0) != (pc > 0))
				{
					atomicAdd(summary + 2, 1);
					if (watched != nullptr && watched[i])
					{
						atomicAdd(summary + 5, 1); // on a hub body that is a change of the constraint graph (solver_internal.h: hContactWatched)
					}
				}
			}
		}
	}
	if (SUMMARY)
	{
		unsigned long long live = __ballot(pc > 0);
		if ((threadIdx.x & 63) == 0 && live != 0ull)
		{
			atomicAdd(summary + 1, __popcll(live));
		}
	}
}

struct Scratch
{
	void* p = nullptr;
	~Scratch()
	{
		if (p)
		{
			(void)hipFree(p);
		}
	}
};

} // namespace

#define NP_TRY(expr)                                                                                                             \
	do                                                                                                                           \
	{                                                                                                                            \
		hipError_t _e = (expr);                                                                                                  \
		if (_e != hipSuccess)                                                                                                    \
		{                                                                                                                        \
			return s2amdFail(S2AMD_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));                                 \
		}                                                                                                                        \
	} while (0)

// resident arrays (world.hip)
void launchUpdateContacts(hipStream_t st, const s2amdBody* bodies, const float* origins, const s2amdShape* shapes, s2amdPairState* pairs,
						  s2amdContact* contacts, int contactCapacity, int32_t* status, uint8_t* pointBytes, int* summary, int* separatedSlots, const uint8_t* watched)
{
	if (contactCapacity <= 0)
	{
		return;
	}
	dim3 grid((unsigned)((contactCapacity + S2_NP_BLOCK - 1) / S2_NP_BLOCK));
	updateContactsKernel<true><<<grid, dim3(S2_NP_BLOCK), 0, st>>>(bodies, (const float2*)origins, shapes, pairs, contacts, contactCapacity, status,
																   pointBytes, summary, separatedSlots, watched);
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_update_contacts(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const float* origins, const s2amdShape* shapes,
						  int32_t shapeCapacity, s2amdPairState* pairs, s2amdContact* contacts, int32_t contactCapacity, int32_t* status)
{
	if (!solver || bodyCapacity < 0 || shapeCapacity < 0 || contactCapacity < 0 || (bodyCapacity > 0 && (!bodies || !origins)) ||
		(shapeCapacity > 0 && !shapes) || (contactCapacity > 0 && (!pairs || !contacts || !status)))
	{
		return s2amdFail(S2AMD_E_INVALID, "bad argument");
	}
	if (contactCapacity == 0)
	{
		return S2AMD_OK;
	}
	for (int i = 0; i < contactCapacity; ++i)
	{
		if (pairs[i].shapeA >= shapeCapacity || pairs[i].shapeB >= shapeCapacity)
		{
			return s2amdFail(S2AMD_E_INVALID, "pair " + std::to_string(i) + " names a shape outside the shape array");
		}
	}
	NP_TRY(hipSetDevice(s2amdDevice(solver)));
	hipStream_t st = s2amdStream(solver);
	auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
	size_t bBytes = (size_t)bodyCapacity * sizeof(s2amdBody), oBytes = (size_t)bodyCapacity * sizeof(float2);
	size_t sBytes = (size_t)shapeCapacity * sizeof(s2amdShape), pBytes = (size_t)contactCapacity * sizeof(s2amdPairState);
	size_t cBytes = (size_t)contactCapacity * sizeof(s2amdContact), tBytes = (size_t)contactCapacity * sizeof(int32_t);
	Scratch buf;
	NP_TRY(hipMalloc(&buf.p, al(bBytes) + al(oBytes) + al(sBytes) + al(pBytes) + al(cBytes) + al(tBytes) + 256));
	char* base = (char*)buf.p;
	s2amdBody* dB = (s2amdBody*)base;
	float2* dO = (float2*)(base + al(bBytes));
	s2amdShape* dS = (s2amdShape*)((char*)dO + al(oBytes));
	s2amdPairState* dP = (s2amdPairState*)((char*)dS + al(sBytes));
	s2amdContact* dC = (s2amdContact*)((char*)dP + al(pBytes));
	int32_t* dT = (int32_t*)((char*)dC + al(cBytes));
	if (bodyCapacity > 0)
	{
		NP_TRY(hipMemcpyAsync(dB, bodies, bBytes, hipMemcpyHostToDevice, st));
		NP_TRY(hipMemcpyAsync(dO, origins, oBytes, hipMemcpyHostToDevice, st));
	}
	if (shapeCapacity > 0)
	{
		NP_TRY(hipMemcpyAsync(dS, shapes, sBytes, hipMemcpyHostToDevice, st));
	}
	NP_TRY(hipMemcpyAsync(dP, pairs, pBytes, hipMemcpyHostToDevice, st));
	NP_TRY(hipMemcpyAsync(dC, contacts, cBytes, hipMemcpyHostToDevice, st));
	dim3 grid((unsigned)((contactCapacity + S2_NP_BLOCK - 1) / S2_NP_BLOCK));
	hipEvent_t e0 = nullptr, e1 = nullptr;
	NP_TRY(hipEventCreate(&e0));
	NP_TRY(hipEventCreate(&e1));
	NP_TRY(hipEventRecord(e0, st));
	updateContactsKernel<false><<<grid, dim3(S2_NP_BLOCK), 0, st>>>(dB, dO, dS, dP, dC, contactCapacity, dT, nullptr, nullptr, nullptr, nullptr);
	NP_TRY(hipEventRecord(e1, st));
	NP_TRY(hipGetLastError());
	NP_TRY(hipMemcpyAsync(pairs, dP, pBytes, hipMemcpyDeviceToHost, st));
	NP_TRY(hipMemcpyAsync(contacts, dC, cBytes, hipMemcpyDeviceToHost, st));
	NP_TRY(hipMemcpyAsync(status, dT, tBytes, hipMemcpyDeviceToHost, st));
	NP_TRY(hipStreamSynchronize(st));
	float ms = 0.0f;
	(void)hipEventElapsedTime(&ms, e0, e1);
	s2amdRecordDeviceMs(solver, ms); // kernel only; the call's wall time is dominated by the host <-> device copies
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop

S2_DEFINE_WARM(narrowphase)
