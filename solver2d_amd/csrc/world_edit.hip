// World edits on the resident world (include/solver2d_amd.h: s2amd_world_edit): the reference's eight per-frame setters --
// s2Body_SetLinearVelocity, _SetAngularVelocity, _ApplyForceToCenter, _ApplyLinearImpulse (src/body.c:337-370), s2MouseJoint_SetTarget
// (src/mouse_joint.c:18-29), s2RevoluteJoint_EnableLimit, _EnableMotor, _SetMotorSpeed (src/revolute_joint.c:890-927) -- as writes into
// the wire records the device owns between steps.  Nothing is downloaded, nothing is marked stale, the structure is kept: an edit
// changes no field a colouring, a strip table or a tree was made from.  Everything is enqueued on the solver's stream, so a call lands
// after the step before it and before the step after it.
//
// The statement (the header) is sequential: edits[0], edits[1], ... one after another.  An edit reads and writes its own target's
// record only, so only the order of the edits ON ONE TARGET matters -- to the bit, because force adds and impulse adds are float sums.
// The host's validation pass looks at every record anyway; it also stamps every target (one word per body slot and per joint slot,
// a generation counter instead of a clear) and so knows whether any target occurs twice.
//
//   all targets distinct   editDistinctKernel: one lane per edit.  The lane reads its record's type word and the fields its kind reads,
//                          and writes the fields of its kind.
//   a target twice         editKeysKernel writes key = (joint ? 1 : 0) << 63 | target << 32 | list index; rocPRIM's radix sort orders the
//                          keys (they are unique, so the result does not depend on the sort's internals); editWalkKernel: one lane per
//                          sorted key, the first lane of a target's segment walks the segment -- its edits in list order -- with the
//                          record's edited fields in registers, and writes them once.  A list that puts thousands of edits on one body is
//                          walked by one lane: correct, not fast.
//
// The skip count (a free slot, a joint of the other type): a wave ballot (distinct) or a wave sum (walk), then one integer atomic per
// wave that has any.  No float atomics.  The arithmetic is fp32 in the reference's operation order; this file is compiled without
// contraction in both libraries (Makefile), because the result is stated bit for bit.
#include "solver_internal.h"

#include "report_common.h"
#include "edit_ops.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>

namespace
{

#define S2_EDIT_LAST_KIND S2AMD_EDIT_REVOLUTE_SET_MOTOR_SPEED

// All targets distinct: one lane per edit.  The host has checked kind and target of every record against the capacities.
__global__ __launch_bounds__(S2_BLOCK) void editDistinctKernel(const s2amdWorldEdit* edits, int count, s2amdBody* bodies, s2amdJoint* joints, int* skipped)
{
	const size_t i = (size_t)blockIdx.x * S2_BLOCK + threadIdx.x;
	bool skip = false;
	if (i < (size_t)count)
	{
		const s2amdWorldEdit e = loadEdit(edits, i);
		if (e.kind < S2_EDIT_FIRST_JOINT_KIND)
		{
			s2amdBody* b = bodies + e.target;
			BodyFixed k;
			BodyFields f;
			loadBody(b, k, f);
			skip = k.type == S2AMD_BODY_FREE;
			if (!skip)
			{
				applyBodyEdit(e, k, f);
				storeBody(b, f);
			}
		}
		else
		{
			s2amdJoint* j = joints + e.target;
			JointFields f;
			loadJoint(j, f);
			skip = !applyJointEdit(e, j->type, f);
			storeJoint(j, f);
		}
	}
	if (skipped != nullptr)
	{
		const unsigned long long m = __ballot(skip);
		if (m != 0ull && (threadIdx.x & 63) == 0)
		{
			atomicAdd(skipped, __popcll(m));
		}
	}
}

// the sort key of edit i: joints behind bodies, then the target, then the place in the list
__global__ __launch_bounds__(S2_BLOCK) void editKeysKernel(const s2amdWorldEdit* edits, int count, unsigned long long* keys)
{
	const size_t i = (size_t)blockIdx.x * S2_BLOCK + threadIdx.x;
	if (i >= (size_t)count)
	{
		return;
	}
	const int2 kt = *(const int2*)(edits + i); // {kind, target}
	const unsigned int who = (kt.x >= S2_EDIT_FIRST_JOINT_KIND ? 0x80000000u : 0u) | (unsigned int)kt.y;
	keys[i] = ((unsigned long long)who << 32) | (unsigned long long)i;
}

// Repeated targets: one lane per sorted key; the first lane of a target's segment walks it.
__global__ __launch_bounds__(S2_BLOCK) void editWalkKernel(const s2amdWorldEdit* edits, const unsigned long long* keys, int count, s2amdBody* bodies, s2amdJoint* joints,
															 int* skipped)
{
	const size_t i = (size_t)blockIdx.x * S2_BLOCK + threadIdx.x;
	int skips = 0;
	if (i < (size_t)count)
	{
		const unsigned int who = (unsigned int)(keys[i] >> 32);
		if (i == 0 || (unsigned int)(keys[i - 1] >> 32) != who)
		{
			const int target = (int)(who & 0x7fffffffu);
			if ((who & 0x80000000u) == 0u)
			{
				s2amdBody* b = bodies + target;
				BodyFixed k;
				BodyFields f;
				loadBody(b, k, f);
				for (size_t at = i; at < (size_t)count && (unsigned int)(keys[at] >> 32) == who; ++at)
				{
					if (k.type == S2AMD_BODY_FREE)
					{
						skips += 1;
						continue;
					}
					applyBodyEdit(loadEdit(edits, (size_t)(unsigned int)keys[at]), k, f);
				}
				storeBody(b, f);
			}
			else
			{
				s2amdJoint* j = joints + target;
				const int type = j->type;
				JointFields f;
				loadJoint(j, f);
				for (size_t at = i; at < (size_t)count && (unsigned int)(keys[at] >> 32) == who; ++at)
				{
					skips += applyJointEdit(loadEdit(edits, (size_t)(unsigned int)keys[at]), type, f) ? 0 : 1;
				}
				storeJoint(j, f);
			}
		}
	}
	if (skipped != nullptr)
	{
		// the wave's sum, then one atomic
		for (int offset = 32; offset > 0; offset >>= 1)
		{
			skips += __shfl_down(skips, offset, 64);
		}
		if ((threadIdx.x & 63) == 0 && skips != 0)
		{
			atomicAdd(skipped, skips);
		}
	}
}

// The pass over the caller's list: every record checked, copied to the pinned stage, its target stamped.  -1: a record is invalid
// (*bad is its index); 0: all targets distinct; 1: some target occurs twice.
int checkAndStage(s2amdSolver* s, const s2amdWorldEdit* edits, int32_t count, int32_t* bad)
{
	const int nb = s->bodyCapacity, nj = s->jointCapacity;
	if ((int)s->hEditBodyStamp.size() != nb || (int)s->hEditJointStamp.size() != nj || s->editGeneration == UINT32_MAX)
	{
		s->hEditBodyStamp.assign((size_t)nb, 0u);
		s->hEditJointStamp.assign((size_t)nj, 0u);
		s->editGeneration = 0;
	}
	const uint32_t generation = ++s->editGeneration;
	s2amdWorldEdit* stage = (s2amdWorldEdit*)s->editStage.buf.p;
	bool repeated = false;
	for (int32_t i = 0; i < count; ++i)
	{
		const s2amdWorldEdit& e = edits[i];
		const bool joint = e.kind >= S2_EDIT_FIRST_JOINT_KIND;
		if (e.kind < S2AMD_EDIT_BODY_SET_LINEAR_VELOCITY || e.kind > S2_EDIT_LAST_KIND || e.reserved != 0 || e.target < 0 || e.target >= (joint ? nj : nb))
		{
			*bad = i;
			return -1;
		}
		uint32_t& stamp = joint ? s->hEditJointStamp[(size_t)e.target] : s->hEditBodyStamp[(size_t)e.target];
		repeated = repeated || stamp == generation;
		stamp = generation;
		stage[i] = e;
	}
	return repeated ? 1 : 0;
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_edit(s2amdSolver* s, const s2amdWorldEdit* edits, int32_t count, int32_t* skipped)
{
	if (!s || count < 0 || (count > 0 && !edits))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (count == 0)
	{
		if (skipped)
		{
			*skipped = 0;
		}
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	hipStream_t st = s->stream;
	// the pinned stage: the caller's list is copied while it is checked, so the caller may reuse it at once and the copy to the device
	// is a true asynchronous one.  The copy of the call before may still be reading the stage: its event is waited for first.
	const size_t listBytes = (size_t)count * sizeof(s2amdWorldEdit);
	if (int rc = s->editStage.begin(listBytes, std::max(reportRound(listBytes + listBytes / 2), (size_t)4096)))
	{
		return rc;
	}
	int32_t bad = -1;
	const int repeated = checkAndStage(s, edits, count, &bad);
	if (repeated < 0)
	{
		return fail(S2AMD_E_INVALID, "world edit " + std::to_string(bad) +
										 " is invalid (a kind outside 1..8, a target outside the uploaded capacity, reserved != 0): nothing was applied");
	}
	// dEdit: {the skip count, the list, [the keys, the sorted keys, rocPRIM's scratch]}
	size_t at = 0;
	(void)reportTake(at, sizeof(int));
	const size_t listAt = reportTake(at, listBytes);
	size_t keysAt = 0, sortedAt = 0, tmpAt = 0, tmpBytes = 0;
	if (repeated)
	{
		HIP_TRY(rocprim::radix_sort_keys(nullptr, tmpBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)count, 0, 64, st));
		keysAt = reportTake(at, (size_t)count * sizeof(unsigned long long));
		sortedAt = reportTake(at, (size_t)count * sizeof(unsigned long long));
		tmpAt = reportTake(at, tmpBytes);
	}
	if (int rc = s->dEdit.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dEdit.p;
	int* dSkipped = skipped ? (int*)base : nullptr;
	const s2amdWorldEdit* dList = (const s2amdWorldEdit*)(base + listAt);
	if (skipped)
	{
		HIP_TRY(hipMemsetAsync(base, 0, sizeof(int), st));
	}
	HIP_TRY(hipMemcpyAsync(base + listAt, s->editStage.buf.p, listBytes, hipMemcpyHostToDevice, st));
	HIP_TRY(s->editStage.record(st));
	s2amdBody* bodies = (s2amdBody*)s->dBodies.p;
	s2amdJoint* joints = (s2amdJoint*)s->dJoints.p;
	if (!repeated)
	{
		editDistinctKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>(dList, count, bodies, joints, dSkipped);
	}
	else
	{
		unsigned long long* keys = (unsigned long long*)(base + keysAt);
		unsigned long long* sorted = (unsigned long long*)(base + sortedAt);
		editKeysKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>(dList, count, keys);
		HIP_TRY(rocprim::radix_sort_keys(base + tmpAt, tmpBytes, keys, sorted, (size_t)count, 0, 64, st));
		editWalkKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>(dList, sorted, count, bodies, joints, dSkipped);
	}
	HIP_TRY(hipGetLastError());
	if (skipped)
	{
		HIP_TRY(hipMemcpyAsync(skipped, base, sizeof(int), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop
