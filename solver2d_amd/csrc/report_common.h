// What the reports, queries and lists of the resident world share on the device: the candidate rules' box test, the live-body test and
// the clamp rule of the actuators and observers, the ordered compaction's tile-prefix step, the body-range kernel behind the stable
// radix sort by body, and the one-wave ordered sum's pieces.  Everything is in an unnamed namespace: each of the files holds its own
// copy of the kernel below under the same name.
#pragma once

#include "solver_internal.h"

#define S2_BLOCK 256

namespace
{

// bits of a body key: every body slot and the value `nb` itself (the key of an entry that belongs to no body)
inline unsigned int bodyKeyBits(int nb)
{
	unsigned int bits = 1;
	while (bits < 32 && (1u << bits) <= (unsigned int)nb)
	{
		bits += 1;
	}
	return bits;
}

inline dim3 gridFor(size_t n)
{
	return dim3((unsigned)((n + S2_BLOCK - 1) / S2_BLOCK));
}

// s2TransformPoint (include/solver2d/math.h:350-356), rot = {s, c}
S2_DEV float2 transformPoint(float2 origin, float2 rot, float2 p)
{
	const float x = (rot.y * p.x - rot.x * p.y) + origin.x;
	const float y = (rot.x * p.x + rot.y * p.y) + origin.y;
	return make_float2(x, y);
}

// s2AABB_Overlaps(fat, box), include/solver2d/aabb.h:111-123: false only when one of the four differences is > 0
S2_DEV bool boxesOverlap(const float* fat, float lx, float ly, float ux, float uy)
{
	const float d1x = lx - fat[2], d1y = ly - fat[3];
	const float d2x = fat[0] - ux, d2y = fat[1] - uy;
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

// a body of the array that is in use: what a list entry may be mounted on, what an observer may read
S2_DEV bool liveBody(const s2amdBody* bodies, int nb, int body)
{
	return body >= 0 && body < nb && bodies[body].type != S2AMD_BODY_FREE;
}

// clamp(gain * x + bias, lower, upper), one operation at a time: an actuator's command, an observer's value.  A NaN fails both
// comparisons and passes through.
S2_DEV float clampedAffine(float x, float gain, float bias, float lower, float upper)
{
	float t = gain * x;
	t = t + bias;
	return t < lower ? lower : (t > upper ? upper : t);
}

// The tile-prefix step of an ordered compaction: this lane's share of the sum of list `list`'s per-tile counts (counts[list * tiles + b])
// over the tiles before `tile`; the caller adds the 64 shares up (the xor-shuffle sum stays with the caller: folded in here, the
// compiler schedules one instruction of the contact report's reportWriteKernel differently, and that kernel is to stay as it was).
S2_DEV int tileCountsBefore(const int* counts, int tiles, int list, int tile, int lane)
{
	int partial = 0;
	for (int b = lane; b < tile; b += 64)
	{
		partial += counts[list * tiles + b];
	}
	return partial;
}

// ranges[2 * body] .. ranges[2 * body + 1]: the body's run in the sorted entries (both zero, from the memset, for a body without any)
__global__ __launch_bounds__(S2_BLOCK) void reportBodyRangesKernel(const uint32_t* keys, int n, int nb, int* ranges)
{
	const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (e >= n)
	{
		return;
	}
	const uint32_t key = keys[e];
	if (key >= (uint32_t)nb)
	{
		return;
	}
	if (e == 0 || keys[e - 1] != key)
	{
		ranges[2 * key] = e;
	}
	if (e == n - 1 || keys[e + 1] != key)
	{
		ranges[2 * key + 1] = e + 1;
	}
}

S2_DEV float laneOf(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

S2_DEV void waveLdsOrder()
{
	// LDS operations of one wave execute in order: this only keeps the compiler from moving them across
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc += comp[0], += comp[1], ... in that order: one dependent add per term (jacobi_kernel.hip: addInOrder)
S2_DEV float addInOrder(float acc, const float* comp, int n)
{
	int k = 0;
	for (; k + 8 <= n; k += 8)
	{
		const float4 a = *(const float4*)(comp + k), b = *(const float4*)(comp + k + 4);
		acc = acc + a.x, acc = acc + a.y, acc = acc + a.z, acc = acc + a.w;
		acc = acc + b.x, acc = acc + b.y, acc = acc + b.z, acc = acc + b.w;
	}
	for (; k < n; ++k)
	{
		acc = acc + comp[k];
	}
	return acc;
}

} // namespace
