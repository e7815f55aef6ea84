// What the queries on the resident world share on the device (scene_query.hip, proximity_query.hip, contact_query.hip, shape_cast.hip;
// sensor_report.hip and force_field.hip use parts): the second half of the ballot-mask -> tile-prefix ->
// offsets -> write sequence that turns per-wave hit masks into CSR lists ascending by slot, the no-hit key of the single-answer queries
// with its decoding (keySlot), the query of a list entry (entryQuery), and a small host helper (queryState).  The candidate rule's box
// test is report_common.h's boxesOverlap.  The first half
// of the sequence -- the mask kernel -- is each file's own; the host side that drives it all is query_host.h.  Everything is in an unnamed
// namespace: each file holds its own copy of the kernels under the same names.
//
//   masks[((query * tiles) + tile) * 4 + wave]   the wave's hits of the query, bit = lane; every word is written by the mask kernel
//   listTilePrefixKernel  one wave per query: the exclusive prefix of the tiles' hit counts, and the query's total.
//   listOffsetsKernel     one wave: the CSR offsets over the queries.
//   listWriteKernel       one lane per ballot word: its set bits are consecutive entries of the query's list, at
//                         offsets[query] + hits of the tiles before + hits of the tile's waves before: ascending by slot, no sort, no atomic.
#pragma once

#include "report_common.h"

namespace
{

#define S2_QUERY_CHUNK S2_BLOCK // queries a workgroup stages: one per lane
#define S2_QUERY_MAX_COUNT (65535 * S2_QUERY_CHUNK)

S2_DEV int tileHits(const unsigned long long* masks, size_t tileWord)
{
	const ulonglong2 a = *(const ulonglong2*)(masks + tileWord), b = *(const ulonglong2*)(masks + tileWord + 2);
	return __popcll(a.x) + __popcll(a.y) + __popcll(b.x) + __popcll(b.y);
}

// inclusive sum over the wave's lanes
S2_DEV int waveInclusive(int v, int lane)
{
	for (int d = 1; d < 64; d <<= 1)
	{
		const int other = __shfl_up(v, d);
		if (lane >= d)
		{
			v += other;
		}
	}
	return v;
}

// tilePrefix[query * tiles + tile] = hits of the query in the tiles before; totals[query]
__global__ __launch_bounds__(S2_BLOCK) void listTilePrefixKernel(const unsigned long long* masks, int count, int tiles, int* tilePrefix, int* totals)
{
	const int lane = (int)(threadIdx.x & 63);
	const int q = (int)(blockIdx.x * (S2_BLOCK / 64) + (threadIdx.x >> 6));
	if (q >= count) // (whole waves)
	{
		return;
	}
	int carry = 0;
	for (int base = 0; base < tiles; base += 64)
	{
		const int t = base + lane;
		const int c = t < tiles ? tileHits(masks, ((size_t)q * tiles + t) * 4) : 0;
		const int inclusive = waveInclusive(c, lane);
		if (t < tiles)
		{
			tilePrefix[(size_t)q * tiles + t] = carry + inclusive - c;
		}
		carry += __shfl(inclusive, 63);
	}
	if (lane == 0)
	{
		totals[q] = carry;
	}
}

// offsets[0 .. count]: one wave
__global__ __launch_bounds__(64) void listOffsetsKernel(const int* totals, int count, int* offsets)
{
	const int lane = (int)threadIdx.x;
	int carry = 0;
	for (int base = 0; base < count; base += 64)
	{
		const int q = base + lane;
		const int c = q < count ? totals[q] : 0;
		const int inclusive = waveInclusive(c, lane);
		if (q < count)
		{
			offsets[q] = carry + inclusive - c;
		}
		carry += __shfl(inclusive, 63);
	}
	if (lane == 0)
	{
		offsets[count] = carry;
	}
}

// out[0 .. capacity): entries beyond the caller's capacity are dropped (the call answers S2AMD_E_CAPACITY from the offsets)
__global__ __launch_bounds__(S2_BLOCK) void listWriteKernel(const unsigned long long* masks, size_t words, int tiles, const int* tilePrefix, const int* offsets, int32_t* out,
															 int capacity)
{
	const size_t w = (size_t)blockIdx.x * S2_BLOCK + threadIdx.x;
	if (w >= words)
	{
		return;
	}
	unsigned long long m = masks[w];
	if (m == 0ull)
	{
		return;
	}
	const int wave = (int)(w & 3);
	const size_t qt = w >> 2;
	const int q = (int)(qt / (size_t)tiles), tile = (int)(qt % (size_t)tiles);
	int at = offsets[q] + tilePrefix[qt];
	for (int v = 0; v < wave; ++v)
	{
		at += __popcll(masks[w - wave + v]);
	}
	const int base = tile * S2_BLOCK + wave * 64;
	while (m != 0ull)
	{
		const int bit = __ffsll((long long)m) - 1;
		m &= m - 1ull;
		if (at < capacity)
		{
			out[at] = base + bit;
		}
		at += 1;
	}
}

// What the single-answer queries propose by a 64-bit integer atomic min: (an ordered key of the answer's figure) << 32 | slot, so the least
// key is the least figure, ties to the lowest slot.  The keys start as the no-hit key: every bit set.
#define S2_QUERY_NO_KEY 0xffffffffffffffffull

// the winner's slot; -1: nothing proposed
S2_DEV int keySlot(unsigned long long key)
{
	return key == S2_QUERY_NO_KEY ? -1 : (int)(uint32_t)(key & 0xffffffffull);
}

// the query of list entry e (0 <= e < offsets[count]): the last one whose offset is <= e
S2_DEV int entryQuery(const int* offsets, int count, int e)
{
	int lo = 0, hi = count; // offsets[lo] <= e < offsets[hi]
	while (hi - lo > 1)
	{
		const int mid = lo + (hi - lo) / 2;
		if (offsets[mid] <= e)
		{
			lo = mid;
		}
		else
		{
			hi = mid;
		}
	}
	return lo;
}

inline int queryState(const s2amdSolver* s)
{
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	return S2AMD_OK;
}

} // namespace
