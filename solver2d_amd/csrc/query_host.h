// The host side that the eight queries on the resident world share (scene_query.hip, proximity_query.hip, contact_query.hip,
// shape_cast.hip; DESIGN.md: "The query facility") and move-and-slide (mover_query.hip): how a call opens, the carver over the solver's query
// block, and the three drivers -- queryBest, one answer per query, queryLists, a list per query, and queryRounds, one answer per query found
// in several rounds of casts.  A query file supplies its kind (record size, the nouns of its error
// texts, its validator, what it stages on the device) and small functions that launch its own kernels with their own argument lists; its
// extern "C" bodies are one call into this header each.  Included after query_list.h, whose kernels queryLists launches: everything is in
// an unnamed namespace, so each file drives its own copy of them.
#pragma once

#include "query_list.h"

#include <cstring>

namespace
{

struct QueryCall;

// what tells one family of queries from another on the host
struct QueryKind
{
	size_t stride;				// bytes of one of the caller's records
	const char* plural;			// "more <plural> than one call takes", "<plural> x shape slots beyond 2^31"
	bool (*valid)(const void*); // one record; null: nothing to validate (point probes, box queries)
	const char* singular;		// "<singular> <index> <rule>": the first invalid record
	const char* rule;
	size_t staged[2];					   // bytes per query of up to two device arrays a stage kernel fills behind the upload (the contact queries); 0: none
	void (*stage)(const QueryCall&);		    // ... and its launch; null: nothing staged
};

// what a launch function gets: the resident arrays as the kernels take them, and where the call's own arrays lie in the query block
struct QueryCall
{
	hipStream_t stream;
	const s2amdShape* shapes;
	int ns, tiles; // shape slots, and tiles of S2_BLOCK slots
	const s2amdBody* bodies;
	const float2* origins;
	int nb;
	const void* records; // the caller's records as uploaded
	void* staged[2];
	int count;
	dim3 grid; // tiles x chunks of S2_QUERY_CHUNK queries: the candidates pass
};

inline bool queryBestArguments(const s2amdSolver* s, const void* records, int32_t count, const void* hits)
{
	return s && count >= 0 && (count == 0 || (records && hits));
}

inline bool queryListArguments(const s2amdSolver* s, const void* records, int32_t count, const int32_t* offsets, const void* payload, int32_t capacity, const int32_t* total)
{
	return s && count >= 0 && capacity >= 0 && total && (count == 0 || (records && offsets)) && (capacity == 0 || payload);
}

// How every call opens, in this order: the arguments, the state, count == 0 (S2AMD_OK with every output untouched), the batch limit,
// the records in index order.  *proceed is false when the call has been answered.
inline int queryOpen(s2amdSolver* s, bool arguments, const QueryKind& kind, const void* records, int32_t count, bool* proceed)
{
	*proceed = false;
	if (!arguments)
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (int rc = queryState(s))
	{
		return rc;
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	if (count > S2_QUERY_MAX_COUNT)
	{
		return fail(S2AMD_E_INVALID, std::string("more ") + kind.plural + " than one call takes: split the batch");
	}
	for (int32_t i = 0; kind.valid != nullptr && i < count; ++i)
	{
		if (!kind.valid((const char*)records + (size_t)i * kind.stride))
		{
			return fail(S2AMD_E_INVALID, std::string(kind.singular) + " " + std::to_string(i) + " " + kind.rule);
		}
	}
	*proceed = true;
	return S2AMD_OK;
}

// The carver over the query block: pieces of at least one byte, 256-byte aligned, in the order they are taken; then one ensure.
inline size_t queryTake(size_t& at, size_t bytes)
{
	return reportTake(at, bytes);
}

// where the pieces every call begins with lie: the caller's records, then what the kind stages
struct QueryInput
{
	size_t records, staged[2];
};

inline QueryInput queryTakeInput(size_t& at, const QueryKind& kind, int32_t count)
{
	QueryInput in = {queryTake(at, (size_t)count * kind.stride), {0, 0}};
	for (int k = 0; k < 2; ++k)
	{
		in.staged[k] = kind.staged[k] != 0 ? queryTake(at, (size_t)count * kind.staged[k]) : 0;
	}
	return in;
}

inline QueryCall queryCallOn(const s2amdSolver* s, const QueryKind& kind, const QueryInput& in, int32_t count)
{
	char* base = (char*)s->dQuery.p;
	const int tiles = (s->shapeCapacity + S2_BLOCK - 1) / S2_BLOCK;
	QueryCall c = {s->stream, (const s2amdShape*)s->dShapes.p, s->shapeCapacity, tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity,
				   base + in.records, {nullptr, nullptr}, count, dim3((unsigned)tiles, (unsigned)((count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK))};
	for (int k = 0; k < 2; ++k)
	{
		c.staged[k] = kind.staged[k] != 0 ? base + in.staged[k] : nullptr;
	}
	return c;
}

// One answer per query: {records, [staged], keys, hits} in the block; the upload, the keys to the no-hit key, [the stage kernel], the
// candidates pass on tiles x chunks (not launched on a world without shape slots: every key stays the no-hit key), the finish pass, one
// copy of the hits into the caller's array, one wait.
inline int queryBest(s2amdSolver* s, const QueryKind& kind, const void* records, int32_t count, void* hits, size_t hitBytes,
					 void (*candidates)(const QueryCall&, unsigned long long* keys), void (*finish)(const QueryCall&, const unsigned long long* keys, void* hits))
{
	bool proceed;
	if (int rc = queryOpen(s, queryBestArguments(s, records, count, hits), kind, records, count, &proceed))
	{
		return rc;
	}
	if (!proceed)
	{
		return S2AMD_OK;
	}
	size_t at = 0;
	const QueryInput in = queryTakeInput(at, kind, count);
	const size_t keysAt = queryTake(at, (size_t)count * sizeof(unsigned long long));
	const size_t hitsAt = queryTake(at, (size_t)count * hitBytes);
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	const QueryCall call = queryCallOn(s, kind, in, count);
	unsigned long long* keys = (unsigned long long*)(base + keysAt);
	HIP_TRY(hipMemcpyAsync(base + in.records, records, (size_t)count * kind.stride, hipMemcpyHostToDevice, call.stream));
	HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)count * sizeof(unsigned long long), call.stream));
	if (kind.stage != nullptr)
	{
		kind.stage(call);
	}
	if (call.tiles > 0)
	{
		candidates(call, keys);
	}
	finish(call, keys, base + hitsAt);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hits, base + hitsAt, (size_t)count * hitBytes, hipMemcpyDeviceToHost, call.stream));
	HIP_TRY(hipStreamSynchronize(call.stream));
	return S2AMD_OK;
}

// what a list call's lists are made of
struct QueryPayload
{
	size_t entryBytes;	  // 0: the shape slots themselves (and, beside them, the floats of perEntry where the caller passes `beside`);
						  // otherwise records of this size, which perEntry fills from the slots
	const char* tooSmall; // the text of S2AMD_E_CAPACITY
	// one lane per entry the lists hold (e < min(offsets[count], capacity)): its float, or its record
	void (*perEntry)(const QueryCall&, const int* offsets, const int32_t* slots, int capacity, void* out);
};

// A list per query, as CSR offsets over `count` queries and at most `capacity` entries ascending by slot.  On a world without shape
// slots the offsets are zeroed and *total is 0 without a launch.  Otherwise {records, [staged], masks, prefix, totals, [slots], out} in
// the block; the upload, [the stage kernel], the file's mask pass on tiles x chunks, query_list.h's three, the per-entry pass where
// there is one and the lists have room.  The answer comes back in one of two ways:
//   slots     out = {offsets, entries[, floats]}: one copy into hQueryStage and one wait, then split on the host -- an entry is 4 or 8
//             bytes, so copying all the caller has room for costs less than a second round trip;
//   records   out = {offsets, padding to 16 bytes, records}: the offsets into the caller's array and a wait, then -- only when
//             0 < total <= capacity -- the `total` records and a second wait: a record is tens of bytes, and only `total` of them exist.
// *total is offsets[count] either way; beyond `capacity` the call answers S2AMD_E_CAPACITY with the offsets and the total written and
// the payload untouched.
inline int queryLists(s2amdSolver* s, const QueryKind& kind, const void* records, int32_t count, int32_t* offsets, void* payload, float* beside, int32_t capacity, int32_t* total,
					  const QueryPayload& lists, void (*masksPass)(const QueryCall&, unsigned long long* masks))
{
	bool proceed;
	if (int rc = queryOpen(s, queryListArguments(s, records, count, offsets, payload, capacity, total), kind, records, count, &proceed))
	{
		return rc;
	}
	if (!proceed)
	{
		return S2AMD_OK;
	}
	const int ns = s->shapeCapacity;
	if (ns <= 0)
	{
		std::memset(offsets, 0, ((size_t)count + 1) * sizeof(int32_t));
		*total = 0;
		return S2AMD_OK;
	}
	const int tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	const size_t words = (size_t)count * tiles * 4;
	if ((size_t)count * (size_t)ns > (size_t)INT32_MAX)
	{
		return fail(S2AMD_E_INVALID, std::string(kind.plural) + " x shape slots beyond 2^31: split the batch");
	}
	// no list is longer than the shape slots, nor all together than the caller's capacity
	const size_t entries = std::min((size_t)capacity, (size_t)count * (size_t)ns);
	const bool asRecords = lists.entryBytes != 0;
	const size_t offsetsBytes = ((size_t)count + 1) * sizeof(int32_t);
	const size_t recordsIn = (offsetsBytes + 15) & ~size_t(15); // (records behind the offsets stay 16-byte aligned)
	const size_t outWords = (size_t)count + 1 + entries + (beside ? entries : 0);
	size_t at = 0;
	const QueryInput in = queryTakeInput(at, kind, count);
	const size_t masksAt = queryTake(at, words * sizeof(unsigned long long));
	const size_t prefixAt = queryTake(at, (size_t)count * tiles * sizeof(int));
	const size_t totalsAt = queryTake(at, (size_t)count * sizeof(int));
	const size_t slotsAt = asRecords ? queryTake(at, entries * sizeof(int32_t)) : 0;
	const size_t outAt = queryTake(at, asRecords ? recordsIn + entries * lists.entryBytes : outWords * sizeof(int32_t));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	const QueryCall call = queryCallOn(s, kind, in, count);
	hipStream_t st = call.stream;
	unsigned long long* masks = (unsigned long long*)(base + masksAt);
	int* dOffsets = (int*)(base + outAt);
	int32_t* dSlots = asRecords ? (int32_t*)(base + slotsAt) : dOffsets + count + 1;
	HIP_TRY(hipMemcpyAsync(base + in.records, records, (size_t)count * kind.stride, hipMemcpyHostToDevice, st));
	if (kind.stage != nullptr)
	{
		kind.stage(call);
	}
	masksPass(call, masks);
	listTilePrefixKernel<<<dim3((unsigned)((count + 3) / 4)), dim3(S2_BLOCK), 0, st>>>(masks, count, tiles, (int*)(base + prefixAt), (int*)(base + totalsAt));
	listOffsetsKernel<<<dim3(1), dim3(64), 0, st>>>((const int*)(base + totalsAt), count, dOffsets);
	listWriteKernel<<<gridFor(words), dim3(S2_BLOCK), 0, st>>>(masks, words, tiles, (const int*)(base + prefixAt), dOffsets, dSlots, (int)entries);
	if (entries > 0 && (asRecords || beside))
	{
		lists.perEntry(call, dOffsets, dSlots, (int)entries, asRecords ? (void*)(base + outAt + recordsIn) : (void*)(dSlots + entries));
	}
	HIP_TRY(hipGetLastError());
	if (asRecords)
	{
		HIP_TRY(hipMemcpyAsync(offsets, dOffsets, offsetsBytes, hipMemcpyDeviceToHost, st));
	}
	else
	{
		s->hQueryStage.resize(outWords);
		HIP_TRY(hipMemcpyAsync(s->hQueryStage.data(), dOffsets, outWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	if (!asRecords)
	{
		std::memcpy(offsets, s->hQueryStage.data(), offsetsBytes);
	}
	*total = offsets[count];
	if (*total > capacity)
	{
		return fail(S2AMD_E_CAPACITY, lists.tooSmall);
	}
	if (*total > 0 && asRecords)
	{
		HIP_TRY(hipMemcpyAsync(payload, base + outAt + recordsIn, (size_t)*total * lists.entryBytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	else if (*total > 0)
	{
		std::memcpy(payload, s->hQueryStage.data() + count + 1, (size_t)*total * sizeof(int32_t));
		if (beside)
		{
			std::memcpy(beside, s->hQueryStage.data() + count + 1 + entries, (size_t)*total * sizeof(float));
		}
	}
	return S2AMD_OK;
}

// what a call in rounds is made of, beside its kind (whose two staged arrays are the state the rounds work on, filled by kind.stage)
struct QueryRounds
{
	bool (*fits)(const s2amdSolver*, const void*); // one record against the resident world, after kind.valid has passed them all
	const char* fitsRule;						   // "<singular> <index> <fitsRule>"
	int (*rounds)(const void* records, int32_t count);
	size_t answerBytes, detailBytes; // per query: the answer, and the details behind it that the caller may decline (a null array)
	void (*candidates)(const QueryCall&, unsigned long long* keys);
	void (*advance)(const QueryCall&, unsigned long long* keys, void* answers, void* details);
};

// One answer per query that takes several casts to find, each from where the last one ended: {records, staged, keys, answers, details}
// in the block; the upload, the keys to the no-hit key, the answers and details to zero bytes, the stage kernel, then `rounds` times the
// candidates pass (not launched on a world without shape slots) and the advance pass, which consumes the keys and leaves them the no-hit
// key again -- no host wait in between.  One copy back and one wait: the answers straight into the caller's array when it declines the
// details, otherwise both into hQueryStage, split on the host.
inline int queryRounds(s2amdSolver* s, const QueryKind& kind, const void* records, int32_t count, void* answers, void* details, const QueryRounds& passes)
{
	bool proceed;
	if (int rc = queryOpen(s, queryBestArguments(s, records, count, answers), kind, records, count, &proceed))
	{
		return rc;
	}
	if (!proceed)
	{
		return S2AMD_OK;
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!passes.fits(s, (const char*)records + (size_t)i * kind.stride))
		{
			return fail(S2AMD_E_INVALID, std::string(kind.singular) + " " + std::to_string(i) + " " + passes.fitsRule);
		}
	}
	const size_t answersBytes = (size_t)count * passes.answerBytes, outBytes = answersBytes + (size_t)count * passes.detailBytes;
	size_t at = 0;
	const QueryInput in = queryTakeInput(at, kind, count);
	const size_t keysAt = queryTake(at, (size_t)count * sizeof(unsigned long long));
	const size_t outAt = queryTake(at, outBytes);
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	const QueryCall call = queryCallOn(s, kind, in, count);
	unsigned long long* keys = (unsigned long long*)(base + keysAt);
	HIP_TRY(hipMemcpyAsync(base + in.records, records, (size_t)count * kind.stride, hipMemcpyHostToDevice, call.stream));
	HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)count * sizeof(unsigned long long), call.stream));
	HIP_TRY(hipMemsetAsync(base + outAt, 0, outBytes, call.stream));
	kind.stage(call);
	const int rounds = passes.rounds(records, count);
	for (int round = 0; round < rounds; ++round)
	{
		if (call.tiles > 0)
		{
			passes.candidates(call, keys);
		}
		passes.advance(call, keys, base + outAt, base + outAt + answersBytes);
	}
	HIP_TRY(hipGetLastError());
	if (details == nullptr)
	{
		HIP_TRY(hipMemcpyAsync(answers, base + outAt, answersBytes, hipMemcpyDeviceToHost, call.stream));
		HIP_TRY(hipStreamSynchronize(call.stream));
		return S2AMD_OK;
	}
	s->hQueryStage.resize((outBytes + sizeof(int32_t) - 1) / sizeof(int32_t));
	HIP_TRY(hipMemcpyAsync(s->hQueryStage.data(), base + outAt, outBytes, hipMemcpyDeviceToHost, call.stream));
	HIP_TRY(hipStreamSynchronize(call.stream));
	std::memcpy(answers, s->hQueryStage.data(), answersBytes);
	std::memcpy(details, (const char*)s->hQueryStage.data() + answersBytes, outBytes - answersBytes);
	return S2AMD_OK;
}

} // namespace
