// The host side that the reports of the resident world share (contact_report.hip, joint_report.hip, shape_report.hip, body_report.hip,
// step_metrics.hip, sensor_report.hip, ray_report.hip, grid_report.hip, observers.hip, episodes.hip) and the resets behind them (resets.hip): the table of the eleven in step order with its walks, the block carver, the prepare and enqueue preambles, the
// setter skeleton, the one device-to-host copy, and the getter shapes; and the host lifecycle of the lists a caller sets (sensors, fields,
// rays, grids, actuators, observers, episode rules): the argument check, the two ways a new list goes in, the per-item getter, the copy out and the
// status counts.  A report supplies its layout, its kernels, its prepare and enqueue bodies, and getters that name their list in terms
// of these ("The report facility").
#include "solver_internal.h"

namespace
{

struct ReportFacility
{
	ReportState SolverRest::*state;
	int (*prepare)(s2amdSolver*);
	int (*enqueue)(s2amdSolver*, const s2amdStepParams*);
};

// the order of a step: each report is enqueued behind the one before it.  The first ten read the world; the eleventh, the resets
// (resets.hip), is the first entry that WRITES it -- the bodies, joints, boxes and contacts of the agents whose episode the tenth found
// finished -- and therefore comes last: every report of this step has read the world the step left.
const ReportFacility facilities[] = {
	{&SolverRest::contactReport, contactReportPrepare, contactReportEnqueue},
	{&SolverRest::jointReport, jointReportPrepare, jointReportEnqueue},
	{&SolverRest::shapeReport, shapeReportPrepare, shapeReportEnqueue},
	{&SolverRest::bodyReport, bodyReportPrepare, bodyReportEnqueue},
	{&SolverRest::metrics, metricsPrepare, metricsEnqueue},
	{&SolverRest::sensorReport, sensorReportPrepare, sensorReportEnqueue},
	{&SolverRest::rayReport, rayReportPrepare, rayReportEnqueue},
	{&SolverRest::gridReport, gridReportPrepare, gridReportEnqueue},
	{&SolverRest::observationReport, observationPrepare, observationEnqueue},
	{&SolverRest::episodeReport, episodePrepare, episodeEnqueue},
	{&SolverRest::resetReport, resetPrepare, resetEnqueue},
};

int badArgument()
{
	return fail(S2AMD_E_INVALID, "bad argument");
}

} // namespace

void reportsForget(s2amdSolver* s)
{
	for (const ReportFacility& f : facilities)
	{
		(s->*f.state).stepFlags = 0;
	}
}

int reportsPrepare(s2amdSolver* s)
{
	for (const ReportFacility& f : facilities)
	{
		const int rc = f.prepare(s);
		if (rc)
		{
			return rc;
		}
	}
	return S2AMD_OK;
}

// (the reports of the attempt that stands, enqueued behind its impulse store and stage 4: a repeated step reports once; nothing waits
// for them here)
int reportsEnqueue(s2amdSolver* s, const s2amdStepParams* params)
{
	for (const ReportFacility& f : facilities)
	{
		ReportState& r = s->*f.state;
		r.stepFlags = 0;
		if (r.flags != 0)
		{
			const int rc = f.enqueue(s, params);
			if (rc)
			{
				return rc;
			}
		}
	}
	return S2AMD_OK;
}

void reportsRelease(s2amdSolver* s)
{
	for (const ReportFacility& f : facilities)
	{
		(s->*f.state).block.release();
	}
}

size_t reportRound(size_t bytes)
{
	return (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
}

size_t reportTake(size_t& at, size_t bytes)
{
	const size_t here = at;
	at += reportRound(bytes);
	return here;
}

bool reportPrepareBegin(const s2amdSolver* s, ReportState& r)
{
	r.stepFlags = 0;
	r.headKnown = false;
	return r.flags != 0 && s->worldResident;
}

int reportPrepareBlock(ReportState& r, size_t total, size_t headOffset)
{
	r.total = total, r.headOffset = headOffset;
	return r.block.ensure(total);
}

int reportEnqueueGuard(const ReportState& r, size_t total, const char* which)
{
	if (r.block.p == nullptr || r.total != total || r.block.bytes < total)
	{
		return fail(S2AMD_E_STATE, std::string("internal: the ") + which + " report's device block was not prepared");
	}
	return S2AMD_OK;
}

int reportSet(const ReportRef& f, int32_t flags, int32_t known, int (*prepare)(s2amdSolver*))
{
	if (!f.s)
	{
		return fail(S2AMD_E_INVALID, "null solver");
	}
	if ((flags & ~known) != 0)
	{
		return fail(S2AMD_E_INVALID, std::string("unknown ") + f.name + " flag bits");
	}
	const bool turnedOn = f.r->flags == 0 && flags != 0;
	f.r->flags = flags;
	// "before" starts as the world stands now; the last step's report (if any) is not of these passes
	return turnedOn ? prepare(f.s) : S2AMD_OK;
}

namespace
{

// the one device-to-host copy of the reports, enqueued on the solver's device and stream; the caller waits
int enqueueFetch(const ReportRef& f, void* out, size_t offset, int count, size_t size)
{
	if (count > 0)
	{
		HIP_TRY(hipSetDevice(f.s->device));
		HIP_TRY(hipMemcpyAsync(out, (const char*)f.r->block.p + offset, (size_t)count * size, hipMemcpyDeviceToHost, f.s->stream));
	}
	return S2AMD_OK;
}

// ... and waited for: `count` entries of `size` bytes at `offset` of the block
int fetch(const ReportRef& f, void* out, size_t offset, int count, size_t size)
{
	const int rc = enqueueFetch(f, out, offset, count, size);
	if (rc == S2AMD_OK && count > 0)
	{
		HIP_TRY(hipStreamSynchronize(f.s->stream));
	}
	return rc;
}

int getterState(const ReportRef& f, int flag, const char* what)
{
	if (!f.s->worldResident || !f.s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (flag != 0 ? (f.r->stepFlags & flag) == 0 : f.r->stepFlags == 0)
	{
		return fail(S2AMD_E_STATE, std::string(what) + ": the last s2amd_world_step did not run with this " + f.name + " flag set (" + f.setter + ", then a step)");
	}
	return S2AMD_OK;
}

} // namespace

int reportHeadFor(const ReportRef& f, int flag, const char* what)
{
	if (!f.s)
	{
		return badArgument();
	}
	int rc = getterState(f, flag, what);
	if (rc || f.r->headKnown)
	{
		return rc;
	}
	// once per step
	if ((rc = fetch(f, f.head, f.r->headOffset, 1, f.headBytes)) == 0)
	{
		f.r->headKnown = true;
	}
	return rc;
}

int reportGetList(const ReportRef& f, int flag, const char* what, const char* tooSmall, int countIndex, size_t offset, size_t size, void* out, int32_t capacity, int32_t* count)
{
	if (!f.s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return badArgument();
	}
	const int rc = reportHeadFor(f, flag, what);
	if (rc)
	{
		return rc;
	}
	*count = ((const int32_t*)f.head)[countIndex];
	if (*count > capacity)
	{
		return fail(S2AMD_E_CAPACITY, tooSmall);
	}
	return fetch(f, out, offset, *count, size);
}

int reportGetEvents(const ReportRef& f, int flag, const char* what, const char* tooSmall, int firstIndex, size_t firstOffset, size_t secondOffset, int32_t* first,
					int32_t firstCapacity, int32_t* firstCount, int32_t* second, int32_t secondCapacity, int32_t* secondCount)
{
	if (!f.s || !firstCount || !secondCount || firstCapacity < 0 || secondCapacity < 0 || (firstCapacity > 0 && !first) || (secondCapacity > 0 && !second))
	{
		return badArgument();
	}
	int rc = reportHeadFor(f, flag, what);
	if (rc)
	{
		return rc;
	}
	*firstCount = ((const int32_t*)f.head)[firstIndex];
	*secondCount = ((const int32_t*)f.head)[firstIndex + 1];
	if (*firstCount > firstCapacity || *secondCount > secondCapacity)
	{
		return fail(S2AMD_E_CAPACITY, tooSmall);
	}
	// (both copies, then one wait)
	if ((rc = enqueueFetch(f, first, firstOffset, *firstCount, sizeof(int32_t))) != 0 || (rc = enqueueFetch(f, second, secondOffset, *secondCount, sizeof(int32_t))) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(f.s->stream));
	return S2AMD_OK;
}

int reportGetPerItem(const ReportRef& f, int flag, const char* what, const char* tooSmall, const void* out, int32_t capacity, int32_t* count, int items, bool emptyFirst)
{
	if (!f.s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return badArgument();
	}
	if (emptyFirst && items == 0)
	{
		*count = 0;
		return S2AMD_OK;
	}
	const int rc = getterState(f, flag, what);
	if (rc)
	{
		return rc;
	}
	*count = items;
	if (*count > capacity)
	{
		return fail(S2AMD_E_CAPACITY, tooSmall);
	}
	return S2AMD_OK;
}

int reportGetBodyArray(const ReportRef& f, int flag, const char* what, size_t offset, size_t size, void* out, int32_t bodyCapacity)
{
	if (!f.s || bodyCapacity < 0 || (bodyCapacity > 0 && !out))
	{
		return badArgument();
	}
	const int rc = getterState(f, flag, what);
	if (rc)
	{
		return rc;
	}
	if (bodyCapacity < f.s->bodyCapacity)
	{
		return fail(S2AMD_E_CAPACITY, "body-sum array smaller than the resident body array");
	}
	return fetch(f, out, offset, f.s->bodyCapacity, size);
}

int reportCopyOut(s2amdSolver* s, void* out, const DevBuf& block, size_t offset, int count, size_t size, hipMemcpyKind kind)
{
	if (count > 0)
	{
		HIP_TRY(hipSetDevice(s->device));
		HIP_TRY(hipMemcpyAsync(out, (const char*)block.p + offset, (size_t)count * size, kind, s->stream));
		HIP_TRY(hipStreamSynchronize(s->stream));
	}
	return S2AMD_OK;
}

int listArgs(const s2amdSolver* s, const void* list, int32_t count, int32_t max)
{
	if (!s || count < 0 || count > max || (count > 0 && !list))
	{
		return badArgument();
	}
	return S2AMD_OK;
}

int listSwapIn(s2amdSolver* s, const std::function<void()>& exchange, int (*prepare)(s2amdSolver*))
{
	exchange();
	const int rc = prepare(s);
	if (rc)
	{
		// (the block or the copy failed: the list before stands, under the block it had or a larger one)
		const std::string why = s2amd_last_error();
		exchange();
		(void)prepare(s);
		return fail(rc, why);
	}
	return S2AMD_OK;
}

int listUpload(s2amdSolver* s, DevBuf& block, size_t total, const std::function<int(char*)>& enqueue)
{
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipStreamSynchronize(s->stream));
	if (int rc = block.ensure(total))
	{
		return rc;
	}
	if (int rc = enqueue((char*)block.p))
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

int listStatusCounts(s2amdSolver* s, const DevBuf& block, long passes, int32_t counts[4])
{
	HIP_TRY(hipSetDevice(s->device));
	// (the set the last pass counted into)
	const int* set = (const int*)block.p + 4 * (int)((passes - 1) & 1);
	HIP_TRY(hipMemcpyAsync(counts, set, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}
