// The body of the resident-island kernels of wide_kernel.hip -- wideIslandKernel<ROUNDS, SELF, POINTS> (s2Solve_TGS_Soft) and
// wideIslandKernelOf<KIND, ROUNDS, SELF, POINTS> (s2Solve_PGS_Soft, s2Solve_SoftStep) --, included INTO each of the two __global__ function
// templates: KIND, ROUNDS, SELF, POINTS and the kernel's parameters (c, g, ta, softCoef0, softCoef1, ops, opCount, wire, wireBodies,
// hostFlags, warmStart, sc, unpackH, stepFailed) are names of the including scope.
// Why text and not a __device__ function: tests/test_kernel_resources.py looks the TGS_Soft kernels up by their demangled names, so KIND
// cannot become a template parameter of that __global__ function, and as a function (forced inline) the body compiled differently -- the
// kernel parameters become values with an address: the two coefficient records went through a 48-byte private frame, and loaded at the
// kernel's entry instead of in the two lanes that store them they cost the eight-round TGS_Soft variants one or two spilled VGPRs.
// Included here the TGS_Soft kernels are the code they were (same registers, no scratch: make resources).
	static_assert(KIND == SOFT_TGS || KIND == SOFT_PGS || (KIND == SOFT_FIXED && ROUNDS <= S2_STRIP_ROUNDS), "wideIslandForm");
	extern __shared__ __attribute__((aligned(16))) float4 lds[];
	if (stepFailed != nullptr && *stepFailed != 0u)
	{
		return; // a persistent strip kernel of this step lost a hand-off: the step will be repeated, nothing of it may reach the wire arrays
	}
	const int tid = (int)threadIdx.x;
	const StripDesc* da = ta.descs + blockIdx.x;
	const int bodyBase = da->bodyBase, nb = da->bodyCount, roundsA = da->batchCount;
	int2 batchA[ROUNDS];
#pragma unroll
	for (int i = 0; i < ROUNDS; ++i)
	{
		batchA[i] = make_int2(da->batch[i].x, da->batch[i].y);
	}
	float4* lvel = lds;
	float4* ldq = lds + nb;
	float4* linteg = lds + 2 * nb;
	float* langDamp = (float*)(lds + 3 * nb);
	float2* lmass = (float2*)(lds + 3 * nb + (nb + 3) / 4);
	float2* llc = (float2*)(lds + 3 * nb + (nb + 3) / 4 + (nb + 1) / 2); // the bodies' local centres (soft_from_wire.h: prepareSoftFromWire)
	const int bodyRecords = 3 * nb + (nb + 3) / 4 + 2 * ((nb + 1) / 2);
	Op* lops = (Op*)(lds + bodyRecords);
	float4* lcoef = lds + bodyRecords + 2 * opCount; // 2 records (the launch adds them to the size)
	constexpr int LA = KIND == SOFT_TGS ? wideIslandLocalsInLds(ROUNDS) : 0, LL0 = ROUNDS - LA;
	float4* llocals = lcoef + 2 + tid; // [record - LL0][point][lane] {lA, lB}
	auto localsOf = [&](int r) { return llocals + 2 * (r - LL0 > 0 ? r - LL0 : 0) * S2_WIDE_THREADS; };
	// ... or, for the other kinds, the arms of the records from AL0 on (never both: wideIslandLocalRecords): [record - AL0][point][lane] {perp(rA0), perp(rB0)}
	constexpr int AA = wideIslandArmsInLds(KIND, ROUNDS), AL0 = ROUNDS - AA;
	constexpr int AK = KIND == SOFT_PGS ? S2_WIDE_PGS_ARMS : KIND; // the kind of a record whose arms are in LDS
	auto armsOf = [&](int r) { return llocals + 2 * (r - AL0 > 0 ? r - AL0 : 0) * S2_WIDE_THREADS; };

	uint32_t id[S2_STRIP_BODY_CHUNKS];
#pragma unroll
	for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
	{
		const int i = tid + ch * S2_WIDE_THREADS;
		id[ch] = i < nb ? (uint32_t)ta.bodyIds[bodyBase + i] : 0u;
	}
	for (int i = tid; i < opCount * 8; i += S2_WIDE_THREADS)
	{
		((int*)lops)[i] = ((const int*)ops)[i];
	}
	if (tid < 2)
	{
		lcoef[tid] = tid ? softCoef1 : softCoef0;
	}
	auto kOfRound = [&](int i) {
		const int k = batchA[i].x + tid;
		return (i < roundsA && k < batchA[i].y) ? k : -1;
	};
	// this thread's constraints: pool slot and group-local body slots (the wire records follow once the bodies are staged)
	int slotOf[ROUNDS];
	int2 localOf[ROUNDS];
#pragma unroll
	for (int i = 0; i < ROUNDS; ++i)
	{
		slotOf[i] = -1;
		localOf[i] = make_int2(0, 0);
		if (kOfRound(i) >= 0)
		{
			slotOf[i] = c.contactIndex[kOfRound(i)];
			localOf[i] = c.localBodies[kOfRound(i)];
		}
	}
	uint32_t flags[S2_STRIP_BODY_CHUNKS];
	float2 pos[S2_STRIP_BODY_CHUNKS]; // SELF: the positions of the bodies this lane stages (s2FinalizePositions adds to them)
#pragma unroll
	for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
	{
		const int i = tid + ch * S2_WIDE_THREADS;
		flags[ch] = 0u;
		pos[ch] = make_float2(0.0f, 0.0f);
		if (i < nb)
		{
			const int gi = (int)(id[ch] & ~S2G_OWNED);
			if constexpr (SELF)
			{
				// body_ops.h: unpackBodyOne, into LDS instead of the SoA arrays
				const s2amdBody* w = wireBodies + gi;
				const int type = w->type;
				uint32_t f = 0x80000000u;
				if (type != S2AMD_BODY_FREE)
				{
					f |= S2F_LIVE | (type == S2AMD_BODY_DYNAMIC ? S2F_DYNAMIC : 0u) | (type != S2AMD_BODY_STATIC ? S2F_MOVES : 0u);
				}
				flags[ch] = f;
				lvel[i] = make_float4(w->linearVelocity[0], w->linearVelocity[1], w->angularVelocity, 0.0f);
				ldq[i] = make_float4(w->deltaPosition[0], w->deltaPosition[1], w->rot[0], w->rot[1]);
				pos[ch] = make_float2(w->position[0], w->position[1]);
				lmass[i] = make_float2(w->invMass, w->invI);
				llc[i] = make_float2(w->localCenter[0], w->localCenter[1]);
				const V2 gravity = v2(sc.gravityX, sc.gravityY);
				const V2 force = v2(w->force[0], w->force[1]);
				const V2 inner = mulAdd(force, w->mass * w->gravityScale, gravity);
				const V2 a = mulSV(unpackH * w->invMass, inner);
				const float aw = unpackH * w->invI * w->torque;
				const float ld = 1.0f / (1.0f + unpackH * w->linearDamping);
				const float ad = 1.0f / (1.0f + unpackH * w->angularDamping);
				linteg[i] = make_float4(a.x, a.y, aw, ld);
				langDamp[i] = ad;
			}
			else
			{
				lvel[i] = g.vel[gi];
				ldq[i] = g.dq[gi];
				flags[ch] = g.flags[gi] | 0x80000000u;
				linteg[i] = g.integ[gi];
				langDamp[i] = g.angDamp[gi];
				lmass[i] = g.massInv[gi];
				llc[i] = make_float2(wireBodies[gi].localCenter[0], wireBodies[gi].localCenter[1]);
			}
		}
	}
	__syncthreads();

	LdsBodies lb{lvel, ldq};
	WideRegs rA[ROUNDS];
#pragma unroll
	for (int i = 0; i < ROUNDS; ++i)
	{
		if (slotOf[i] >= 0)
		{
			const SoftRegs<KIND> t = prepareSoftFromWire<KIND>(wire + slotOf[i], wireBodies, hostFlags, lb, lmass, localOf[i], g.capacity, warmStart, llc);
			rA[i] = wideFromSoft<KIND>(t);
			const bool st = lmass[localOf[i].x].x == 0.0f || lmass[localOf[i].y].x == 0.0f; // the doubled contact hertz of a static side
			rA[i].idx |= st ? 1u << 30 : 0u;
			if (i >= LL0)
			{
#pragma unroll
				for (int j = 0; j < 2; ++j)
				{
					localsOf(i)[j * S2_WIDE_THREADS] = make_float4(rA[i].lA[j].x, rA[i].lA[j].y, rA[i].lB[j].x, rA[i].lB[j].y);
				}
			}
			if (AA > 0 && i >= AL0)
			{
#pragma unroll
				for (int j = 0; j < 2; ++j)
				{
					armsOf(i)[j * S2_WIDE_THREADS] = wideArmsOf(t.r0[j]);
				}
			}
		}
	}
	for (int oi = 0; oi < opCount; ++oi)
	{
		const Op op = lops[oi];
		uint32_t salt;
		asm volatile("s_mov_b32 %0, 0" : "=s"(salt));
		if (op.code == OP_INTEGRATE_VEL)
		{
#pragma unroll
			for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
			{
				if ((flags[ch] & S2F_DYNAMIC) != 0)
				{
					const int i = tid + ch * S2_WIDE_THREADS;
					float4 v = lvel[i], k = linteg[i];
					V2 lv = add(v2(v.x, v.y), v2(k.x, k.y));
					float w = v.z + k.z;
					lv = mulSV(k.w, lv);
					w *= langDamp[i];
					lvel[i] = make_float4(lv.x, lv.y, w, 0.0f);
				}
			}
			__syncthreads();
		}
		else if (op.code == OP_INTEGRATE_POS)
		{
#pragma unroll
			for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
			{
				if ((flags[ch] & S2F_MOVES) != 0)
				{
					const int i = tid + ch * S2_WIDE_THREADS;
					float4 v = lvel[i], d = ldq[i];
					V2 dpos = mulAdd(v2(d.x, d.y), op.h, v2(v.x, v.y));
					Rot q;
					q.s = d.z, q.c = d.w;
					q = integrateRot(q, op.h * v.z);
					ldq[i] = make_float4(dpos.x, dpos.y, q.s, q.c);
				}
			}
			__syncthreads();
		}
		else if (op.code == OP_FINALIZE)
		{
#pragma unroll
			for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
			{
				if constexpr (SELF)
				{
					// s2FinalizePositions (solve_common.c:70-91; body_ops.h: finalizePositionsOne) on the lane's own copy of the position
					if ((flags[ch] & (op.flag ? S2F_DYNAMIC : S2F_MOVES)) != 0)
					{
						const int i = tid + ch * S2_WIDE_THREADS;
						const float4 d = ldq[i];
						const V2 np = add(v2(pos[ch].x, pos[ch].y), v2(d.x, d.y));
						pos[ch] = make_float2(np.x, np.y);
						ldq[i] = make_float4(0.0f, 0.0f, d.z, d.w);
					}
				}
				else if (flags[ch] != 0u)
				{
					finalizePositionsOne(lb, tid + ch * S2_WIDE_THREADS, g, (int)(id[ch] & ~S2G_OWNED), op.flag, (id[ch] & S2G_OWNED) != 0);
				}
			}
			__syncthreads();
		}
		else if (op.code == OP_WARM)
		{
#pragma unroll
			for (int i = 0; i < ROUNDS; ++i)
			{
				if (i < roundsA)
				{
					if (kOfRound(i) >= 0)
					{
						if (i >= LL0)
						{
							warmWide<KIND, POINTS, true>(rA[i], lvel, ldq, lmass, salt, nullptr, localsOf(i));
						}
						else if (AA > 0 && i >= AL0)
						{
							warmWide<AK, POINTS>(rA[i], lvel, ldq, lmass, salt, armsOf(i));
						}
						else
						{
							warmWide<KIND, POINTS>(rA[i], lvel, ldq, lmass, salt);
						}
					}
					__syncthreads();
				}
			}
		}
		else if (op.code == OP_SOLVE_SOFT)
		{
#pragma unroll
			for (int i = 0; i < ROUNDS; ++i)
			{
				if (i < roundsA)
				{
					if (kOfRound(i) >= 0)
					{
						const WidePrep pre = (i >= LL0)				? prepWide<KIND, POINTS, true>(rA[i], ldq, lcoef, op.inv_h, op.useBias, salt, nullptr, localsOf(i))
											 : (AA > 0 && i >= AL0) ? prepWide<AK, POINTS>(rA[i], ldq, lcoef, op.inv_h, op.useBias, salt, armsOf(i))
																	: prepWide<KIND, POINTS>(rA[i], ldq, lcoef, op.inv_h, op.useBias, salt);
						chainWide<POINTS>(rA[i], pre, lvel, lmass, lcoef, salt);
					}
					__syncthreads();
				}
			}
		}
	}
#pragma unroll
	for (int ch = 0; ch < S2_STRIP_BODY_CHUNKS; ++ch)
	{
		const int i = tid + ch * S2_WIDE_THREADS;
		if (i < nb && (id[ch] & S2G_OWNED) != 0)
		{
			const int gi = (int)(id[ch] & ~S2G_OWNED);
			if constexpr (SELF)
			{
				if ((flags[ch] & S2F_LIVE) != 0) // body_ops.h: packBodyOne
				{
					s2amdBody* w = wireBodies + gi;
					const float4 v = lvel[i], d = ldq[i];
					w->position[0] = pos[ch].x, w->position[1] = pos[ch].y;
					w->rot[0] = d.z, w->rot[1] = d.w;
					w->linearVelocity[0] = v.x, w->linearVelocity[1] = v.y;
					w->angularVelocity = v.z;
					w->deltaPosition[0] = d.x, w->deltaPosition[1] = d.y;
				}
			}
			else
			{
				g.vel[gi] = lvel[i];
				g.dq[gi] = ldq[i];
			}
		}
	}
	// s2StoreContactImpulses (solve_common.c:396-410): straight into the manifolds
#pragma unroll
	for (int i = 0; i < ROUNDS; ++i)
	{
		if (slotOf[i] >= 0)
		{
			const int pointCount = (int)((rA[i].idx >> 26) & 3u);
			s2amdContact* contact = wire + slotOf[i];
#pragma unroll
			for (int j = 0; j < 2; ++j)
			{
				if (j < pointCount)
				{
					contact->points[j].normalImpulse = rA[i].imp[j].x;
					contact->points[j].tangentImpulse = rA[i].imp[j].y;
				}
			}
		}
	}
