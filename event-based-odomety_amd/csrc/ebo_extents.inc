// ebo_extents.inc — the per-unit time-extent table behind k_eval3's bounding box (box_extents.h), included inside
// ebo_kernels.hip's anonymous namespace.
//
// k_unit_extents: one workgroup per unit.  The smallest and the largest dt of every source column and row of the
// unit's rect, by LDS integer min / max, then the slot in one coalesced write.  Launched on the context's stream by
// every load, behind the units and the events it reads (ebo_windows.cpp: upload_launch_order); flows never enter.
__global__ void __launch_bounds__(256) k_unit_extents(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
													  int32_t* __restrict__ table)
{
	__shared__ int32_t slot[kExtStride];
	const Unit u = units[blockIdx.x];
	const int rw = u.rw, rh = u.rh;
	for (int i = threadIdx.x; i < kExtStride; i += blockDim.x)
	{
		slot[i] = i < kExtEntries ? 0 : ((i & 1) ? kExtEmptyMax : kExtEmptyMin);  // (kExtEntries is even: min, max, min, ...)
	}
	__syncthreads();
	const bool tabled = !(u.flags & kUnitStray) && rw >= 1 && rh >= 1 && rw <= kExtMaxSide && rh <= kExtMaxSide;
	int outside = 0;
	if (tabled)
	{
		const uint64_t* ev = events + u.ev_off;
		int32_t* e = slot + kExtEntries;
		for (uint32_t k = threadIdx.x; k < u.n_ev; k += blockDim.x)
		{
			int x, y, pos, dt;
			unpack(ev[k], x, y, pos, dt);
			const int cx = x - u.rx, cy = y - u.ry;
			if (cx < 0 || cx >= rw || cy < 0 || cy >= rh)
			{
				outside = 1;
				continue;
			}
			atomicMin(&e[2 * cx], dt);
			atomicMax(&e[2 * cx + 1], dt);
			atomicMin(&e[2 * (rw + cy)], dt);
			atomicMax(&e[2 * (rw + cy) + 1], dt);
		}
	}
	outside = __syncthreads_or(outside);
	if (threadIdx.x == 0)
	{
		slot[0] = (tabled && !outside) ? kExtValid : kExtNone;
	}
	__syncthreads();
	int32_t* out = table + static_cast<size_t>(blockIdx.x) * kExtStride;
	for (int i = threadIdx.x; i < kExtStride; i += blockDim.x)
	{
		out[i] = slot[i];
	}
}

// The box of a unit from its slot (box_extents.h), by every wave for itself and without LDS: lane i < rw takes column i,
// the next rh lanes the rows (a second step where rw + rh > 64).  True: the box is the event pass's, in every lane.
// The decision depends on the slot and the flow alone: the same in every wave, workgroup and row tile of the unit.
// Nothing branches on the status before the entries are asked for: status and entries come in one memory latency, as
// the event pass's records do (in a slot without a table the pairs are empty and the status refuses whatever they give).
__device__ __forceinline__ bool box_from_extents(const int32_t* __restrict__ slot, int rx, int ry, int rw, int rh, double m0,
												 double m1, const EvalConsts& c, int& xmin, int& xmax, int& ymin, int& ymax)
{
	const int lane = threadIdx.x & 63;
	const int2* ent = reinterpret_cast<const int2*>(slot + kExtEntries);
	const int32_t status = slot[0];  // (looked at last)
	int xlo = kExtEmptyMin, xhi = kExtEmptyMax, ylo = kExtEmptyMin, yhi = kExtEmptyMax;
	bool ok = true;
	for (int i = lane; i < rw + rh; i += 64)
	{
		const int2 t = ent[i & (2 * kExtMaxSide - 1)];  // (inside the slot whatever the rect of a unit without a table)
		if (i < rw)
		{
			box_entry(rx + i, t.x, t.y, c.scale, m0, rx, rw, xlo, xhi, ok);
		}
		else
		{
			box_entry(ry + (i - rw), t.x, t.y, c.scale, m1, ry, rh, ylo, yhi, ok);
		}
	}
	xlo = __builtin_amdgcn_readlane(wave_min(xlo), kWaveResultLane);
	xhi = __builtin_amdgcn_readlane(wave_max(xhi), kWaveResultLane);
	ylo = __builtin_amdgcn_readlane(wave_min(ylo), kWaveResultLane);
	yhi = __builtin_amdgcn_readlane(wave_max(yhi), kWaveResultLane);
	const int all = __builtin_amdgcn_readlane(wave_min(ok ? 1 : 0), kWaveResultLane);
	if (status != kExtValid || !box_admits(all != 0, xlo, xhi, ylo, yhi, rw, rh))
	{
		return false;
	}
	xmin = xlo;
	xmax = xhi;
	ymin = ylo;
	ymax = yhi;
	return true;
}
