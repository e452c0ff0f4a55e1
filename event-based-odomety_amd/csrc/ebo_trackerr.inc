// ebo_trackerr.inc — track evaluation on the device: the error of estimated feature tracks against ground-truth
// tracks interpolated in time, and the age each one reaches before that error first exceeds a threshold, one wave per
// (track, threshold) unit, the whole batch in one launch.  The protocol is the one published for event-based trackers
// on real recordings (Gehrig et al., "EKLT: Asynchronous Photometric Feature Tracking using Events and Frames"); the
// reference has no counterpart in code, its report states the two figures (mean track error, feature age).  Included
// inside ebo_kernels.hip's anonymous namespace, after ebo_relpose.inc, whose RP_FN / rp_reduce / rp_finite it uses:
// the tree of its sums is R6's.  The rules are written out in include/ebo.h ("track evaluation", V1-V9);
// tests/trackerr_ref.py restates them in numpy.  Float64, one rounding per operation in the association written here:
// the library is compiled with -ffp-contract=off, so the plain operators below are the rules' operations.
//
// Only the bodies handed to rp_reduce / te_firsts / te_reduce depend on the lane: lane l takes the track's samples
// (V1, V2-V5) or the unit's inliers (V7) l, l + 64, ..  Everything else is scalar state that every lane carries alike:
// no LDS, no barrier, no atomics; the search of V3 has the same trip count for every sample of a track.  A host build
// (EBO_RELPOSE_RULES_ONLY, tools/track_errors_serial.cpp) runs the lanes of a reduction one after the other.

// one unit: a track's samples on both sides and the threshold
struct TeView
{
	int nEst;             // estimated samples of the track
	int nGt;              // ground-truth samples of the track
	const int64_t* estT;  // [nEst], non-decreasing
	const double* estXy;  // [nEst][2]
	const int64_t* gtT;   // [nGt], strictly increasing
	const double* gtXy;   // [nGt][2]
	double tau;
	double* sampleErr;    // [nEst] or null: V8, handed to the track's first unit alone
};

// V2, V5: three indices at once, each the smallest of what the lanes found
constexpr int kTeFirsts = 3;
#ifdef EBO_RELPOSE_RULES_ONLY
template <class F>
inline void te_firsts(F&& body, int (&out)[kTeFirsts])
{
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		int part[kTeFirsts];
		body(lane, part);
		for (int k = 0; k < kTeFirsts; ++k)
		{
			out[k] = (lane == 0 || part[k] < out[k]) ? part[k] : out[k];
		}
	}
}
#else
template <class F>
__device__ __forceinline__ void te_firsts(F&& body, int (&out)[kTeFirsts])
{
	int acc[kTeFirsts];
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1), acc);
#pragma unroll
	for (int k = 0; k < kTeFirsts; ++k)
	{
		int v = acc[k];
#pragma unroll
		for (int s = kRpLanes / 2; s > 0; s /= 2)
		{
			const int o = __shfl_xor(v, s, kRpLanes);
			v = o < v ? o : v;
		}
		out[k] = __builtin_amdgcn_readfirstlane(v);
	}
}
#endif

// V7's three results at once: slots 0 and 1 are sums in R6's tree (e, q), slot 2 a maximum over the same tree
// (partial[i] takes partial[i + s] when that is strictly larger)
constexpr int kTeSlots = 3;
RP_FN void te_merge(double (&a)[kTeSlots], const double (&b)[kTeSlots])
{
	a[0] = a[0] + b[0];
	a[1] = a[1] + b[1];
	a[2] = b[2] > a[2] ? b[2] : a[2];
}
#ifdef EBO_RELPOSE_RULES_ONLY
template <class F>
inline void te_reduce(F&& body, double (&out)[kTeSlots])
{
	double part[kRpLanes][kTeSlots];
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		body(lane, part[lane]);
	}
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		for (int i = 0; i < s; ++i)
		{
			te_merge(part[i], part[i + s]);
		}
	}
	for (int k = 0; k < kTeSlots; ++k)
	{
		out[k] = part[0][k];
	}
}
#else
template <class F>
__device__ __forceinline__ void te_reduce(F&& body, double (&out)[kTeSlots])
{
	double acc[kTeSlots];
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1), acc);
#pragma unroll
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		double other[kTeSlots];
#pragma unroll
		for (int k = 0; k < kTeSlots; ++k)
		{
			other[k] = __shfl_down(acc[k], s, kRpLanes);  // lanes >= s merge what no later step reads
		}
		te_merge(acc, other);
	}
#pragma unroll
	for (int k = 0; k < kTeSlots; ++k)
	{
		out[k] = __shfl(acc[k], 0, kRpLanes);
	}
}
#endif

// V3, V4 for estimated sample i, which lies within the ground truth's span: q and e
RP_FN void te_error(const TeView& v, int steps, int i, double& q, double& e)
{
	const int64_t t = v.estT[i];
	const int j = te_search(v.gtT, v.nGt, steps, t);
	double gx, gy;
	te_interp(v.gtT, v.gtXy, v.nGt, j, t, gx, gy);
	const double dx = v.estXy[2 * static_cast<size_t>(i)] - gx;
	const double dy = v.estXy[2 * static_cast<size_t>(i) + 1] - gy;
	q = dx * dx + dy * dy;
	e = sqrt(q);
}

// what a unit without statistics returns (V1): zeros under its status
RP_FN void te_zero(ebo_track_error_result* out, int status)
{
	if (RP_FIRST_LANE())
	{
		out->err_mean = out->err_rmse = out->err_max = 0.0;
		out->age_us = out->t_first_us = 0;
		out->n_inliers = out->n_comparable = out->first = out->cut = 0;
		out->status = status;
		out->pad = 0;
	}
}

// the same before any sample was looked at: none of them has an error (V8)
RP_FN void te_none(const TeView& v, ebo_track_error_result* out, int status)
{
	if (v.sampleErr)
	{
		rp_for_lanes([&](int lane) RP_BODY {
			for (int i = lane; i < v.nEst; i += kRpLanes)
			{
				v.sampleErr[i] = -1.0;
			}
		});
	}
	te_zero(out, status);
}

RP_FN void te_unit(const TeView& v, ebo_track_error_result* out)
{
	// V1: nothing to compare; then one pass over both sides for the count of samples with a non-finite coordinate
	if (v.nEst <= 0 || v.nGt < 2)
	{
		te_none(v, out, 1);
		return;
	}
	double bad[1];
	rp_reduce<1>(
		[&](int lane, double(&acc)[1]) RP_BODY {
			acc[0] = 0.0;
			for (int i = lane; i < v.nEst; i += kRpLanes)
			{
				const bool ok = rp_finite(v.estXy[2 * static_cast<size_t>(i)]) && rp_finite(v.estXy[2 * static_cast<size_t>(i) + 1]);
				acc[0] = acc[0] + (ok ? 0.0 : 1.0);
			}
			for (int i = lane; i < v.nGt; i += kRpLanes)
			{
				const bool ok = rp_finite(v.gtXy[2 * static_cast<size_t>(i)]) && rp_finite(v.gtXy[2 * static_cast<size_t>(i) + 1]);
				acc[0] = acc[0] + (ok ? 0.0 : 1.0);
			}
		},
		bad);
	if (RP_UNIFORM(static_cast<int>(bad[0] != 0.0)))
	{
		te_none(v, out, 2);
		return;
	}
	// V2-V5, V8: one pass over the estimated samples for the first comparable one (i0), the first past the span (i1)
	// and the first comparable one beyond tau (c)
	const int steps = te_steps(v.nGt);
	const int64_t t0 = v.gtT[0], t1 = v.gtT[v.nGt - 1];
	const double tau = v.tau;
	int firsts[kTeFirsts];
	te_firsts(
		[&](int lane, int(&acc)[kTeFirsts]) RP_BODY {
			acc[0] = acc[1] = acc[2] = v.nEst;
			for (int i = lane; i < v.nEst; i += kRpLanes)
			{
				const int64_t t = v.estT[i];
				double err = -1.0;
				if (t >= t0 && t <= t1)
				{
					double q;
					te_error(v, steps, i, q, err);
					acc[0] = i < acc[0] ? i : acc[0];
					if (err > tau)
					{
						acc[2] = i < acc[2] ? i : acc[2];
					}
				}
				else if (t > t1)
				{
					acc[1] = i < acc[1] ? i : acc[1];
				}
				if (v.sampleErr)
				{
					v.sampleErr[i] = err;
				}
			}
		},
		firsts);
	const int i0 = firsts[0], i1 = firsts[1];
	if (i0 >= i1)
	{
		// V1: no estimated sample within the span (the pass above has written -1 everywhere)
		te_zero(out, 1);
		return;
	}
	const bool isCut = firsts[2] < i1;
	const int end = isCut ? firsts[2] : i1;  // one past the last inlier
	const int inliers = end - i0;
	// V7: the inliers again, inlier k in lane k mod 64
	double st[kTeSlots] = {0.0, 0.0, 0.0};
	if (inliers > 0)
	{
		te_reduce(
			[&](int lane, double(&acc)[kTeSlots]) RP_BODY {
				acc[0] = acc[1] = acc[2] = 0.0;
				for (int i = i0 + lane; i < end; i += kRpLanes)
				{
					double q, e;
					te_error(v, steps, i, q, e);
					acc[0] = acc[0] + e;
					acc[1] = acc[1] + q;
					acc[2] = e > acc[2] ? e : acc[2];
				}
			},
			st);
	}
	if (RP_FIRST_LANE())
	{
		const double nd = static_cast<double>(inliers);
		out->err_mean = inliers > 0 ? st[0] / nd : 0.0;
		out->err_rmse = inliers > 0 ? sqrt(st[1] / nd) : 0.0;
		out->err_max = st[2];
		out->age_us = inliers > 0 ? v.estT[end - 1] - v.estT[i0] : 0;
		out->t_first_us = v.estT[i0];
		out->n_inliers = inliers;
		out->n_comparable = i1 - i0;
		out->first = i0;
		out->cut = isCut ? firsts[2] : -1;
		out->status = 0;
		out->pad = 0;
	}
}

#ifndef EBO_RELPOSE_RULES_ONLY
// one wave per unit.  Unit u = k * nTaus + j is track k, samples estOff[k] .. estOff[k + 1] - 1 of the estimate and
// gtOff[k] .. gtOff[k + 1] - 1 of the ground truth, at threshold taus[j]; sampleErr may be null
__global__ void __launch_bounds__(kRpLanes) k_track_errors(int nEst, int nGt, const int* __restrict__ estOff, const int64_t* __restrict__ estT,
														   const double* __restrict__ estXy, const int* __restrict__ gtOff,
														   const int64_t* __restrict__ gtT, const double* __restrict__ gtXy, int nTaus,
														   const double* __restrict__ taus, ebo_track_error_result* __restrict__ results,
														   double* __restrict__ sampleErr)
{
	const int u = static_cast<int>(blockIdx.x);
	const int k = u / nTaus, j = u - k * nTaus;
	// the entry has refused such offsets; never past the arrays
	int eb = estOff[k], ee = estOff[k + 1], gb = gtOff[k], ge = gtOff[k + 1];
	eb = eb < 0 ? 0 : (eb > nEst ? nEst : eb);
	ee = ee < eb ? eb : (ee > nEst ? nEst : ee);
	gb = gb < 0 ? 0 : (gb > nGt ? nGt : gb);
	ge = ge < gb ? gb : (ge > nGt ? nGt : ge);
	TeView v;
	v.nEst = ee - eb;
	v.nGt = ge - gb;
	v.estT = estT + eb;
	v.estXy = estXy + 2 * static_cast<size_t>(eb);
	v.gtT = gtT + gb;
	v.gtXy = gtXy + 2 * static_cast<size_t>(gb);
	v.tau = taus[j];
	v.sampleErr = (sampleErr && j == 0) ? sampleErr + eb : nullptr;
	te_unit(v, results + u);
}
#endif
