// ebo_kernels.hip — hand-written HIP kernels for gfx950 (MI355X, CDNA4).
//
// Hot path of nurlanov-zh/event-based-odomety's motion compensation:
//   warp each event by its patch's candidate flow over its dt      (contrast_functor.h:47-54)
//   7x7 Gaussian splat into the 3W x 3H image of warped events     (contrast_functor.h:56-86)
//   variance objective + forward-mode Jacobian                     (contrast_functor.h:101-150)
//   per-patch Levenberg-Marquardt on the device                    (feature_detector.cpp:401-414, TV = 0)
//   integer event-count images                                     (feature_detector.cpp:433-482, :270-295; patch.cpp:65-130)
//
// Design (DESIGN.md has the numbers):
//   * events are 8-byte packed records, bucketed by patch, streamed from HBM in
//     coalesced 512-B wave reads; one lane owns one event.
//   * the image of warped events lives only in LDS (planar f64 channels: value,
//     d/dm0, d/dm1); taps are scatter-added with native ds_add_f64; nothing but
//     7 partial sums per workgroup ever goes back to HBM.
//   * reductions: wave64 shuffles, then one LDS hop across waves, fixed order.
//   * no MFMA: this is scatter + reduce, not a contraction.
// Built with -ffp-contract=off: the warped coordinate must round exactly like
// the CPU path (one rounding per operation) because it is truncated to a bin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <cstdlib>

#include "box_extents.h"
#include "ebo_internal.h"
#include "eval_deal.h"
#include "eval_interior.h"
#include "eval_plan.h"
#include "exp_taps.h"
#include "tap_moments.h"

namespace ebo
{
namespace
{
__device__ __forceinline__ void unpack(uint64_t rec, int& x, int& y, int& pos, int& dt)
{
	const uint32_t lo = static_cast<uint32_t>(rec);
	dt = static_cast<int>(static_cast<uint32_t>(rec >> 32));
	x = static_cast<int>(lo << 17) >> 17;
	y = static_cast<int>(lo << 1) >> 17;
	pos = (lo >> 15) & 1u;
}

// Phase clocks of the edge and variance kernels (build with -DEBO_EDGE_TIMING,
// tools/edge_phase_clock.py, tools/eval_phase_clock.py): every wave keeps the shader-clock cycles
// between two barrier-separated points in scalar accumulators; thread 0 of the workgroup adds
// them to a device table when the unit is done (64 rows by workgroup index: same-address atomics
// from every workgroup at every phase would dominate what is being measured).  Never compiled
// into the shipped library.
#ifdef EBO_EDGE_TIMING
__device__ unsigned long long g_edge_clk[64 * 32];
#define EDGE_TICK_DECL                       \
	unsigned long long edgeClk_ = clock64(); \
	unsigned long long edgeAcc_[24] = {0}
#define EDGE_TICK(k)                                  \
	do                                                \
	{                                                 \
		const unsigned long long now_ = clock64();    \
		edgeAcc_[k] += now_ - edgeClk_;               \
		edgeClk_ = now_;                              \
	} while (0)
#define EDGE_COUNT(k, v) edgeAcc_[k] += static_cast<unsigned long long>(v)
#define EDGE_TICK_FLUSH                                                                       \
	do                                                                                        \
	{                                                                                         \
		if (threadIdx.x == 0)                                                                 \
		{                                                                                     \
			for (int k_ = 0; k_ < 24; ++k_)                                                   \
			{                                                                                 \
				if (edgeAcc_[k_])                                                             \
				{                                                                             \
					atomicAdd(&g_edge_clk[(blockIdx.x & 63) * 32 + k_], edgeAcc_[k_]);        \
				}                                                                             \
			}                                                                                 \
		}                                                                                     \
	} while (0)
#define EDGE_TICK_ARG , unsigned long long &edgeClk_, unsigned long long(&edgeAcc_)[24]
#define EDGE_TICK_PASS , edgeClk_, edgeAcc_
#else
#define EDGE_TICK(k) do { } while (0)
#define EDGE_TICK_DECL do { } while (0)
#define EDGE_COUNT(k, v) do { } while (0)
#define EDGE_TICK_FLUSH do { } while (0)
#define EDGE_TICK_ARG
#define EDGE_TICK_PASS
#endif

__device__ __forceinline__ bool convertible(double c)
{
	return fabs(c) < 1073741824.0;  // int(double) is defined; same guard as the CPU path
}

// Wave-wide reductions on the DPP path (no LDS round trip: __shfl_down is a ds_bpermute, ~100
// cycles of latency per step on the queue the LDS atomics use).  The source lanes of one step:
// quad neighbours, the other pair of the quad, 4 and 8 lanes down the row of 16, then lane 15 of
// the previous row into rows 1 and 3 and lane 31 into rows 2 and 3.  A lane with no source gets
// `idle` (the operation's identity).  The wave's result is in LANE 63 (kWaveResultLane).
// Whole waves only: every launch site of a kernel that reduces uses a workgroup size that is a
// multiple of 64 (the environment overrides are validated), so lane 63 of every wave exists.
constexpr int kWaveResultLane = 63;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_take(int v, int idle)
{
	return __builtin_amdgcn_update_dpp(idle, v, CTRL, ROW_MASK, 0xf, false);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_take(double v, double idle)
{
	const int lo = dpp_take<CTRL, ROW_MASK>(__double2loint(v), __double2loint(idle));
	const int hi = dpp_take<CTRL, ROW_MASK>(__double2hiint(v), __double2hiint(idle));
	return __hiloint2double(hi, lo);
}

// v <- op(v, source lane's v) over the six steps; Op(a, b) must be commutative and associative
// up to what the caller tolerates (sums: a fixed order, so results are reproducible run to run).
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, T idle, Op op)
{
	v = op(v, dpp_take<0xb1, 0xf>(v, idle));   // quad_perm [1,0,3,2]
	v = op(v, dpp_take<0x4e, 0xf>(v, idle));   // quad_perm [2,3,0,1]
	v = op(v, dpp_take<0x114, 0xf>(v, idle));  // row_shr 4
	v = op(v, dpp_take<0x118, 0xf>(v, idle));  // row_shr 8
	v = op(v, dpp_take<0x142, 0xa>(v, idle));  // row_bcast 15 into rows 1, 3
	v = op(v, dpp_take<0x143, 0xc>(v, idle));  // row_bcast 31 into rows 2, 3
	return v;
}

// The fixed-point form of a tap is the double (value + bias) with the bias's high dword taken off its high dword: ONE
// 32-bit subtract, the low dword goes as it is.  Left alone, the compiler re-forms the 64-bit difference (the double as
// an integer minus biasHi << 32) and spends v_subrev_co_u32 (low dword minus 0, for a carry that is always 0) + s_nop +
// v_subb_co_u32 per tap -- 49 times per event in the scatter, 64 times per entry in the edge loss's reverse pass.  An
// empty asm on the high dword keeps the halves apart.
__device__ __forceinline__ void keep32(unsigned int& v)
{
#ifndef EBO_FIX_UNPINNED
	asm volatile("" : "+v"(v));
#endif
}

// One 8-byte LDS read that stays ONE ds_read_b64.  The compiler pairs neighbouring 8-byte reads of one base into
// ds_read2_b64, which the LDS serves as two accesses in four groups of 16 lanes (128 B/clk/CU, banks mod 32) where a
// ds_read_b64 goes in two groups of 32 lanes (256 B/clk/CU, banks mod 64): with per-lane random bases -- every lane
// reads at its own event's footprint -- the paired form is the slower one.  A relaxed wavefront-scope atomic load is
// the same instruction, and the load / store optimiser leaves ordered accesses alone.
__device__ __forceinline__ double lds_ld(const double* p)
{
#ifdef EBO_LDS_PAIRED_READS
	return *p;
#else
	return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
														__HIP_MEMORY_SCOPE_WAVEFRONT));
#endif
}

__device__ __forceinline__ double wave_sum(double v)  // total in lane kWaveResultLane
{
	return wave_reduce(v, 0.0, [](double a, double b) { return a + b; });
}

__device__ __forceinline__ int wave_min(int v)
{
	return wave_reduce(v, 0x7fffffff, [](int a, int b) { return min(a, b); });
}

__device__ __forceinline__ int wave_max(int v)
{
	return wave_reduce(v, static_cast<int>(0x80000000u), [](int a, int b) { return max(a, b); });
}

// Sums NV per-thread values over the workgroup; every thread gets the totals.
// Order is fixed (lanes by the DPP tree of wave_reduce, then waves 0..nw-1) => deterministic.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red)
{
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
	for (int k = 0; k < NV; ++k)
	{
		v[k] = wave_sum(v[k]);
	}
	__syncthreads();  // red may still be read by a previous call
	if (lane == kWaveResultLane)
	{
#pragma unroll
		for (int k = 0; k < NV; ++k)
		{
			red[wave * 8 + k] = v[k];
		}
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < NV; ++k)
	{
		double s = red[k];
		for (int w = 1; w < nw; ++w)
		{
			s += red[w * 8 + k];
		}
		v[k] = s;
	}
}

// Up to 16 values per thread in ONE pass (two barriers) for workgroups of at most eight waves: the same wave
// reduction and the same order over the waves per value as block_sum, so a value has the bits block_sum gives it.
template <int NV>
__device__ __forceinline__ void block_sum_wide(double (&v)[NV], double* red)
{
	static_assert(NV <= 16, "block_sum_wide: at most 16 values");
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	const int nw = (blockDim.x + 63) >> 6;  // <= 8: red holds 128 doubles
#pragma unroll
	for (int k = 0; k < NV; ++k)
	{
		v[k] = wave_sum(v[k]);
	}
	__syncthreads();  // red may still be read by a previous call
	if (lane == kWaveResultLane)
	{
#pragma unroll
		for (int k = 0; k < NV; ++k)
		{
			red[wave * 16 + k] = v[k];
		}
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < NV; ++k)
	{
		double s = red[k];
		for (int w = 1; w < nw; ++w)
		{
			s += red[w * 16 + k];
		}
		v[k] = s;
	}
}

// ---------------------------------------------------------------------------
// Warp + 7x7 Gaussian splat of one unit's events into rows [r0, r0+rows) of its
// 3W x 3H image (contrast_functor.h:38-88).  C = 1: value only (the T=double
// instantiation); C = 3: value, d/dm0, d/dm1 (the Jet<double,2> instantiation).
//   c = p + (t_ref - t) * scale * m;  b = int(c)  (truncation)
//   tap (i,j): w = N * exp(hs * ((b.x+i-c.x)^2 + (b.y+j-c.y)^2))
//   dw/dm0 = w * (b.x+i-c.x) * tau / sigma^2,   dw/dm1 likewise in y
// The Gaussian is evaluated as a product of two 1-D factors (7+7 exps instead
// of 49): same real number, last-bit differences only.
// ---------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void splat_rows(const uint64_t* __restrict__ ev, uint32_t nEv,
											int rx, int ry, int rw, int rh, int r0, int rows,
											double m0, double m1, const EvalConsts& c,
											double* __restrict__ img, int plane)
{
	const int W3 = 3 * rw;
	for (uint32_t e = threadIdx.x; e < nEv; e += blockDim.x)
	{
		int x, y, pos, dt;
		unpack(ev[e], x, y, pos, dt);
		const double tau = static_cast<double>(dt) * c.scale;
		const double cx = static_cast<double>(x) + tau * m0;
		const double cy = static_cast<double>(y) + tau * m1;
		if (!convertible(cx) || !convertible(cy))
		{
			continue;
		}
		const int bx = static_cast<int>(cx);
		const int by = static_cast<int>(cy);
		const int pxc = bx - rx + rw;       // column of tap i = 0
		const int pyc = by - ry + rh - r0;  // tile-local row of tap j = 0
		if (pxc + 3 < 0 || pxc - 3 >= W3 || pyc + 3 < 0 || pyc - 3 >= rows)
		{
			continue;
		}
		const double fx = cx - static_cast<double>(bx);  // exact
		const double fy = cy - static_cast<double>(by);
		const double g = tau * c.inv_sigsq;

		double wx[7], wy[7], ax[7], ay[7];
#pragma unroll
		for (int k = 0; k < 7; ++k)
		{
			const double dx = static_cast<double>(k - 3) - fx;  // == (b.x+i) - c.x
			const double dy = static_cast<double>(k - 3) - fy;
			wx[k] = c.norm * exp(c.hs * (dx * dx));
			wy[k] = exp(c.hs * (dy * dy));
			if (C == 3)
			{
				ax[k] = wx[k] * (g * dx);
				ay[k] = wy[k] * (g * dy);
			}
		}
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
			const int row = pyc + j - 3;
			if (row < 0 || row >= rows)
			{
				continue;
			}
			double* rowp = img + row * W3 + (pxc - 3);
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				const int col = pxc + i - 3;
				if (col < 0 || col >= W3)
				{
					continue;
				}
				atomicAdd(rowp + i, wx[i] * wy[j]);
				if (C == 3)
				{
					atomicAdd(rowp + plane + i, ax[i] * wy[j]);
					atomicAdd(rowp + 2 * plane + i, wx[i] * ay[j]);
				}
			}
		}
	}
}

// contrast_functor.h:122-149 from the sums S1 = sum I, S2 = sum I^2, n, D1k = sum dIk,
// D2k = sum I dIk over the pixels with I > 0 (contrast_functor.h:111-121, :129-139).
// counterNonZero starts at 1 (:110).
//   mean = S1/cnt;  var = sum_{I>0}(I-mean)^2 / cnt = (S2 - 2 mean S1 + n mean^2)/cnt
//   r = maxRes - var, or the out-of-window penalty maxRes (1 + m0^2 + m1^2) if mean <= 0.
__device__ __forceinline__ void variance_from_sums(const double* S, bool wantJac, double m0,
													double m1, double maxRes, double& r,
													double& j0, double& j1)
{
	const double n = S[2];
	const double cntInv = 1.0 / (n + 1.0);
	const double mean = S[0] * cntInv;
	if (mean > 0.0)
	{
		const double var = (S[1] - 2.0 * mean * S[0] + n * mean * mean) * cntInv;
		r = maxRes - var;
		if (wantJac)
		{
			const double dm0 = S[3] * cntInv;
			const double dm1 = S[4] * cntInv;
			j0 = -(2.0 * (S[5] - mean * S[3] - dm0 * S[0] + n * mean * dm0) * cntInv);
			j1 = -(2.0 * (S[6] - mean * S[4] - dm1 * S[0] + n * mean * dm1) * cntInv);
		}
	}
	else
	{
		r = maxRes * (1.0 + m0 * m0 + m1 * m1);
		j0 = maxRes * (m0 + m0);
		j1 = maxRes * (m1 + m1);
	}
}

__device__ __forceinline__ void fd_offset(int set, double h, double& m0, double& m1)
{
	if (set == 1) m0 += h;
	if (set == 2) m0 -= h;
	if (set == 3) m1 += h;
	if (set == 4) m1 -= h;
}

// ===========================================================================
// Shared by the variance evaluation (ebo_eval3.inc) and the edge loss
// (ebo_edge.inc): the LDS header, the warp of one event onto its unit's canvas,
// the seven taps of one axis and the workgroup's bounding box.
// ===========================================================================
constexpr int kRedDoubles = 128;  // 16 waves x 8
constexpr int kLdsHeader = 160;   // red[128] + 32 doubles of int scratch
// (k_eval3's header follows its workgroup's waves, eval_plan.h; this is the one of 16 waves, which k_solve_independent,
// the dump kernel and the edge loss keep)
static_assert(kRedDoubles == ebo::eval_sum_doubles(ebo::kEvalHeaderWavesMax) && kLdsHeader == ebo::eval_header_doubles(ebo::kEvalHeaderWavesMax),
			  "eval_unit3's header of 16 waves is the shared one");

// ACCEPTED: the caller knows that neither test rejects the event (eval_interior.h: every event of an all-interior
// unit); the tests are then not compiled, the other statements are the same.
template <bool ACCEPTED = false>
__device__ __forceinline__ bool warp_event(uint64_t rec, int rx, int ry, int rw, int rh,
											double m0, double m1, const EvalConsts& c, int& pxc,
											int& pyc, double& fx, double& fy, double& tau)
{
	int x, y, pos, dt;
	unpack(rec, x, y, pos, dt);
	tau = static_cast<double>(dt) * c.scale;
	const double cx = static_cast<double>(x) + tau * m0;  // not fused: -ffp-contract=off
	const double cy = static_cast<double>(y) + tau * m1;
	if (!ACCEPTED && (!convertible(cx) || !convertible(cy)))
	{
		return false;
	}
	const int bx = static_cast<int>(cx);  // truncation (contrast_functor.h:59,63)
	const int by = static_cast<int>(cy);
	pxc = bx - rx + rw;  // canvas column / row of the centre tap
	pyc = by - ry + rh;
	if (!ACCEPTED && (pxc + 3 < 0 || pxc - 3 >= 3 * rw || pyc + 3 < 0 || pyc - 3 >= 3 * rh))
	{
		return false;
	}
	fx = cx - static_cast<double>(bx);  // exact
	fy = cy - static_cast<double>(by);
	return true;
}

// The fixed-point grid of one unit's value image: make_consts' exponent k (from norm alone) raised until the
// unit's events cannot fill a pixel, n_ev * norm < 2^(11 + k) (a pixel wraps at 2^(12 + k)).  Units below that
// keep make_consts' grid, and its bits.
// preX, preY: the prefactors of the subnormal form of a tap (fix_form.h) on the same grid -- preY is halved wherever the
// bias is doubled.  Uniform over the workgroup: preX is a kernel argument (scalar); preY takes the uniform vector register
// pair the bias held in the scatter (forced into scalars with readfirstlane, k_eval3<true> spills one at its 106).
__device__ __forceinline__ void unit_fix_grid(const EvalConsts& c, uint32_t nEv, double& bias, double& scale, double& preX,
											  double& preY)
{
	bias = c.fix_bias;  // 1.5 * 2^k
	scale = c.fix_scale;
	preY = c.fix_pre_y;
	const double top = static_cast<double>(nEv) * c.norm * (1.5 / 2048.0);  // n_ev * norm >= 2^(11 + k) <=> top >= bias
	while (top >= bias)
	{
		bias *= 2.0;
		scale *= 2.0;
		preY *= 0.5;
	}
	preX = c.fix_pre_x;
}

__device__ __forceinline__ void unit_fix_grid(const EvalConsts& c, uint32_t nEv, double& bias, double& scale)
{
	double preX, preY;
	unit_fix_grid(c, nEv, bias, scale, preX, preY);
}

// w[k] = pre * exp(hs (k-3-f)^2), k = 0..6, from three exps.
__device__ __forceinline__ void axis_taps(double f, double pre, const EvalConsts& c, double (&w)[7])
{
	const double e0 = pre * exp(c.hs * (f * f));
	const double a = f * c.inv_sigsq;
	const double p = exp(a);
	const double q = exp(-a);
	const double p2 = p * p, q2 = q * q;
	const double e1 = c.ck1 * e0, e2 = c.ck2 * e0, e3 = c.ck3 * e0;
	w[3] = e0;
	w[4] = e1 * p;
	w[5] = e2 * p2;
	w[6] = e3 * (p2 * p);
	w[2] = e1 * q;
	w[1] = e2 * q2;
	w[0] = e3 * (q2 * q);
}

__device__ __forceinline__ void block_minmax(int& xmin, int& xmax, int& ymin, int& ymax, int* ired)
{
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	const int nw = (blockDim.x + 63) >> 6;
	xmin = wave_min(xmin);
	xmax = wave_max(xmax);
	ymin = wave_min(ymin);
	ymax = wave_max(ymax);
	__syncthreads();
	if (lane == kWaveResultLane)
	{
		ired[wave * 4 + 0] = xmin;
		ired[wave * 4 + 1] = xmax;
		ired[wave * 4 + 2] = ymin;
		ired[wave * 4 + 3] = ymax;
	}
	__syncthreads();
	xmin = ired[0];
	xmax = ired[1];
	ymin = ired[2];
	ymax = ired[3];
	for (int w = 1; w < nw; ++w)
	{
		xmin = min(xmin, ired[w * 4 + 0]);
		xmax = max(xmax, ired[w * 4 + 1]);
		ymin = min(ymin, ired[w * 4 + 2]);
		ymax = max(ymax, ired[w * 4 + 3]);
	}
}

// Adds the row tiles of each unit in tile order and finishes the objective.
// flow sets: 1 (C = 1 or 3), or 5 value-only sets for central differences.
__global__ void k_combine_variance(const Unit* __restrict__ units, int nUnits,
								   const double* __restrict__ flows, int tiles, int sets,
								   int channels, double fdStep,
								   const double* __restrict__ partials, double* __restrict__ out,
								   EvalConsts c)
{
	const int unit = blockIdx.x * blockDim.x + threadIdx.x;
	if (unit >= nUnits)
	{
		return;
	}
	const Unit u = units[unit];
	if (u.flags & kUnitStray)
	{
		return;  // stray buckets carry no objective and own no output slot
	}
	double res[5] = {0, 0, 0, 0, 0};
	double j0 = 0.0, j1 = 0.0;
	if (u.flags & kUnitActive)
	{
		for (int s = 0; s < sets; ++s)
		{
			double S[7] = {0, 0, 0, 0, 0, 0, 0};
			const double* p =
				partials + ((static_cast<size_t>(s) * nUnits + unit) * tiles) * kPartialStride;
			for (int t = 0; t < tiles; ++t)
			{
				for (int k = 0; k < 7; ++k)
				{
					S[k] += p[t * kPartialStride + k];
				}
			}
			double m0 = flows[2 * u.flow_idx];
			double m1 = flows[2 * u.flow_idx + 1];
			fd_offset(s, fdStep, m0, m1);
			double a = 0.0, b = 0.0;
			variance_from_sums(S, channels == 3, m0, m1, c.max_res, res[s], a, b);
			if (s == 0)
			{
				j0 = a;
				j1 = b;
			}
		}
		if (sets == 5)
		{
			j0 = (res[1] - res[2]) / (2.0 * fdStep);
			j1 = (res[3] - res[4]) / (2.0 * fdStep);
		}
	}
	out[3 * u.flow_idx + 0] = res[0];
	out[3 * u.flow_idx + 1] = j0;
	out[3 * u.flow_idx + 2] = j1;
}

// Diagnostic: the image of warped events of one unit, tile by tile, to HBM.
template <int C>
__global__ void k_dump_image(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
							 int unit, const double* __restrict__ flow, int tiles,
							 double* __restrict__ image, EvalConsts c)
{
	extern __shared__ double lds[];
	const Unit u = units[unit];
	const int W3 = 3 * u.rw;
	const int H3 = 3 * u.rh;
	const int R = (H3 + tiles - 1) / tiles;
	const size_t full = static_cast<size_t>(W3) * H3;
	for (int tile = 0; tile < tiles; ++tile)
	{
		const int r0 = tile * R;
		const int rows = min(R, H3 - r0);
		if (rows <= 0)
		{
			break;
		}
		const int plane = rows * W3;
		for (int i = threadIdx.x; i < C * plane; i += blockDim.x)
		{
			lds[i] = 0.0;
		}
		__syncthreads();
		splat_rows<C>(events + u.ev_off, u.n_ev, u.rx, u.ry, u.rw, u.rh, r0, rows, flow[0],
					  flow[1], c, lds, plane);
		__syncthreads();
		for (int ch = 0; ch < C; ++ch)
		{
			for (int i = threadIdx.x; i < plane; i += blockDim.x)
			{
				image[ch * full + static_cast<size_t>(r0) * W3 + i] = lds[ch * plane + i];
			}
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------
// Device-resident solve, one workgroup per patch (EBO_SOLVE_INDEPENDENT).
// Trust-region Levenberg-Marquardt exactly as ebo_solver_opts describes it
// (Ceres 2.0: TrustRegionMinimizer, LevenbergMarquardtStrategy,
// TrustRegionStepEvaluator) on a 1-residual / 2-parameter problem, options of
// feature_detector.cpp:401-410.  Every thread carries the (uniform) solver state;
// the objective is evaluated cooperatively.  No host round trips.
// ---------------------------------------------------------------------------
#include "ebo_extents.inc"
#include "ebo_eval3.inc"

// The objective and its Jacobian at (m0, m1) of a unit evaluated as one row band.  (A function of its own: written
// out inside k_solve_independent, the same statements compile to a different instruction schedule.)
template <bool SMALL>
__device__ __forceinline__ void eval_unit(const uint64_t* __restrict__ ev, const Unit& u, double m0, double m1,
										   bool wantJac, int capDoubles, const EvalConsts& c, double* lds, double& r,
										   double& j0, double& j1, EvalReuse* ru, const int32_t* __restrict__ ext)
{
	double S[7];
	eval_unit3<SMALL, false>(ev, u, m0, m1, wantJac, 0, 1, capDoubles, c, lds, S, ebo::kEvalHeaderWavesMax, ru, ext);  // (the gather forms D1: ebo_eval3.inc)
	j0 = 0.0;
	j1 = 0.0;
	variance_from_sums(S, wantJac, m0, m1, c.max_res, r, j0, j1);
}

// The whole trust-region LM of ONE 2-parameter, 1-residual problem (the per-patch problem of
// EBO_SOLVE_INDEPENDENT; Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy with the options
// of feature_detector.cpp:401-410) as a resumable state machine, replicated in every thread of the
// workgroup (uniform control flow).  The kernel owns ONE evaluation site:
//     lm.begin();  do { evaluate(lm.q0, lm.q1, lm.qJac) -> r, J0, J1 } while (lm.advance(r, J0, J1, o));
// (three inlined copies of an objective as large as the edge loss made the register allocator
// spill several hundred VGPRs).  Value-only for the cost at a candidate, value + Jacobian after an
// accepted step -- the sequence Ceres follows.
struct LmUnit
{
	// the evaluation wanted next
	double q0, q1;
	bool qJac;
	// results
	double best0, best1;
	int iteration, evalsCost, evalsJac, termination;
	// solver state
	int phase;  // 0: first evaluation, 1: cost at a candidate, 2: Jacobian at an accepted point
	double x0, x1, f, J0, J1, xCost, g0, g1, sc0, sc1, j0, j1, xNorm, gradMax, minimumCost;
	double seMinimum, seCurrent, seReference, seCandidate, seAccRef, seAccCand;
	int seNumNonmono;
	double radius, decreaseFactor, d0, d1;
	bool reuseDiagonal, lastSuccessful;
	int numInvalid;
	double c0, c1, modelCostChange, candCost, quality;

	// Where the objective needs the registers (the edge loss), the state lives in LDS and ONE lane
	// runs the solver between two evaluations (k_solve_edge): replicated in every lane it is ~100
	// VGPRs that stay live across the objective (176-185 spilled VGPRs, ~0.5 KB of scratch per lane in
	// round 2), and replicated in every WAVE the solver's serial f64 code (divisions, square roots)
	// cost the workgroup as many vector instructions as a value-only evaluation itself.
	int more;  // k_solve_edge: advance()'s answer, for the other waves

	__device__ __forceinline__ void begin()
	{
		best0 = best1 = 0.0;
		iteration = evalsCost = evalsJac = 0;
		termination = 1;
		phase = 0;
		more = 1;
		x0 = x1 = 0.0;  // feature_detector.cpp:318-326
		q0 = q1 = 0.0;
		qJac = true;
	}

	// the loop of TrustRegionMinimizer from its top to the next evaluation; false = finished
	__device__ __forceinline__ bool next_step(const SolveConsts& o)
	{
		for (;;)
		{
			if (lastSuccessful && xCost < minimumCost)
			{
				minimumCost = xCost;
				best0 = x0;
				best1 = x1;
			}
			if (iteration >= o.max_num_iterations)
			{
				termination = 1;
				return false;
			}
			if (lastSuccessful && gradMax <= o.gradient_tolerance)
			{
				termination = 0;
				return false;
			}
			if (radius < o.min_radius)
			{
				termination = 0;
				return false;
			}
			iteration++;
			lastSuccessful = false;

			if (!reuseDiagonal)
			{
				d0 = fmin(fmax(j0 * j0, o.min_lm_diagonal), o.max_lm_diagonal);
				d1 = fmin(fmax(j1 * j1, o.min_lm_diagonal), o.max_lm_diagonal);
			}
			const double l0 = sqrt(d0 / radius);
			const double l1 = sqrt(d1 / radius);
			reuseDiagonal = true;
			// (J'J + D'D) y = J'f by Cholesky; step = -y.
			const double h00 = j0 * j0 + l0 * l0;
			const double h10 = j1 * j0;
			const double h11 = j1 * j1 + l1 * l1;
			bool valid = (h00 > 0.0) && isfinite(h00);
			double s0 = 0.0, s1 = 0.0;
			if (valid)
			{
				const double L00 = sqrt(h00);
				const double L10 = h10 / L00;
				const double dd = h11 - L10 * L10;
				valid = (dd > 0.0) && isfinite(dd);
				if (valid)
				{
					const double L11 = sqrt(dd);
					double b0 = (j0 * f) / L00;
					double b1 = ((j1 * f) - L10 * b0) / L11;
					b1 = b1 / L11;
					b0 = (b0 - L10 * b1) / L00;
					valid = isfinite(b0) && isfinite(b1);
					s0 = -b0;
					s1 = -b1;
				}
			}
			modelCostChange = 0.0;
			if (valid)
			{
				const double mr = j0 * s0 + j1 * s1;
				modelCostChange = 0.0 - mr * (f + mr / 2.0);
				valid = modelCostChange > 0.0;
			}
			if (!valid)
			{
				numInvalid++;
				if (numInvalid >= o.max_invalid)
				{
					termination = 2;
					return false;
				}
				radius *= 0.5;
				reuseDiagonal = true;
				continue;
			}
			numInvalid = 0;
			c0 = x0 + s0 * sc0;
			c1 = x1 + s1 * sc1;
			q0 = c0;
			q1 = c1;
			qJac = false;
			phase = 1;
			return true;
		}
	}

	// takes the result of the evaluation asked for; true = another evaluation is wanted
	__device__ __forceinline__ bool advance(double r, double a, double b, const SolveConsts& o)
	{
		if (phase == 0)
		{
			f = r;
			J0 = a;
			J1 = b;
			evalsJac++;
			xCost = 0.5 * f * f;
			termination = 1;
			if (!isfinite(xCost))
			{
				termination = 2;
				return false;
			}
			g0 = J0 * f;
			g1 = J1 * f;
			sc0 = 1.0;
			sc1 = 1.0;
			if (o.jacobi_scaling)
			{
				sc0 = 1.0 / (1.0 + sqrt(J0 * J0));
				sc1 = 1.0 / (1.0 + sqrt(J1 * J1));
			}
			j0 = J0 * sc0;
			j1 = J1 * sc1;
			xNorm = sqrt(x0 * x0 + x1 * x1);
			gradMax = fmax(fabs(g0), fabs(g1));
			minimumCost = xCost;
			seMinimum = seCurrent = seReference = seCandidate = xCost;
			seAccRef = seAccCand = 0.0;
			seNumNonmono = 0;
			radius = o.initial_radius;
			decreaseFactor = 2.0;
			// iteration zero counts as successful: a start already within the gradient
			// tolerance converges immediately
			reuseDiagonal = false;
			lastSuccessful = true;
			d0 = d1 = 0.0;
			numInvalid = 0;
		}
		else if (phase == 1)
		{
			evalsCost++;
			candCost = 0.5 * r * r;
			if (!isfinite(candCost))
			{
				candCost = 1.7976931348623157e308;
			}
			const double e0 = x0 - c0, e1 = x1 - c1;
			const double stepNorm = sqrt(e0 * e0 + e1 * e1);
			if (stepNorm <= o.parameter_tolerance * (xNorm + o.parameter_tolerance))
			{
				termination = 0;
				return false;
			}
			const double costChange = xCost - candCost;
			if (fabs(costChange) <= o.function_tolerance * xCost)
			{
				termination = 0;
				return false;
			}
			const double relDec = (seCurrent - candCost) / modelCostChange;
			const double histDec = (seReference - candCost) / (seAccRef + modelCostChange);
			quality = fmax(relDec, histDec);
			if (quality > o.min_relative_decrease)
			{
				x0 = c0;
				x1 = c1;
				xNorm = sqrt(x0 * x0 + x1 * x1);
				q0 = x0;
				q1 = x1;
				qJac = true;
				phase = 2;
				return true;
			}
			radius = radius / decreaseFactor;
			decreaseFactor *= 2.0;
			reuseDiagonal = true;
		}
		else
		{
		// phase 2: the Jacobian at the accepted point
		f = r;
		J0 = a;
		J1 = b;
		evalsJac++;
		xCost = 0.5 * f * f;
		if (!isfinite(xCost))
		{
			termination = 2;
			return false;
		}
		g0 = J0 * f;
		g1 = J1 * f;
		j0 = J0 * sc0;
		j1 = J1 * sc1;
		gradMax = fmax(fabs(g0), fabs(g1));
		lastSuccessful = true;
		const double q = 2.0 * quality - 1.0;
		radius = radius / fmax(1.0 / 3.0, 1.0 - q * q * q);
		radius = fmin(o.max_radius, radius);
		decreaseFactor = 2.0;
		reuseDiagonal = false;
		seCurrent = candCost;
		seAccCand += modelCostChange;
		seAccRef += modelCostChange;
		if (seCurrent < seMinimum)
		{
			seMinimum = seCurrent;
			seNumNonmono = 0;
			seCandidate = seCurrent;
			seAccCand = 0.0;
		}
		else
		{
			++seNumNonmono;
			if (seCurrent > seCandidate)
			{
				seCandidate = seCurrent;
				seAccCand = 0.0;
			}
		}
		if (seNumNonmono == o.max_nonmono)
		{
			seReference = seCandidate;
			seAccRef = seAccCand;
		}
		}
		// ONE copy of the loop's top (three inlined copies cost the kernels that hold this solver ~70 VGPRs)
		return next_step(o);
	}
};

// SMALL: exp_taps.h's polynomials (sigma >= 1) instead of the library exp (ebo_eval3.inc)
template <bool SMALL>
__global__ void __launch_bounds__(512) k_solve_independent(const uint64_t* __restrict__ events,
									const Unit* __restrict__ units, int capDoubles,
									double* __restrict__ flowsOut, int32_t* __restrict__ stats,
									EvalConsts c, SolveConsts o, int noReuse, const uint32_t* __restrict__ order,
									const int32_t* __restrict__ unitExt)
{
	extern __shared__ double lds[];
	const uint32_t unit = order[blockIdx.x];  // heaviest first (launch_order.h): n_ev is the known part of a solve's length
	const Unit u = units[unit];
	const int32_t* ext = unitExt ? unitExt + static_cast<size_t>(unit) * kExtStride : nullptr;  // box_extents.h
	const uint64_t* ev = events + u.ev_off;
	int iteration = 0, evalsCost = 0, evalsJac = 0, termination = 0;
	double best0 = 0.0, best1 = 0.0;

	if (u.flags & kUnitActive)
	{
		// The solver state lives in LDS (the reduction scratch rows of waves 8..15, which a workgroup of
		// at most 512 lanes never uses) and thread 0 runs the solver between two evaluations: replicated
		// in every wave its serial f64 code (divisions, square roots) was a fifth of the workgroup's
		// vector instructions, replicated in every lane ~100 VGPRs live across the objective.
		static_assert(sizeof(LmUnit) <= 64 * sizeof(double), "LmUnit must fit red[64..127]");
		LmUnit& lm = *reinterpret_cast<LmUnit*>(lds + 64);
		// the record of the image in LDS (ebo_eval3.inc, EvalReuse): doubles 148..157 of the header, behind the 32
		// ints the bounding-box reduction uses (at most eight waves)
		EvalReuse* ru = !noReuse ? reinterpret_cast<EvalReuse*>(lds + kRedDoubles + 20) : nullptr;
		static_assert(sizeof(EvalReuse) <= (kLdsHeader - kRedDoubles - 20) * sizeof(double), "EvalReuse must fit the header");
		if (threadIdx.x == 0)
		{
			lm.begin();
			if (ru)
			{
				ru->valid = 0.0;
			}
		}
		for (;;)
		{
			__syncthreads();  // the point to evaluate (or the end) is published; every thread is past the previous evaluation
			if (!lm.more)
			{
				break;
			}
			const double q0 = lm.q0, q1 = lm.q1;
			const bool qJac = lm.qJac;
			double r, a, b;
			eval_unit<SMALL>(ev, u, q0, q1, qJac, capDoubles, c, lds, r, a, b, ru, ext);
			if (threadIdx.x == 0)
			{
				lm.more = lm.advance(r, a, b, o) ? 1 : 0;
			}
		}
		if (threadIdx.x == 0)
		{
			iteration = lm.iteration;
			evalsCost = lm.evalsCost;
			evalsJac = lm.evalsJac;
			termination = lm.termination;
			best0 = lm.best0;
			best1 = lm.best1;
		}
	}
	if (threadIdx.x == 0 && !(u.flags & kUnitStray))
	{
		flowsOut[2 * u.flow_idx] = best0;
		flowsOut[2 * u.flow_idx + 1] = best1;
		if (stats)
		{
			stats[4 * u.flow_idx + 0] = iteration;
			stats[4 * u.flow_idx + 1] = evalsCost;
			stats[4 * u.flow_idx + 2] = evalsJac;
			stats[4 * u.flow_idx + 3] = termination;
		}
	}
}

constexpr float kSureBase = 0.499999f;  // 0.5 - 1e-6: slack for the f64 roundings of the reference's own expression

// Destination pixel of one event for the count images; MODE = EBO_COUNT_*.  Returns false
// when the event contributes nothing (outside the image, or a coordinate the reference's
// int conversion does not define).  Straight-line code: every lane of a wave runs it.
//   MODE 1: newP = round(p + (t_ref - t) * scale * mf[patch])      feature_detector.cpp:443-451
//   MODE 2: same with the float32 field at the event's own pixel   :276-285
template <int MODE>
__device__ __forceinline__ bool count_target(uint64_t rec, bool live, int dtWin, double m0, double m1,
											 const float* __restrict__ field /* window's field */,
											 const EvalConsts& c, int& nx, int& ny)
{
	int x, y, pos, dt;
	unpack(rec, x, y, pos, dt);
	nx = x;
	ny = y;
	if (MODE != 0)
	{
		if (MODE == 2)
		{
			live = live && x >= 0 && x < c.image_w && y >= 0 && y < c.image_h;
			const size_t at = live ? 2 * (static_cast<size_t>(y) * c.image_w + x) : 0;
			const float2 f = *reinterpret_cast<const float2*>(field + at);
			m0 = static_cast<double>(f.x);
			m1 = static_cast<double>(f.y);
		}
		// Float first.  The reference's position is fl64(x + fl64(fl64(dtw * scale) * m)); the same
		// expression in float differs from it by at most 4e-7 |displacement| + 6e-8 |position| (five
		// roundings of 2^-24 on the product, one on the sum, inputs rounded to float).  If the float
		// value is farther than that (+ 1e-6) from every half-integer, both round to the same pixel,
		// and the double arithmetic (half-rate, conversions, truncations and compares) is not needed.
		// Anything else -- a value near a rounding boundary (0.04 % of the events at sensor
		// coordinates: a wave of 64 takes the exact branch 2-3 % of the time; with the position term
		// bounded by its worst case 2^15 instead, 0.8 % and 40 %), huge, infinite or NaN (comparisons
		// false) -- takes the exact path below.
		const float prod = static_cast<float>(dt + dtWin) * static_cast<float>(c.scale);
		const float px = prod * static_cast<float>(m0), py = prod * static_cast<float>(m1);
		const float vx = static_cast<float>(x) + px, vy = static_cast<float>(y) + py;
		const float rx = rintf(vx), ry = rintf(vy);
		const bool sure = fabsf(vx - rx) < kSureBase - 4e-7f * fabsf(px) - 6e-8f * fabsf(vx) &&
						  fabsf(vy - ry) < kSureBase - 4e-7f * fabsf(py) - 6e-8f * fabsf(vy);
		if (sure)
		{
			nx = static_cast<int>(rx);
			ny = static_cast<int>(ry);
		}
		else
		{
			const double dtw = static_cast<double>(dt + dtWin);
			const double fx = static_cast<double>(x) + dtw * c.scale * m0;
			const double fy = static_cast<double>(y) + dtw * c.scale * m1;
			live = live && convertible(fx) && convertible(fy);
			nx = static_cast<int>(round(live ? fx : 0.0));
			ny = static_cast<int>(round(live ? fy : 0.0));
		}
	}
	return live && nx >= 0 && nx < c.image_w && ny >= 0 && ny < c.image_h;
}

// The flow of the patch a stray event (outside the sensor) is attributed to in the final
// loop (:436-441, index clamped at 0: negative indices are undefined there).
__device__ __forceinline__ void stray_flow(uint64_t rec, const double* __restrict__ windowFlows,
										   const EvalConsts& c, double& m0, double& m1)
{
	int x, y, pos, dt;
	unpack(rec, x, y, pos, dt);
	const int px = max(min(x / c.patch_w, c.npx - 1), 0);
	const int py = max(min(y / c.patch_h, c.npy - 1), 0);
	m0 = windowFlows[2 * (py * c.npx + px)];
	m1 = windowFlows[2 * (py * c.npx + px) + 1];
}

// Exclusive prefix sum of one value per thread over the workgroup (wave scans by shuffles, then
// the wave totals); tmp: at least blockDim / 64 + 1 words of LDS.  Returns the exclusive prefix,
// total = sum over the workgroup.  Ends with the values in tmp still needed: callers barrier before
// reusing tmp.
__device__ __forceinline__ unsigned int block_exclusive_scan(unsigned int v, unsigned int* tmp, unsigned int& total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nWaves = (blockDim.x + 63) >> 6;
	unsigned int incl = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1)
	{
		const unsigned int up = __shfl_up(incl, d, 64);
		if (lane >= d)
		{
			incl += up;
		}
	}
	if (lane == 63)
	{
		tmp[wave] = incl;
	}
	__syncthreads();
	unsigned int before = 0;
	total = 0;
	for (int k = 0; k < nWaves; ++k)
	{
		const unsigned int t = tmp[k];
		before += k < wave ? t : 0u;
		total += t;
	}
	return before + incl - v;
}

// LDS rates in the evaluation kernels' own access shape, measured in the run that quotes them (bench.py's roofline.lds;
// the same loop as tools/microbench/lds_atomics.hip, "7x7 taps ..., any base"): per "event" a pseudo-random base slot per
// lane, then the 49 taps of a 7 x 7 footprint at immediate offsets (row pitch 41 slots) as 64-bit LDS atomic adds (ATOMIC)
// or single 64-bit LDS reads -- what k_eval3's scatter and gather issue.  `iters` operations per lane (a multiple of 49),
// 4 workgroups of 256 lanes per CU.  (Rounds 1-3 probed ONE random operation per loop trip with the generator in between,
// a latency-bound figure 15-25 % below these.)
template <bool ATOMIC>
__global__ void __launch_bounds__(256) k_lds_rate(double* __restrict__ sink, int iters)
{
	constexpr int kElems = 4096, kPitch = 41;
	__shared__ unsigned long long cell[kElems + 7 * kPitch];
	for (int i = threadIdx.x; i < kElems + 7 * kPitch; i += blockDim.x)
	{
		cell[i] = static_cast<unsigned long long>(i);
	}
	__syncthreads();
	unsigned rnd = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 12345u;
	unsigned long long acc = 0;
	for (int ev = 0; ev < iters / 49; ++ev)
	{
		rnd = rnd * 1664525u + 1013904223u;
		unsigned long long* p = cell + ((rnd >> 10) & (kElems - 1));
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				if (ATOMIC)
				{
					atomicAdd(p + j * kPitch + i, 1ull);
				}
				else
				{
					acc += __hip_atomic_load(p + j * kPitch + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);  // one ds_read_b64 (lds_ld)
				}
			}
		}
	}
	__syncthreads();
	for (int i = threadIdx.x; i < kElems; i += blockDim.x)
	{
		acc += cell[i];
	}
	if (acc == 0x0123456789abcdefull)  // never: keeps the loads and the adds alive
	{
		sink[blockIdx.x] = 1.0;
	}
}

// Yardstick of the count-image kernels (bench.py, diagnostic): the same bytes with no work -- every packed
// event read once with 16-byte loads, every image pixel written once with 16-byte stores -- by 2048
// workgroups that each take a contiguous slice of both.  What this reaches on the chip is what "100 %"
// means for a kernel of that traffic (the loads are kept alive by an XOR the compiler must produce).
__global__ void __launch_bounds__(256) k_stream_yardstick(const uint4* __restrict__ events16, size_t nEv16,
														   double2* __restrict__ image16, size_t nPx16)
{
	// grid-stride over both streams at once, four 16-byte loads and four 16-byte stores in flight per lane:
	// reads and writes are interleaved at instruction level everywhere on the chip
	const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
	const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	const size_t n = nEv16 > nPx16 ? nEv16 : nPx16;
	unsigned int x = 0;
	const double2 zero = make_double2(0.0, 0.0);
	for (size_t i = first; i < n; i += 4 * stride)
	{
		const size_t i1 = i + stride, i2 = i + 2 * stride, i3 = i + 3 * stride;
		const uint4 a = (i < nEv16) ? events16[i] : make_uint4(0, 0, 0, 0);
		const uint4 b = (i1 < nEv16) ? events16[i1] : make_uint4(0, 0, 0, 0);
		const uint4 c = (i2 < nEv16) ? events16[i2] : make_uint4(0, 0, 0, 0);
		const uint4 d = (i3 < nEv16) ? events16[i3] : make_uint4(0, 0, 0, 0);
		if (i < nPx16) image16[i] = zero;
		if (i1 < nPx16) image16[i1] = zero;
		if (i2 < nPx16) image16[i2] = zero;
		if (i3 < nPx16) image16[i3] = zero;
		x ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
	}
	asm volatile("" ::"v"(x));  // the loads are used
}

// The final image of warped events (feature_detector.cpp:433-463) of windows whose patches are SHARDED
// over ranks (BASELINE config 4): the context holds, per window, the units of this rank's
// patch rows (ebo_set_patches), `flows` are those of ALL patches of the grid (after the all-gather of
// the solved flows) and dtWin[unit] = t_ref(window) - t_ref(unit) with the WINDOW's reference time,
// which a shard cannot derive from its own events.  Workgroup = unit; every event takes the flow of
// the grid patch its own coordinates select (:436-441) and adds 1.0 at its rounded warped position.
// The partial images of the ranks are integer-valued doubles: their sum is exact in any order.
__global__ void k_count_shard(const uint64_t* __restrict__ events, const Unit* __restrict__ units, int unitsPerWindow,
							  const BandUnit* __restrict__ table, const double* __restrict__ flows,
							  double* __restrict__ image, EvalConsts c)
{
	const Unit un = units[blockIdx.x];
	const int w = blockIdx.x / unitsPerWindow;
	const int P = c.npx * c.npy;
	const double* windowFlows = flows + 2 * static_cast<size_t>(w) * P;
	double* img = image + static_cast<size_t>(w) * c.image_w * c.image_h;
	const int dtw = table[blockIdx.x].dt_win;
	for (uint32_t e = threadIdx.x; e < un.n_ev; e += blockDim.x)
	{
		const uint64_t rec = events[un.ev_off + e];
		double m0, m1;
		stray_flow(rec, windowFlows, c, m0, m1);
		int nx, ny;
		if (count_target<1>(rec, true, dtw, m0, m1, nullptr, c, nx, ny))
		{
			unsafeAtomicAdd(&img[static_cast<size_t>(ny) * c.image_w + nx], 1.0);  // exact on integer counts
		}
	}
}

#include "ebo_count.inc"

// Patch::integrateEvents (patch.cpp:65-85) / integrateMotionCompensatedEvents
// (patch.cpp:87-130): signed counts in an LDS tile, one workgroup per patch.
__global__ void k_patch_integrate(const uint64_t* __restrict__ events,
								  const uint32_t* __restrict__ offsets,
								  const double* __restrict__ rects, const double* __restrict__ traj,
								  const uint64_t* __restrict__ nablaOff, double* __restrict__ nabla)
{
	extern __shared__ int tile[];
	const int p = blockIdx.x;
	const double rx = rects[4 * p + 0], ry = rects[4 * p + 1];
	const double rw = rects[4 * p + 2], rh = rects[4 * p + 3];
	const int cols = static_cast<int>(rw);
	const int rows = static_cast<int>(rh);
	double* out = nabla + nablaOff[p];
	double dirX = 0.0, dirY = 0.0, tDif = 1.0;
	bool mc = traj != nullptr;
	if (mc)
	{
		if (traj[4 * p + 3] == 0.0)
		{
			return;  // patch.cpp:99-100 time test failed: image left untouched
		}
		dirX = traj[4 * p + 0];
		dirY = traj[4 * p + 1];
		tDif = traj[4 * p + 2];
	}
	for (int i = threadIdx.x; i < rows * cols; i += blockDim.x)
	{
		tile[i] = 0;
	}
	__syncthreads();
	const uint32_t e0 = offsets[p], e1 = offsets[p + 1];
	for (uint32_t e = e0 + threadIdx.x; e < e1; e += blockDim.x)
	{
		int x, y, pos, dt;
		unpack(events[e], x, y, pos, dt);
		int ix = x, iy = y;
		if (mc)
		{
			const double f = static_cast<double>(dt) / tDif;
			const double cx = static_cast<double>(x) + f * dirX;
			const double cy = static_cast<double>(y) + f * dirY;
			if (!convertible(cx) || !convertible(cy))
			{
				continue;
			}
			ix = static_cast<int>(rint(cx));  // cv::saturate_cast<int>: half to even
			iy = static_cast<int>(rint(cy));
		}
		const double dx = static_cast<double>(ix);
		const double dy = static_cast<double>(iy);
		if (rx <= dx && dx < rx + rw && ry <= dy && dy < ry + rh)
		{
			const int px = static_cast<int>(dx - rx);
			const int py = static_cast<int>(dy - ry);
			atomicAdd(&tile[py * cols + px], pos ? 1 : -1);
		}
	}
	__syncthreads();
	for (int i = threadIdx.x; i < rows * cols; i += blockDim.x)
	{
		out[i] = static_cast<double>(tile[i]);
	}
}

// FeatureDetector::updatePatches' routing test for a chunk of the stream (feature_detector.cpp:
// 589-596, cv::Rect2d::contains on the integer point): one wave per tracked patch walks the
// chunk from start[p], 256 events per step (four coalesced 256-byte loads), compacts the indices
// of the events inside the rect with ballots -- no barriers, no atomics, stream order kept -- and
// stops at the event that fills the patch's quota.
__global__ void __launch_bounds__(64) k_route(const uint32_t* __restrict__ xy, uint32_t nEvents,
											  const double* __restrict__ rects, const uint32_t* __restrict__ start,
											  const uint32_t* __restrict__ take, uint32_t cap,
											  uint32_t* __restrict__ outIndex, uint32_t* __restrict__ outCount,
											  uint32_t* __restrict__ outNext)
{
	const int p = blockIdx.x;
	const double rx = rects[4 * p + 0], ry = rects[4 * p + 1];
	const double rx1 = rx + rects[4 * p + 2], ry1 = ry + rects[4 * p + 3];
	const uint32_t quota = min(take[p], cap);
	uint32_t* out = outIndex + static_cast<size_t>(p) * cap;
	const int lane = threadIdx.x;
	uint32_t taken = 0;
	uint32_t next = nEvents;
	for (uint32_t base = start[p]; base < nEvents && taken < quota; base += 256)
	{
		uint32_t v[4];
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			const uint32_t e = base + k * 64 + lane;
			v[k] = e < nEvents ? xy[e] : 0u;
		}
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			const uint32_t e = base + k * 64 + lane;
			const double px = static_cast<double>(static_cast<int>(static_cast<int16_t>(v[k] & 0xFFFFu)));
			const double py = static_cast<double>(static_cast<int>(static_cast<int16_t>(v[k] >> 16)));
			const bool in = e < nEvents && rx <= px && px < rx1 && ry <= py && py < ry1;
			const unsigned long long m = __ballot(in);
			const uint32_t rank = taken + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
			if (in && rank < quota)
			{
				out[rank] = e;
				if (rank + 1 == quota)
				{
					next = e + 1;  // exactly one lane of the whole walk
				}
			}
			taken += static_cast<uint32_t>(__popcll(m));
		}
	}
	// `next` lives in the lane that took the last event: publish it to the wave
	const unsigned long long who = __ballot(next != nEvents);
	if (who)
	{
		next = __shfl(next, __ffsll(static_cast<long long>(who)) - 1);
	}
	if (lane == 0)
	{
		outCount[p] = min(taken, quota);
		outNext[p] = (quota == 0) ? start[p] : next;
	}
}

#include "ebo_edge.inc"
#include "ebo_bucket.inc"
#include "ebo_camera.inc"
#include "ebo_twoview.inc"
#include "ebo_abspose.inc"
#include "ebo_bundle.inc"
#include "ebo_relpose.inc"
#include "ebo_align.inc"
#include "ebo_rpe.inc"
#include "ebo_trackerr.inc"
#include "ebo_landmark.inc"
#include "ebo_rotation.inc"
#include "ebo_depth.inc"
#include "ebo_maptrack.inc"
#include "ebo_field.inc"
#include "ebo_fieldtv.inc"
#include "ebo_optimizer.inc"
#include "ebo_band.inc"
#include "ebo_frontend.inc"

int check_launch()
{
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename K>
int allow_big_lds(K kernel, size_t bytes)
{
	if (bytes <= 64 * 1024)
	{
		return 0;
	}
	return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
							   hipFuncAttributeMaxDynamicSharedMemorySize,
							   static_cast<int>(bytes)) == hipSuccess
			   ? 0
			   : -2;
}

}  // namespace

int launch_unit_extents(const uint64_t* d_events, const Unit* d_units, int n_units, int32_t* d_unit_ext, void* stream)
{
	if (n_units == 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_unit_extents, dim3(n_units), dim3(256), 0, static_cast<hipStream_t>(stream), d_events, d_units, d_unit_ext);
	return check_launch();
}

namespace
{
// the instantiation of k_eval3 a launch runs: sigma >= 1 (and not the A/B build's guarded biased form) takes <true>
bool eval_variance_small(const EvalConsts& c)
{
	return c.inv_sigsq <= 1.0 && c.fix_form != kFixBiasedGuard;
}
auto eval_variance_kernel(const EvalConsts& c)
{
	return eval_variance_small(c) ? k_eval3<true> : k_eval3<false>;
}
}  // namespace

int eval_variance_waves_per_cu(const EvalConsts& c)
{
	// __launch_bounds__(512, 4) / (512, 3): four resp. three waves on each of a CU's four SIMDs
	return eval_variance_small(c) ? 16 : 12;
}

int eval_variance_resident(const EvalLaunch& L, int* groups)
{
	auto kern = eval_variance_kernel(L.c);
	if (allow_big_lds(kern, L.lds_bytes))
	{
		return -2;
	}
	return hipOccupancyMaxActiveBlocksPerMultiprocessor(groups, kern, L.block, L.lds_bytes) == hipSuccess ? 0 : -2;
}

int launch_eval_variance(const EvalLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.n_units == 0)
	{
		return 0;
	}
	if (!L.d_order)
	{
		return -2;  // no launch without the units' order table
	}
	const dim3 grid(L.n_units * L.tiles, L.flow_sets);
	auto kern = eval_variance_kernel(L.c);
	if (allow_big_lds(kern, L.lds_bytes))
	{
		return -2;
	}
	const bool fusedPath = L.tiles == 1 && L.flow_sets == 1;
	LiveWindows live = L.live;
	if (!fusedPath)
	{
		live.n = 0;
	}
	hipLaunchKernelGGL(kern, live.n > 0 ? dim3(live.n * live.upw) : grid, dim3(L.block), L.lds_bytes, s, L.d_events, L.d_units,
					   L.d_flows, L.tiles, L.channels == 3 ? 1 : 0, L.cap_doubles, L.header_waves, L.fd_step,
					   L.d_partials, L.d_out, L.c, fusedPath ? L.d_modes : nullptr, live, L.d_order, L.box);
	if (check_launch())
	{
		return -2;
	}
	if (!fusedPath)
	{
		hipLaunchKernelGGL(k_combine_variance, dim3((L.n_units + 127) / 128), dim3(128), 0, s,
						   L.d_units, L.n_units, L.d_flows, L.tiles, L.flow_sets, L.channels,
						   L.fd_step, L.d_partials, L.d_out, L.c);
	}
	return check_launch();
}

int launch_init_field(const FieldLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t npx = static_cast<size_t>(L.w) * L.h;
	if (hipMemsetAsync(L.d_field, 0, npx * 2 * sizeof(float), s) != hipSuccess)
	{
		return -2;
	}
	hipLaunchKernelGGL(k_field_fixed, dim3(1), dim3(64), 0, s, L.w, L.h, L.scale, L.n_patches, L.d_off,
					   L.d_xy, L.d_t, L.timestamp, L.d_field, L.d_fixed, L.d_avg, L.d_nfixed);
	if (check_launch())
	{
		return -2;
	}
	hipLaunchKernelGGL(k_field_fill, dim3(static_cast<unsigned>((npx + 255) / 256)), dim3(256), 0, s, L.w,
					   L.h, L.use_average, L.d_field, L.d_fixed, L.d_avg, L.d_nfixed);
	return check_launch();
}

namespace
{
// grid sizes of the multigrid levels: halve until <= 256 nodes
int tvf_mg_dims(int w, int h, int (&lw)[12], int (&lh)[12])
{
	int n = 0;
	lw[0] = w;
	lh[0] = h;
	n = 1;
	while (lw[n - 1] * lh[n - 1] > 256 && n < 12)
	{
		lw[n] = (lw[n - 1] + 1) / 2;
		lh[n] = (lh[n - 1] + 1) / 2;
		++n;
	}
	return n;
}
size_t al256(size_t v)
{
	return (v + 255) & ~static_cast<size_t>(255);
}
}  // namespace

size_t tvf_workspace_bytes(int w, int h)
{
	const size_t n = static_cast<size_t>(w) * h;
	const size_t nAl = al256(n);
	size_t bytes = nAl /*mask*/ + 5 * nAl * 8 + 10 * nAl * 16 + 2 * (4 * 1024 * 8) + 256 /*scal*/;
	// multigrid: level 0 masked weights + x; levels >= 1 three weight arrays + three vectors
	int lw[12], lh[12];
	const int L = tvf_mg_dims(w, h, lw, lh);
	bytes += 2 * al256(n * 8) + al256(n * 16);
	for (int l = 1; l < L; ++l)
	{
		const size_t nl = static_cast<size_t>(lw[l]) * lh[l];
		bytes += 3 * al256(nl * 8) + 3 * al256(nl * 16);
	}
	return bytes;
}

void tvf_carve(TvfArgs& A, TvfMg& M, int w, int h, void* base, double2** xbest)
{
	const size_t n = static_cast<size_t>(w) * h;
	const size_t nAl = al256(n);
	char* b = static_cast<char*>(base);
	auto take = [&](size_t bytes) {
		char* r = b;
		b += al256(bytes);
		return r;
	};
	A.w = w;
	A.h = h;
	A.n = static_cast<int>(n);
	double2** v2[] = {&A.x, &A.xc, xbest, &A.g, &A.y, &A.r, &A.z, &A.p0, &A.p1, &A.q};
	for (double2** v : v2)
	{
		*v = reinterpret_cast<double2*>(take(nAl * 16));
	}
	double** v1[] = {&A.wh, &A.wv, &A.deg, &A.s2, &A.diag};
	for (double** v : v1)
	{
		*v = reinterpret_cast<double*>(take(nAl * 8));
	}
	A.partials = reinterpret_cast<double*>(take(4 * 1024 * 8));
	A.partials_rz = reinterpret_cast<double*>(take(4 * 1024 * 8));
	A.scal = reinterpret_cast<double*>(take(256));
	A.mask = reinterpret_cast<unsigned char*>(take(nAl));
	// multigrid hierarchy
	int lw[12], lh[12];
	M.levels = tvf_mg_dims(w, h, lw, lh);
	for (int l = 0; l < M.levels; ++l)
	{
		const size_t nl = static_cast<size_t>(lw[l]) * lh[l];
		TvfLevel& L = M.lv[l];
		L.w = lw[l];
		L.h = lh[l];
		M.wh_m[l] = reinterpret_cast<double*>(take(nl * 8));
		M.wv_m[l] = reinterpret_cast<double*>(take(nl * 8));
		if (l == 0)
		{
			M.diag_m[0] = A.diag;  // deg + damping, 1 on the pixels that are not free (k_tvf_cg_init)
			L.b = A.r;             // the CG residual
			L.x = reinterpret_cast<double2*>(take(nl * 16));
			L.xo = A.z;            // z = M^-1 r
		}
		else
		{
			M.diag_m[l] = reinterpret_cast<double*>(take(nl * 8));
			L.b = reinterpret_cast<double2*>(take(nl * 16));
			L.x = reinterpret_cast<double2*>(take(nl * 16));
			L.xo = reinterpret_cast<double2*>(take(nl * 16));
		}
		L.wh = M.wh_m[l];
		L.wv = M.wv_m[l];
		L.diag = M.diag_m[l];
	}
	M.omega = 0.8;
	M.kappa = 1.8;
	M.coarse_sweeps = 8;
}

namespace
{
// Workgroups of the chunk-walking kernels: a multiple of 8 (one band per XCD), <= 1024.
unsigned tvf_grid(int n)
{
	const int chunks = (n + 255) / 256;
	const int perBand = (chunks + 7) / 8;
	return 8u * static_cast<unsigned>(std::min(perBand, 128));
}
}  // namespace

int launch_tvf_prepare(const TvfArgs& A, const float* d_field, const int* d_fixed, int n_fixed, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (hipMemsetAsync(A.scal, 0, 256, s) != hipSuccess)
	{
		return -2;
	}
	const unsigned G = tvf_grid(A.n);
	hipLaunchKernelGGL(k_tvf_prepare, dim3(G), dim3(256), 0, s, A, reinterpret_cast<const float2*>(d_field));
	hipLaunchKernelGGL((k_tvf_reduce<1, 0>), dim3(1), dim3(256), 0, s, A.partials, static_cast<int>(G),
					   A.scal + kTvfNorm, 1);
	if (n_fixed > 0)
	{
		hipLaunchKernelGGL(k_tvf_mark_fixed, dim3((n_fixed + 255) / 256), dim3(256), 0, s, A, d_fixed, n_fixed);
	}
	return check_launch();
}

int launch_tvf_linearize(const TvfArgs& A, const double2* X, int first, int cost_only, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const unsigned G = tvf_grid(A.n);
	hipLaunchKernelGGL(k_tvf_linearize, dim3(G), dim3(256), 0, s, A, X, first, cost_only);
	// cost only: the |x|^2 and max |g| slots of the current point stay as they are
	if (cost_only)
	{
		hipLaunchKernelGGL((k_tvf_reduce<3, 1>), dim3(1), dim3(256), 0, s, A.partials, static_cast<int>(G),
						   A.scal + 20, 0);
	}
	else
	{
		hipLaunchKernelGGL((k_tvf_reduce<3, 1>), dim3(1), dim3(256), 0, s, A.partials, static_cast<int>(G),
						   A.scal + kTvfCost, 0);
	}
	return check_launch();
}

namespace
{
// z = M^-1 r by one V(1,1) cycle; the last kernel leaves the r'z partials for the CG.
void tvf_mg_vcycle(const TvfArgs& A, const TvfMg& M, hipStream_t s)
{
	const int L = M.levels;
	for (int l = 0; l + 1 < L; ++l)
	{
		const TvfLevel& f = M.lv[l];
		const TvfLevel& c = M.lv[l + 1];
		const int nc = c.w * c.h;
		hipLaunchKernelGGL(k_mg_down, dim3((nc + 255) / 256), dim3(256), 0, s, f, c.w, c.h, c.b, M.omega);
	}
	hipLaunchKernelGGL(k_mg_coarse, dim3(1), dim3(256), 0, s, M.lv[L - 1], M.omega, M.coarse_sweeps);
	for (int l = L - 2; l >= 0; --l)
	{
		const TvfLevel& f = M.lv[l];
		const TvfLevel& c = M.lv[l + 1];
		hipLaunchKernelGGL(k_mg_up, dim3(tvf_grid(f.w * f.h)), dim3(256), 0, s, f, c.xo, c.w, M.omega, M.kappa,
						   l == 0 ? A.partials_rz : nullptr, l == 0 ? A.mask : nullptr);
	}
}
}  // namespace

// The hierarchy of the operator cg_init just defined (weights of this linearisation, damping of
// this radius), then the first V-cycle (z and r'z of CG iteration 0).
int launch_tvf_mg_build(const TvfArgs& A, const TvfMg& M, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (M.levels < 2)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_mg_mask0, dim3(tvf_grid(A.n)), dim3(256), 0, s, A, M.wh_m[0], M.wv_m[0]);
	for (int l = 0; l + 1 < M.levels; ++l)
	{
		const TvfLevel& c = M.lv[l + 1];
		const int nc = c.w * c.h;
		hipLaunchKernelGGL(k_mg_coarsen, dim3((nc + 255) / 256), dim3(256), 0, s, M.lv[l], c, M.wh_m[l + 1],
						   M.wv_m[l + 1], M.diag_m[l + 1]);
	}
	tvf_mg_vcycle(A, M, s);
	return check_launch();
}

int launch_tvf_cg_init(const TvfArgs& A, const TvfMg& M, double radius, void* stream)
{
	hipLaunchKernelGGL(k_tvf_cg_init, dim3(tvf_grid(A.n)), dim3(256), 0, static_cast<hipStream_t>(stream), A, radius,
					   M.levels >= 2 ? 1 : 0);
	if (check_launch())
	{
		return -2;
	}
	return launch_tvf_mg_build(A, M, stream);
}

int launch_tvf_cg_iters(const TvfArgs& A, const TvfMg& M, int first_iter, int iters, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const unsigned G = tvf_grid(A.n);
	const int mg = M.levels >= 2 ? 1 : 0;
	for (int k = first_iter; k < first_iter + iters; ++k)
	{
		const double2* pOld = (k & 1) ? A.p1 : A.p0;
		double2* pNew = (k & 1) ? A.p0 : A.p1;
		hipLaunchKernelGGL(k_tvf_cg_apply, dim3(G), dim3(256), 0, s, A, pOld, pNew, k);
		hipLaunchKernelGGL(k_tvf_cg_update, dim3(G), dim3(256), 0, s, A, pNew, k, mg);
		if (mg)
		{
			tvf_mg_vcycle(A, M, s);
		}
	}
	return check_launch();
}

int launch_tvf_model(const TvfArgs& A, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const unsigned G = tvf_grid(A.n);
	hipLaunchKernelGGL(k_tvf_model, dim3(G), dim3(256), 0, s, A);
	hipLaunchKernelGGL((k_tvf_reduce<3, 0>), dim3(1), dim3(256), 0, s, A.partials, static_cast<int>(G),
					   A.scal + kTvfYg, 0);
	return check_launch();
}

int launch_tvf_store(const TvfArgs& A, const double2* X, float* d_field, void* stream)
{
	const unsigned blocks = static_cast<unsigned>((A.n + 255) / 256);
	hipLaunchKernelGGL(k_tvf_store, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), A.n, X,
					   reinterpret_cast<float2*>(d_field));
	return check_launch();
}

namespace
{
size_t optimizer_lds_bytes(int maxPixels)
{
	return (128 + static_cast<size_t>(maxPixels) * 6) * sizeof(double);
}
}  // namespace

int launch_optimizer_eval(const OptLaunch& L, void* stream)
{
	if (L.n_patches == 0)
	{
		return 0;
	}
	const size_t lds = optimizer_lds_bytes(L.max_pixels);
	if (lds > 160 * 1024 - 512 || allow_big_lds(k_optimizer_eval, lds))
	{
		return -2;
	}
	hipLaunchKernelGGL(k_optimizer_eval, dim3(L.n_patches), dim3(256), lds, static_cast<hipStream_t>(stream),
					   L.d_grid, L.img_w, L.img_h, L.d_patches, L.d_nabla, L.d_x, L.d_res, L.d_jac_pose,
					   L.d_jac_flow);
	return check_launch();
}

int launch_optimizer_cost_map(const OptLaunch& L, const double* d_xcells, int cells, double* d_out, void* stream)
{
	if (L.n_patches == 0 || cells == 0)
	{
		return 0;
	}
	const size_t lds = optimizer_lds_bytes(L.max_pixels);
	if (lds > 160 * 1024 - 512 || allow_big_lds(k_optimizer_cost_map, lds))
	{
		return -2;
	}
	hipLaunchKernelGGL(k_optimizer_cost_map, dim3(cells, L.n_patches), dim3(256), lds, static_cast<hipStream_t>(stream),
					   L.d_grid, L.img_w, L.img_h, L.d_patches, L.d_nabla, d_xcells, d_out);
	return check_launch();
}

int launch_optimizer_solve(const OptLaunch& L, void* stream)
{
	if (L.n_patches == 0)
	{
		return 0;
	}
	const size_t lds = optimizer_lds_bytes(L.max_pixels);
	if (lds > 160 * 1024 - 512 || allow_big_lds(k_optimizer_solve, lds))
	{
		return -2;
	}
	// measured (25x25 patches): 256 lanes best up to ~100 patches (0.27 / 0.38 ms for 1 / 100), 128
	// lanes at 1000 (1.13 vs 1.32 ms); 384+ lanes slower everywhere.  EBO_OPT_BLOCK for A/B.
	int block = L.n_patches >= 512 ? 128 : 256;
	if (const char* v = ab_env("EBO_OPT_BLOCK"))
	{
		block = std::min(std::max((std::atoi(v) / 64) * 64, 64), 256);
	}
	hipLaunchKernelGGL(k_optimizer_solve, dim3(L.n_patches), dim3(block), lds, static_cast<hipStream_t>(stream),
					   L.d_grid, L.img_w, L.img_h, L.d_patches, L.d_nabla, L.d_x, L.d_stats, L.huber, L.s,
					   ab_env("EBO_OPT_NO_SPECULATE") ? 0 : 1);
	return check_launch();
}

int launch_optimizer_normalize(const OptPatch* d_patches, int n, const double* d_in, double* d_out, void* stream)
{
	if (n == 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_optimizer_normalize, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), d_patches,
					   d_in, d_out);
	return check_launch();
}

int launch_optimizer_interleave(const double* d_gx, const double* d_gy, size_t n, double2* d_grid, void* stream)
{
	hipLaunchKernelGGL(k_optimizer_interleave, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
					   static_cast<hipStream_t>(stream), d_gx, d_gy, n, d_grid);
	return check_launch();
}

int launch_estimate_num_events(const double2* d_grid, int w, int h, int n, const double* d_rects, const double* d_poses,
								const double* d_flows, double* d_sums, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_estimate_num_events, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), d_grid, w, h, n,
					   d_rects, d_poses, d_flows, d_sums);
	return check_launch();
}

int launch_patch_warp_image(const double2* d_grid, int w, int h, int n, const double* d_rects, const double* d_poses,
							const double* d_flows, const int* d_skip, const size_t* d_offsets, double* d_out, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_patch_warp_image, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), d_grid, w, h, n, d_rects,
					   d_poses, d_flows, d_skip, d_offsets, d_out);
	return check_launch();
}

template <class Rec>
static int launch_bucket_t(const BucketLaunch& L, Rec raw, hipStream_t s)
{
	const int nUnits = L.n_windows * (L.P + 1);
	const int w0 = L.w0, w1 = L.w1 < 0 ? L.n_windows : L.w1;
	const int nw = w1 - w0;
	if (w0 == 0)
	{
		hipLaunchKernelGGL(k_bucket_init, dim3((nUnits + 255) / 256), dim3(256), 0, s, L.d_cnt, L.d_tmin,
						   L.d_tmax, nUnits, L.d_flag);
		if (check_launch())
		{
			return -2;
		}
	}
	if (nw <= 0)
	{
		return 0;
	}
	const size_t lds = static_cast<size_t>(L.P + 1) * (2 * sizeof(long long) + sizeof(int)) + 8;
	if (L.max_chunks > 0)
	{
		if (allow_big_lds(k_bucket_count<Rec>, lds))
		{
			return -2;
		}
		hipLaunchKernelGGL(k_bucket_count<Rec>, dim3(L.max_chunks, nw), dim3(256), lds, s, raw,
						   L.d_offsets, w0, L.P, L.d_cnt, L.d_tmin, L.d_tmax, L.d_flag, L.d_chunk_hist, L.chunk_events, L.c);
		if (check_launch())
		{
			return -2;
		}
	}
	hipLaunchKernelGGL(k_bucket_scan<Rec>, dim3(nw), dim3(256), 0, s, raw, L.d_offsets, w0,
					   L.n_windows, L.P, L.d_cnt, L.d_tmin, L.d_tmax, L.min_events, L.d_units,
					   L.d_unit_tref, L.d_unit_maxdt, L.d_win_tref, L.d_flag, L.c);
	if (check_launch())
	{
		return -2;
	}
	if (L.max_chunks > 0)
	{
		hipLaunchKernelGGL(k_bucket_chunk_scan, dim3((L.P + 1 + 255) / 256, nw), dim3(256), 0, s, L.d_offsets, w0, L.P,
						   L.max_chunks, L.chunk_events, L.d_chunk_hist);
		if (check_launch())
		{
			return -2;
		}
		const size_t curLds = static_cast<size_t>(L.P + 1) * sizeof(unsigned int);
		if (allow_big_lds(k_bucket_scatter<Rec>, curLds))
		{
			return -2;
		}
		hipLaunchKernelGGL(k_bucket_scatter<Rec>, dim3(L.max_chunks, nw), dim3(64), curLds, s, raw,
						   L.d_offsets, w0, L.P, L.d_chunk_hist, L.d_units, L.d_unit_tref, L.d_win_tref, L.d_packed,
						   L.d_flag, L.chunk_events, L.c);
		if (check_launch())
		{
			return -2;
		}
		const size_t sortLds = static_cast<size_t>(kSortMax) * sizeof(unsigned long long);
		if (allow_big_lds(k_bucket_canon, sortLds))
		{
			return -2;
		}
		hipLaunchKernelGGL(k_bucket_canon, dim3(nw * (L.P + 1)), dim3(256), sortLds, s,
						   L.d_units + static_cast<size_t>(w0) * (L.P + 1), L.d_packed);
	}
	return check_launch();
}

// the same record read through the rectification table (ebo_camera.inc)
template <class Rec>
static int launch_bucket_rectified(const BucketLaunch& L, Rec raw, hipStream_t s)
{
	Rectified<Rec> r;
	r.inner = raw;
	r.lut = static_cast<const short2*>(L.d_rectify);
	r.w = L.c.image_w;
	r.h = L.c.image_h;
	return launch_bucket_t(L, r, s);
}

int launch_bucket(const BucketLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.compact)
	{
		Rec8 r;
		r.p = static_cast<const uint2*>(L.d_raw);
		r.tbase = L.d_tbase;
		return L.d_rectify ? launch_bucket_rectified(L, r, s) : launch_bucket_t(L, r, s);
	}
	Rec24 r;
	r.p = static_cast<const RawEvent*>(L.d_raw);
	return L.d_rectify ? launch_bucket_rectified(L, r, s) : launch_bucket_t(L, r, s);
}

int launch_camera_unproject(const CameraConsts& k, int n, const double* d_uv, double* d_bearing, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_camera_unproject, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), k, n, d_uv,
					   d_bearing);
	return check_launch();
}

int launch_camera_project(const CameraConsts& k, int n, const double* d_xyz, double* d_uv, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_camera_project, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), k, n, d_xyz,
					   d_uv);
	return check_launch();
}

int launch_rectify_fit(const CameraConsts& k, int w, int h, double* d_extremes, int* d_bad, void* stream)
{
	hipLaunchKernelGGL(k_rectify_fit, dim3(1), dim3(kFitThreads), 0, static_cast<hipStream_t>(stream), k, w, h, d_extremes,
					   d_bad);
	return check_launch();
}

int launch_rectify_image(const CameraConsts& k, const RectifiedConsts& r, int w, int h, const uint8_t* d_img, uint8_t* d_out,
						 double* d_src, void* stream)
{
	const dim3 grid((w + kRectTileW - 1) / kRectTileW, (h + kRectTileH - 1) / kRectTileH);
	hipLaunchKernelGGL(k_rectify_image, grid, dim3(kRectTileW, kRectTileH), 0, static_cast<hipStream_t>(stream), k, r, w, h,
					   d_img, d_out, d_src);
	return check_launch();
}

int launch_rectify_map(const CameraConsts& k, const RectifiedConsts& r, int w, int h, double* d_map, void* d_lut, int* d_bad,
					   void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (hipMemsetAsync(d_bad, 0, sizeof(int), s) != hipSuccess)
	{
		return -2;
	}
	hipLaunchKernelGGL(k_rectify_map, dim3((w * h + 255) / 256), dim3(256), 0, s, k, r, w, h, d_map,
					   static_cast<short2*>(d_lut), d_bad);
	return check_launch();
}

// two-view geometry (ebo_twoview.inc)
int launch_tv_hypotheses(int n_pairs, int H, const int* d_offsets, const double* d_f1, const double* d_f2, uint64_t seed,
						 double* d_models, int* d_valid, int* d_samples, void* stream)
{
	const long long total = static_cast<long long>(n_pairs) * H;
	if (total <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_tv_hypotheses, dim3(static_cast<unsigned int>((total + kTvGroups - 1) / kTvGroups)), dim3(256), 0,
					   static_cast<hipStream_t>(stream), n_pairs, H, d_offsets, d_f1, d_f2, static_cast<unsigned long long>(seed),
					   d_models, d_valid, d_samples);
	return check_launch();
}

int launch_tv_triangulate(int n_poses, const double* d_poses, int n, const int* d_pose_pair, const double* d_f1,
						  const double* d_f2, double* d_points, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_tv_triangulate, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), n_poses, d_poses, n,
					   d_pose_pair, d_f1, d_f2, d_points);
	return check_launch();
}

int launch_tv_epipolar(const double* model12, int n, const double* d_f1, const double* d_f2, double threshold,
					   unsigned char* d_flags, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	TvModelArg m;
	std::copy(model12, model12 + 12, m.m);
	hipLaunchKernelGGL(k_tv_epipolar, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), m, n, d_f1, d_f2,
					   threshold, d_flags);
	return check_launch();
}

// absolute pose (ebo_abspose.inc)
int launch_ap_hypotheses(int n_frames, int H, const int* d_offsets, const double* d_f, const double* d_points, uint64_t seed,
						 double* d_models, int* d_valid, int* d_samples, void* stream)
{
	const long long total = static_cast<long long>(n_frames) * H;
	if (total <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_ap_hypotheses, dim3(static_cast<unsigned int>((total + kApBlock - 1) / kApBlock)), dim3(kApBlock), 0,
					   static_cast<hipStream_t>(stream), n_frames, H, d_offsets, d_f, d_points, static_cast<unsigned long long>(seed),
					   d_models, d_valid, d_samples);
	return check_launch();
}

// what the two RANSAC paths share (ebo_ransac.inc)
int launch_ransac_count(RansacKind kind, int n_groups, int H, int max_n, const int* d_offsets, const double* d_a, const double* d_b,
						const double* d_models, const int* d_valid, double threshold, int* d_counts, void* stream)
{
	const bool tv = kind == RansacKind::kTwoView;
	if (n_groups <= 0 || H <= 0 || max_n < (tv ? TvProblem::kSample : ApProblem::kSample))
	{
		return 0;
	}
	hipLaunchKernelGGL(tv ? k_ransac_count<TvProblem> : k_ransac_count<ApProblem>,
					   dim3((H + kRansacHypChunk - 1) / kRansacHypChunk, n_groups, (max_n + kRansacTile - 1) / kRansacTile), dim3(256), 0,
					   static_cast<hipStream_t>(stream), H, d_offsets, d_a, d_b, d_models, d_valid, threshold, d_counts);
	return check_launch();
}

int launch_ransac_winner_flags(RansacKind kind, int n_groups, int H, int max_n, const int* d_offsets, const double* d_a,
							   const double* d_b, const double* d_models, const int* d_valid, const int* d_winner, double threshold,
							   unsigned char* d_flags, double* d_win_models, void* stream)
{
	if (n_groups <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(kind == RansacKind::kTwoView ? k_ransac_winner_flags<TvProblem> : k_ransac_winner_flags<ApProblem>,
					   dim3(max_n > 0 ? (max_n + 255) / 256 : 1, n_groups), dim3(256), 0, static_cast<hipStream_t>(stream), H, d_offsets,
					   d_a, d_b, d_models, d_valid, d_winner, threshold, d_flags, d_win_models);
	return check_launch();
}

int launch_ransac_scores(RansacKind kind, const double* model12, int n, const double* d_a, const double* d_b, double threshold,
						 double* d_scores, unsigned char* d_flags, void* stream)
{
	if (n <= 0)
	{
		return 0;
	}
	TvModelArg m;
	std::copy(model12, model12 + 12, m.m);
	hipLaunchKernelGGL(kind == RansacKind::kTwoView ? k_ransac_scores<TvProblem> : k_ransac_scores<ApProblem>, dim3((n + 255) / 256),
					   dim3(256), 0, static_cast<hipStream_t>(stream), m, n, d_a, d_b, threshold, d_scores, d_flags);
	return check_launch();
}

// bundle adjustment (ebo_bundle.inc)
int launch_bundle_adjust(int n_problems, int max_frames, const BaTables& t, const ebo_camera& cam, double huber, int fix_points,
						 const ebo_solver_opts& o, ebo_summary* d_summaries, double* d_trace, void* stream)
{
	if (n_problems <= 0)
	{
		return 0;
	}
	const size_t lds = sizeof(double) * (ba_reduced_doubles(max_frames) + 1);
	if (allow_big_lds(k_bundle_adjust, lds + 8 * 1024))
	{
		return -2;
	}
	hipLaunchKernelGGL(k_bundle_adjust, dim3(n_problems), dim3(kBaLanes), lds, static_cast<hipStream_t>(stream), t, cam, huber,
					   fix_points, o, d_summaries, d_trace);
	return check_launch();
}

// relative-pose refinement (ebo_relpose.inc): one wave per pair
int launch_relpose_refine(int n_pairs, const int* d_offsets, const int* d_n_inliers, const double* d_f1, const double* d_f2,
						  const int* d_inlier_idx, double* d_models, double* d_work, const ebo_solver_opts& o, ebo_summary* d_summaries,
						  double* d_trace, void* stream)
{
	if (n_pairs <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_relpose_refine, dim3(n_pairs), dim3(kRpLanes), 0, static_cast<hipStream_t>(stream), d_offsets, d_n_inliers, d_f1,
					   d_f2, d_inlier_idx, d_models, d_work, o, d_summaries, d_trace);
	return check_launch();
}

// trajectory alignment (ebo_align.inc): one wave per segment
int launch_align_sim3(int n_points, const double* d_data, const double* d_model, int n_segments, const int* d_seg_begin,
					  const int* d_seg_end, int fix_scale, ebo_align_result* d_results, void* stream)
{
	if (n_segments <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_align_sim3, dim3(n_segments), dim3(kRpLanes), 0, static_cast<hipStream_t>(stream), n_points, d_data, d_model,
					   d_seg_begin, d_seg_end, fix_scale, d_results);
	return check_launch();
}

// relative pose error (ebo_rpe.inc): one wave per (segment, delta) unit
int launch_trajectory_rpe(int n_poses, const double* d_gt, const double* d_est, int n_segments, const int* d_seg_begin,
						  const int* d_seg_end, const double* d_seg_scale, int n_deltas, const int* d_deltas, ebo_rpe_result* d_results,
						  void* stream)
{
	if (n_segments <= 0 || n_deltas <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_trajectory_rpe, dim3(n_segments * n_deltas), dim3(kRpLanes), 0, static_cast<hipStream_t>(stream), n_poses, d_gt,
					   d_est, d_seg_begin, d_seg_end, d_seg_scale, n_deltas, d_deltas, d_results);
	return check_launch();
}

// landmark maintenance (ebo_landmark.inc): a group of `lanes` lanes per landmark, 64 / lanes landmarks per wave
template <bool SOLVE, int W>
int launch_landmarks_as(int n_poses, const double* d_poses, int n_landmarks, const int* d_offsets, const int* d_obs_pose,
						const double* d_obs_f, const double* d_points, const LmParamsArg& prm, ebo_landmark_result* d_results,
						double* d_scores, uint8_t* d_flags, void* stream)
{
	constexpr int kGroups = 64 / W;
	hipLaunchKernelGGL((k_landmarks<SOLVE, W>), dim3((n_landmarks + kGroups - 1) / kGroups), dim3(64), 0, static_cast<hipStream_t>(stream),
					   n_poses, d_poses, n_landmarks, d_offsets, d_obs_pose, d_obs_f, d_points, prm, d_results, d_scores, d_flags);
	return check_launch();
}

int launch_landmarks(int solve, int lanes, int n_poses, const double* d_poses, int n_landmarks, const int* d_offsets,
					 const int* d_obs_pose, const double* d_obs_f, const double* d_points, const ebo_landmark_params* params,
					 ebo_landmark_result* d_results, double* d_scores, uint8_t* d_flags, void* stream)
{
	if (n_landmarks <= 0)
	{
		return 0;
	}
	const LmParamsArg prm = {params->threshold, params->min_parallax, params->min_inliers, params->max_hypotheses, params->seed};
	if (solve)
	{
		return lanes == 16 ? launch_landmarks_as<true, 16>(n_poses, d_poses, n_landmarks, d_offsets, d_obs_pose, d_obs_f, d_points, prm,
														   d_results, d_scores, d_flags, stream)
						   : launch_landmarks_as<true, 64>(n_poses, d_poses, n_landmarks, d_offsets, d_obs_pose, d_obs_f, d_points, prm,
														   d_results, d_scores, d_flags, stream);
	}
	return lanes == 16 ? launch_landmarks_as<false, 16>(n_poses, d_poses, n_landmarks, d_offsets, d_obs_pose, d_obs_f, d_points, prm,
														d_results, d_scores, d_flags, stream)
					   : launch_landmarks_as<false, 64>(n_poses, d_poses, n_landmarks, d_offsets, d_obs_pose, d_obs_f, d_points, prm,
														d_results, d_scores, d_flags, stream);
}

// rotational contrast maximisation (ebo_rotation.inc): one chunk of windows per call
int launch_rot_votes(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					 const RotScratch& s, double* d_F, void* stream)
{
	if (L.n <= 0)
	{
		return 0;
	}
	hipStream_t st = static_cast<hipStream_t>(stream);
	const size_t np = static_cast<size_t>(k.w) * k.h;
	if (hipMemsetAsync(s.imgX, 0, static_cast<size_t>(L.n) * np * sizeof(unsigned long long), st) != hipSuccess)
	{
		return -2;
	}
	hipLaunchKernelGGL(k_rot_vote, dim3(k.P, L.n), dim3(kRotBlock), 0, st, d_events, d_units, L, k, d_omegas,
					   static_cast<unsigned long long*>(s.imgX));
	if (d_F)
	{
		hipLaunchKernelGGL(k_rot_scale, dim3(rot_blocks(k.w, k.h), L.n), dim3(kRotBlock), 0, st, k, static_cast<const long long*>(s.imgX), d_F);
	}
	return check_launch();
}

int launch_rot_eval(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					const RotScratch& s, double* d_r, double* d_g, void* stream)
{
	if (L.n <= 0)
	{
		return 0;
	}
	if (launch_rot_votes(d_events, d_units, L, k, d_omegas, s, nullptr, stream))
	{
		return -2;
	}
	hipStream_t st = static_cast<hipStream_t>(stream);
	const int nb = rot_blocks(k.w, k.h);
	const dim3 px(nb, L.n), blk(kRotBlock);
	hipLaunchKernelGGL((k_rot_hpass<false, true>), px, blk, 0, st, k, static_cast<const void*>(s.imgX), static_cast<const double*>(nullptr),
					   s.imgY, static_cast<double*>(nullptr));
	hipLaunchKernelGGL((k_rot_vpass<true>), px, blk, 0, st, k, static_cast<const double*>(s.imgY), s.imgZ, s.partB);
	hipLaunchKernelGGL(k_rot_mean, dim3(L.n), dim3(64), 0, st, k, nb, static_cast<const double*>(s.partB), s.mu);
	if (d_g)
	{
		hipLaunchKernelGGL((k_rot_hpass<true, true>), px, blk, 0, st, k, static_cast<const void*>(s.imgZ), static_cast<const double*>(s.mu),
						   static_cast<double*>(s.imgX), s.partV);
		hipLaunchKernelGGL((k_rot_vpass<false>), px, blk, 0, st, k, static_cast<const double*>(s.imgX), s.imgY, static_cast<double*>(nullptr));
		hipLaunchKernelGGL(k_rot_gather, dim3(k.P, L.n), blk, 0, st, d_events, d_units, L, k, d_omegas, static_cast<const double*>(s.imgY),
						   s.partG);
	}
	else
	{
		hipLaunchKernelGGL((k_rot_hpass<true, false>), px, blk, 0, st, k, static_cast<const void*>(s.imgZ), static_cast<const double*>(s.mu),
						   static_cast<double*>(nullptr), s.partV);
	}
	hipLaunchKernelGGL(k_rot_finish, dim3(L.n), dim3(64), 0, st, L, k, nb, static_cast<const double*>(s.partV),
					   static_cast<const double*>(s.partG), d_r, d_g);
	return check_launch();
}

int launch_rot_images(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					  const RotScratch& s, double* d_B, void* stream)
{
	if (L.n <= 0)
	{
		return 0;
	}
	if (launch_rot_votes(d_events, d_units, L, k, d_omegas, s, nullptr, stream))
	{
		return -2;
	}
	hipStream_t st = static_cast<hipStream_t>(stream);
	const dim3 px(rot_blocks(k.w, k.h), L.n), blk(kRotBlock);
	hipLaunchKernelGGL((k_rot_hpass<false, true>), px, blk, 0, st, k, static_cast<const void*>(s.imgX), static_cast<const double*>(nullptr),
					   s.imgY, static_cast<double*>(nullptr));
	hipLaunchKernelGGL((k_rot_vpass<false>), px, blk, 0, st, k, static_cast<const double*>(s.imgY), d_B, static_cast<double*>(nullptr));
	return check_launch();
}

// pose from events against a map (ebo_maptrack.inc): one workgroup per unit
int launch_map_track(const MtCall& k, int n_units, const int* d_unit_image, double* d_poses, const ebo_solver_opts& o,
					 ebo_map_track_result* d_results, double* d_trace, void* stream)
{
	if (n_units <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_map_track, dim3(n_units), dim3(kMtLanes), 0, static_cast<hipStream_t>(stream), k, d_unit_image, d_poses, o,
					   d_results, d_trace);
	return check_launch();
}

// depth from events by space sweep (ebo_depth.inc): the votes of one chunk of windows
int launch_dsi_vote(const uint64_t* d_events, const Unit* d_units, int P, const DsiWindows& L, const DsiConsts& k, const DsiPose* d_poses,
					const double* d_z, uint32_t* d_H, void* stream)
{
	if (L.n <= 0 || k.planes < 1)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_dsi_vote, dim3(P, L.n, (k.nz + k.planes - 1) / k.planes), dim3(kDsiBlock), 0, static_cast<hipStream_t>(stream),
					   d_events, d_units, L, k, d_poses, d_z, d_H);
	return check_launch();
}

int launch_dsi_extract(const DsiConsts& k, int r, long long off, int m, const double* d_z, const uint32_t* d_H, const DsiScratch& s,
					   int max_points, void* stream)
{
	hipStream_t st = static_cast<hipStream_t>(stream);
	const int nb = dsi_blocks(k.w, k.h);
	const dim3 px(nb), blk(kDsiBlock);
	hipLaunchKernelGGL(k_dsi_argmax, px, blk, 0, st, k, d_H, s.conf, s.kbest);
	hipLaunchKernelGGL(k_dsi_keep, px, blk, 0, st, k, r, off, static_cast<const unsigned int*>(s.conf), s.keep);
	hipLaunchKernelGGL(k_dsi_median, px, blk, 0, st, k, m, static_cast<const int*>(s.kbest), static_cast<const unsigned char*>(s.keep), d_z,
					   s.index, s.depth);
	hipLaunchKernelGGL(k_dsi_count, px, blk, 0, st, k, static_cast<const int*>(s.index), s.blockCount);
	hipLaunchKernelGGL(k_dsi_scan, dim3(1), blk, 0, st, nb, s.blockCount);
	if (s.points && max_points > 0)
	{
		hipLaunchKernelGGL(k_dsi_points, px, blk, 0, st, k, static_cast<const int*>(s.index), d_z, static_cast<const int*>(s.blockCount),
						   max_points, s.points);
	}
	return check_launch();
}

// track evaluation (ebo_trackerr.inc): one wave per (track, threshold) unit
int launch_track_errors(int n_est, int n_gt, int n_tracks, const int* d_est_off, const int64_t* d_est_t, const double* d_est_xy,
						const int* d_gt_off, const int64_t* d_gt_t, const double* d_gt_xy, int n_taus, const double* d_taus,
						ebo_track_error_result* d_results, double* d_sample_err, void* stream)
{
	if (n_tracks <= 0 || n_taus <= 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_track_errors, dim3(n_tracks * n_taus), dim3(kRpLanes), 0, static_cast<hipStream_t>(stream), n_est, n_gt, d_est_off,
					   d_est_t, d_est_xy, d_gt_off, d_gt_t, d_gt_xy, n_taus, d_taus, d_results, d_sample_err);
	return check_launch();
}

int launch_lds_rate(int atomic, int blocks, int iters, double* d_sink, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (atomic)
	{
		hipLaunchKernelGGL(k_lds_rate<true>, dim3(blocks), dim3(256), 0, s, d_sink, iters);
	}
	else
	{
		hipLaunchKernelGGL(k_lds_rate<false>, dim3(blocks), dim3(256), 0, s, d_sink, iters);
	}
	return check_launch();
}

int launch_stream_yardstick(const uint64_t* d_events, size_t n_events, double* d_image, size_t n_pixels, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	hipLaunchKernelGGL(k_stream_yardstick, dim3(2048), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_events), n_events / 2,
					   reinterpret_cast<double2*>(d_image), n_pixels / 2);
	return check_launch();
}

int launch_count_shard(const uint64_t* d_events, const Unit* d_units, int n_units, int units_per_window,
					   const BandUnit* d_table, const double* d_flows, double* d_image, const EvalConsts& c, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (n_units == 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_count_shard, dim3(n_units), dim3(256), 0, s, d_events, d_units, units_per_window, d_table,
					   d_flows, d_image, c);
	return check_launch();
}

int launch_count_band(const BandLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const int bandRows = L.band1 - L.band0;
	if (L.n_windows <= 0 || L.per <= 0 || bandRows <= 0)
	{
		return 0;
	}
	// tiles of <= 15360 counters (60 KB) + the selection list: two workgroups per CU; about 160 columns wide, so
	// that a tile's units are few (events are re-read once per tile their reach touches)
	const int W = L.c.image_w;
	const int tilesX = std::max(1, (W + 159) / 160);
	int tw = (W + tilesX - 1) / tilesX;
	const int thMax = std::max(1, 15360 / tw);
	const int tilesY = (bandRows + thMax - 1) / thMax;
	const int th = (bandRows + tilesY - 1) / tilesY;
	BandGeom g;
	g.band0 = L.band0;
	g.own0 = L.own0;
	g.own1 = L.own1;
	g.band1 = L.band1;
	g.tileW = tw;
	g.tileH = th;
	g.tilesX = tilesX;
	g.tilesY = tilesY;
	const size_t lds = (static_cast<size_t>(tw) * th + 1 + static_cast<size_t>(L.per)) * sizeof(int);
	if (lds > 160 * 1024 || allow_big_lds(k_count_band, lds))
	{
		return -2;
	}
	hipLaunchKernelGGL(k_count_band, dim3(tilesX * tilesY, L.n_windows), dim3(512), lds, s, L.d_events, L.d_units, L.d_band_units,
					   L.per, L.d_flows, g, L.d_top, L.d_own, L.d_bottom, L.d_escaped, L.c);
	return check_launch();
}

int launch_band_finish(const unsigned int* d_own, const unsigned int* d_from_above, const unsigned int* d_from_below,
					   int own_rows, int recv_above, int recv_below, int W, int n_windows, double* d_image, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t n = static_cast<size_t>(n_windows) * own_rows * W;
	if (n == 0)
	{
		return 0;
	}
	const int blocks = static_cast<int>(std::min<size_t>((n + 255) / 256, 4096));
	hipLaunchKernelGGL(k_band_finish, dim3(blocks), dim3(256), 0, s, d_own, d_from_above, d_from_below, own_rows, recv_above,
					   recv_below, W, n, d_image);
	return check_launch();
}

int launch_eval_edge(const EdgeLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.n_units == 0)
	{
		return 0;
	}
	const bool narrow = L.block <= 256 && !L.wide_kernel;  // MAXT 256 (two workgroups per CU, persistent) or 768 (one workgroup per item)
	LiveWindows live = L.live;
	if (L.flow_sets != 1)
	{
		live.n = 0;
	}
	const int nItemsX = live.n > 0 ? live.n * live.upw : L.n_units;
	if (narrow)
	{
		using EdgeKern = decltype(&k_eval_edge<true, true, 256>);
		EdgeKern edgeKern = L.alias_lds ? (L.want_jac ? k_eval_edge<true, true, 256> : k_eval_edge<true, false, 256>)
										: (L.want_jac ? k_eval_edge<false, true, 256> : k_eval_edge<false, false, 256>);
		if (allow_big_lds(edgeKern, L.lds_bytes))
		{
			return -2;
		}
		EdgeKArgs ka;
		ka.events = L.d_events;
		ka.units = L.d_units;
		ka.flows = L.d_flows;
		ka.wantJac = L.want_jac;
		ka.capPx = L.cap_px;
		ka.fdStep = L.fd_step;
		ka.scratch = L.d_scratch;
		ka.scratchStride = L.scratch_stride;
		ka.sets = L.d_sets;
		ka.out = L.d_out;
		ka.c = L.c;
		ka.ec = L.ec;
		ka.modes = L.flow_sets == 1 ? L.d_modes : nullptr;
		ka.live = live;
		ka.nItemsX = nItemsX;
		ka.nSets = L.flow_sets;
		ka.itemList = nullptr;
		ka.itemCount = nullptr;
		ka.bbox = nullptr;
		if (L.compact.list_cap > 0 && L.alias_lds && L.flow_sets == 1)
		{
			// Two launches (round 5).  First every unit on the COMPACT layout, three 256-lane workgroups per CU (the
			// 168-VGPR instantiation); a unit whose box does not fit goes on the deferred list.  Then the deferred
			// units on the 20 B layout, two per CU, persistent workgroups that read the list's length on the device.
			using WideKern = decltype(&k_eval_edge_wg<true, true, 768>);
			int4* const bbox = static_cast<int4*>(L.compact.bbox);
			WideKern wide = bbox ? (L.want_jac ? k_eval_edge_wg<true, true, 768, true> : k_eval_edge_wg<true, false, 768, true>)
								 : (L.want_jac ? k_eval_edge_wg<true, true, 768> : k_eval_edge_wg<true, false, 768>);
			if (allow_big_lds(wide, L.compact_lds_bytes))
			{
				return -2;
			}
			if (hipMemsetAsync(L.compact.defer_count, 0, sizeof(int), s) != hipSuccess)
			{
				return -2;
			}
			EdgeConsts ecCompact = L.ec;
			ecCompact.cs_stride = L.compact_table_px;  // one slot per unit, as in rounds 1-4; the most pixels a box of this launch may have
			if (bbox)
			{
				// the bounding-box pass of every unit, and the list of the second launch, in one small kernel up front
				hipLaunchKernelGGL(k_edge_classify, dim3((nItemsX + 15) / 16), dim3(1024), 0, s, L.d_events, L.d_units, L.d_flows, L.d_modes,
								   live, nItemsX, L.compact_cap_px, L.compact_table_px, L.c, bbox, L.compact.defer_list, L.compact.defer_count);
				if (check_launch())
				{
					return -2;
				}
			}
			hipLaunchKernelGGL(wide, dim3(nItemsX, 1), dim3(256), L.compact_lds_bytes, s, L.d_events, L.d_units, L.d_flows,
							   L.want_jac, L.compact_cap_px, L.fd_step, L.d_scratch, L.scratch_stride, L.d_sets, L.d_out, L.c, ecCompact,
							   L.d_modes, live, L.compact, bbox);
			if (check_launch())
			{
				return -2;
			}
			ka.itemList = L.compact.defer_list;
			ka.itemCount = L.compact.defer_count;
			ka.bbox = bbox;
		}
		const int grid = std::min(nItemsX * L.flow_sets, std::max(L.wg_slots, 1));  // persistent workgroups
		hipLaunchKernelGGL(edgeKern, dim3(grid), dim3(L.block), L.lds_bytes, s, ka);
	}
	else
	{
		using EdgeKern = decltype(&k_eval_edge_wg<true, true, 768>);
		EdgeKern edgeKern = L.alias_lds ? (L.want_jac ? k_eval_edge_wg<true, true, 768> : k_eval_edge_wg<true, false, 768>)
										: (L.want_jac ? k_eval_edge_wg<false, true, 768> : k_eval_edge_wg<false, false, 768>);
		if (allow_big_lds(edgeKern, L.lds_bytes))
		{
			return -2;
		}
		hipLaunchKernelGGL(edgeKern, dim3(nItemsX, L.flow_sets), dim3(L.block), L.lds_bytes, s, L.d_events, L.d_units, L.d_flows,
						   L.want_jac, L.cap_px, L.fd_step, L.d_scratch, L.scratch_stride, L.d_sets, L.d_out, L.c, L.ec,
						   L.flow_sets == 1 ? L.d_modes : nullptr, live, EdgeCompact(), static_cast<const int4*>(nullptr));
	}
	if (check_launch())
	{
		return -2;
	}
	if (L.flow_sets == 5)
	{
		hipLaunchKernelGGL(k_edge_central, dim3((L.n_units + 127) / 128), dim3(128), 0, s, L.d_units,
						   L.n_units, L.fd_step, L.d_sets, L.d_out);
	}
	return check_launch();
}

int launch_solve_edge(const EdgeLaunch& L, const SolveConsts& o, double* d_flows_out, int32_t* d_stats, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.n_units == 0)
	{
		return 0;
	}
	using SolveKern = decltype(&k_solve_edge<true, 256>);
	if (L.block > 512)
	{
		return -2;  // the solve's instantiations are 256 and 512 lanes (edge_launch_setup clamps EBO_EDGE_BLOCK)
	}
	const bool narrow = L.block <= 256;
	SolveKern kern = L.alias_lds ? (narrow ? k_solve_edge<true, 256> : k_solve_edge<true, 512>)
								 : (narrow ? k_solve_edge<false, 256> : k_solve_edge<false, 512>);
	if (allow_big_lds(kern, L.lds_bytes))
	{
		return -2;
	}
	hipLaunchKernelGGL(kern, dim3(L.n_units), dim3(L.block), L.lds_bytes, s, L.d_events, L.d_units, L.cap_px,
					   L.d_scratch, L.scratch_stride, d_flows_out, d_stats, L.c, L.ec, o, ab_env("EBO_SOLVE_NO_REUSE") ? 1 : 0);
	return check_launch();
}

int launch_dump_image(const EvalLaunch& L, int unit, double* d_image, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	auto kern = (L.channels == 3) ? k_dump_image<3> : k_dump_image<1>;
	if (allow_big_lds(kern, L.lds_bytes))
	{
		return -2;
	}
	hipLaunchKernelGGL(kern, dim3(1), dim3(L.block), L.lds_bytes, s, L.d_events, L.d_units, unit,
					   L.d_flows, L.tiles, d_image, L.c);
	return check_launch();
}

int launch_solve_independent(const SolveLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.n_units == 0)
	{
		return 0;
	}
	if (!L.d_order)
	{
		return -2;  // no launch without the units' order table
	}
	const bool smallExp = L.c.inv_sigsq <= 1.0 && L.c.fix_form != kFixBiasedGuard;
	auto kern = smallExp ? k_solve_independent<true> : k_solve_independent<false>;
	if (allow_big_lds(kern, L.lds_bytes))
	{
		return -2;
	}
	hipLaunchKernelGGL(kern, dim3(L.n_units), dim3(L.block), L.lds_bytes, s, L.d_events,
					   L.d_units, L.cap_doubles, L.d_flows_out, L.d_stats, L.c, L.s, ab_env("EBO_SOLVE_NO_REUSE") ? 1 : 0, L.d_order, L.d_unit_ext);
	return check_launch();
}

// Launches what plan_count_image (count_plan.h) chose; the choice itself is pinned on the CPU (tests/test_count_plan.py).
// A planned size is <= 160 KB of LDS, which gfx950 grants: a refused attribute is an error, not a reason to fall back.
int launch_count_image(const CountLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const CountPlan& p = L.plan;
	const dim3 grid(p.grid_x, p.grid_y), block(p.block);
	switch (p.kind)
	{
	case kCountTiles:
		if (allow_big_lds(k_count_tiles, p.lds))
		{
			return -2;
		}
		hipLaunchKernelGGL(k_count_tiles, grid, block, p.lds, s, L.d_events, L.d_units, L.d_unit_maxdt, L.units_per_window,
						   static_cast<const double*>(L.d_aux), p.tile_w, p.tile_h, p.tiles_x, p.tiles_y, p.tile_bytes,
						   L.n_windows, L.d_image, L.c);
		if (check_launch())
		{
			return -2;
		}
		if (p.stray)
		{
			hipLaunchKernelGGL(k_count_stray, dim3(L.n_windows), dim3(256), 0, s, L.d_events, L.d_units, L.units_per_window,
							   static_cast<const double*>(L.d_aux), L.d_image, L.c);
		}
		return check_launch();
	case kCountUnits:
	{
		auto kern = p.u16 ? k_count_units<true> : k_count_units<false>;
		if (allow_big_lds(kern, p.lds))
		{
			return -2;
		}
		hipLaunchKernelGGL(kern, grid, block, p.lds, s, L.d_events, L.d_units, L.d_unit_maxdt, L.units_per_window, L.d_aux,
						   p.rows_per_band, L.n_windows, L.d_image, L.c);
		return check_launch();
	}
	case kCountWindowLds:
	{
		auto kern = p.u16 ? (L.mode == 1 ? k_count_window_lds<true, 1> : k_count_window_lds<true, 2>)
						  : (L.mode == 1 ? k_count_window_lds<false, 1> : k_count_window_lds<false, 2>);
		if (allow_big_lds(kern, p.lds))
		{
			return -2;
		}
		hipLaunchKernelGGL(kern, grid, block, p.lds, s, L.d_events, L.d_units, L.units_per_window, L.d_aux, p.rows_per_band,
						   L.n_windows, L.d_image, L.c);
		return check_launch();
	}
	case kCountSorted:
	{
		auto count = p.u16 ? k_csort_count<true> : k_csort_count<false>;
		if (allow_big_lds(count, p.lds))
		{
			return -2;
		}
		if (hipMemsetAsync(L.d_sort_bins, 0, static_cast<size_t>(p.bins) * sizeof(unsigned int), s) != hipSuccess)
		{
			return -2;
		}
		const dim3 chunks(p.chunks, L.n_windows);
		unsigned int* dstList = L.d_sorted + p.list_events;  // second half of the list buffer
		auto hist = L.mode == 1 ? k_csort_hist<1> : k_csort_hist<2>;
		hipLaunchKernelGGL(hist, chunks, dim3(256), p.lds_hist, s, L.d_events,
						   L.d_units, L.units_per_window, L.d_aux, p.rows_per_band, p.bands, L.d_sort_bins, dstList, L.c);
		hipLaunchKernelGGL(k_csort_scan, dim3(1), dim3(1024), 0, s, L.d_sort_bins, p.bins);
		hipLaunchKernelGGL(k_csort_scatter, chunks, dim3(256), p.lds_scatter, s, L.d_units, L.units_per_window, dstList,
						   p.rows_per_band, p.bands, L.d_sort_bins, p.bins, L.d_sorted, L.c);
		hipLaunchKernelGGL(count, grid, block, p.lds, s, L.d_sort_bins, p.bins, L.d_sorted, p.rows_per_band, p.bands,
						   L.d_image, L.c);
		return check_launch();
	}
	case kCountBands:
	{
		auto kern = p.u16 ? k_count_bands<true> : k_count_bands<false>;
		if (allow_big_lds(kern, p.lds))
		{
			return -2;
		}
		hipLaunchKernelGGL(kern, grid, block, p.lds, s, L.d_events, L.d_units, L.units_per_window, p.prb, p.n_regular,
						   p.col_tiles, L.d_image, L.c);
		return check_launch();
	}
	case kCountScatter:
		break;
	}
	if (p.grid_x > 0)
	{
		hipLaunchKernelGGL(k_count_scatter, grid, block, 0, s, L.d_events, L.d_units, L.units_per_window, L.mode, L.d_aux,
						   L.d_counts, L.c);
		if (check_launch())
		{
			return -2;
		}
	}
	const size_t n = static_cast<size_t>(L.n_windows) * L.c.image_w * L.c.image_h;
	hipLaunchKernelGGL(k_counts_to_f64, dim3(p.convert_blocks), dim3(256), 0, s, L.d_counts, L.d_image, n);
	return check_launch();
}

int launch_route(const RouteLaunch& L, void* stream)
{
	if (L.n_patches == 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_route, dim3(L.n_patches), dim3(64), 0, static_cast<hipStream_t>(stream), L.d_xy, L.n_events,
					   L.d_rects, L.d_start, L.d_take, L.cap, L.d_index, L.d_count, L.d_next);
	return check_launch();
}

int launch_patch_integrate(const PatchIntLaunch& L, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (L.n_patches == 0)
	{
		return 0;
	}
	const size_t lds = 64 * 1024;  // tiles up to 16384 pixels (default patch is 25x25)
	hipLaunchKernelGGL(k_patch_integrate, dim3(L.n_patches), dim3(256), lds, s, L.d_events,
					   L.d_offsets, L.d_rects, L.d_traj, L.d_nabla_off, L.d_nabla);
	return check_launch();
}

}  // namespace ebo

// ---- image front end (ebo_frontend.inc) ----
namespace ebo
{
int launch_fe_gradients(const uint8_t* d_img, const double* d_lut, int w, int h, double* d_gx, double* d_gy, void* stream)
{
	const dim3 grid((w + kFeTileW - 1) / kFeTileW, (h + kFeTileH - 1) / kFeTileH);
	hipLaunchKernelGGL(k_fe_gradients, grid, dim3(kFeTileW, kFeTileH), 0, static_cast<hipStream_t>(stream), d_img, d_lut,
					   w, h, d_gx, d_gy);
	return check_launch();
}

int fe_harris_blocks(int w, int h)
{
	return ((w + kFeHarrisT - 1) / kFeHarrisT) * ((h + kFeHarrisT - 1) / kFeHarrisT);
}

int launch_fe_harris(const uint8_t* d_img, const uint8_t* d_mask, int w, int h, int block_size, double k, double quality,
					 double* d_resp, double* d_bmax, double* d_candR, int* d_candI, int* d_count, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (hipMemsetAsync(d_count, 0, sizeof(int), s) != hipSuccess)
	{
		return -2;
	}
	const dim3 grid((w + kFeHarrisT - 1) / kFeHarrisT, (h + kFeHarrisT - 1) / kFeHarrisT);
	hipLaunchKernelGGL(k_fe_harris, grid, dim3(kFeHarrisT, kFeHarrisT), 0, s, d_img, d_mask, w, h, block_size, k, d_resp,
					   d_bmax);
	if (check_launch())
	{
		return -2;
	}
	const int npx = w * h;
	hipLaunchKernelGGL(k_fe_candidates, dim3((npx + 255) / 256), dim3(256), 0, s, d_resp, d_mask, w, h, quality, d_bmax,
					   fe_harris_blocks(w, h), d_candR, d_candI, d_count);
	return check_launch();
}

int launch_fe_select(double* d_candR, int* d_candI, const int* d_count, int n, int cap, int w, int max_corners,
					 double min_distance, float* d_corners, int* d_nout, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const int sorted = n > kFeLdsSort ? 1 : 0;
	if (sorted)
	{
		int N = 1;
		while (N < n)
		{
			N <<= 1;
		}
		if (N > cap)
		{
			return -1;
		}
		hipLaunchKernelGGL(k_fe_pad, dim3((N + 255) / 256), dim3(256), 0, s, d_candR, d_candI, d_count, N);
		for (int kk = 2; kk <= N; kk <<= 1)
		{
			for (int jj = kk >> 1; jj > 0; jj >>= 1)
			{
				hipLaunchKernelGGL(k_fe_bitonic_step, dim3((N + 255) / 256), dim3(256), 0, s, d_candR, d_candI, N, kk, jj);
			}
		}
		if (check_launch())
		{
			return -2;
		}
	}
	hipLaunchKernelGGL(k_fe_select, dim3(1), dim3(1024), 0, s, d_candR, d_candI, d_count, sorted, w, max_corners,
					   min_distance, d_corners, d_nout);
	return check_launch();
}

int launch_fe_pyramid(char* d_pyr, const FeLevel* lv, int n_levels, void* stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	for (int l = 1; l < n_levels; ++l)
	{
		const int np = lv[l].w * lv[l].h;
		hipLaunchKernelGGL(k_fe_pyrdown, dim3((np + 255) / 256), dim3(256), 0, s,
						   reinterpret_cast<const uint8_t*>(d_pyr + lv[l - 1].img), lv[l - 1].w, lv[l - 1].h,
						   reinterpret_cast<uint8_t*>(d_pyr + lv[l].img), lv[l].w, lv[l].h);
	}
	for (int l = 0; l < n_levels; ++l)
	{
		const int np = lv[l].w * lv[l].h;
		hipLaunchKernelGGL(k_fe_scharr, dim3((np + 255) / 256), dim3(256), 0, s,
						   reinterpret_cast<const uint8_t*>(d_pyr + lv[l].img), lv[l].w, lv[l].h,
						   reinterpret_cast<short2*>(d_pyr + lv[l].der));
	}
	return check_launch();
}

int launch_fe_lk(const char* d_prev, const char* d_next, const FeLevel* d_lv, int n_levels, int n, const float* d_prev_xy,
				 float* d_next_xy, uint8_t* d_status, float* d_err, int win_w, int win_h, int max_count, double eps2,
				 float min_eig, void* stream)
{
	if (n == 0)
	{
		return 0;
	}
	hipLaunchKernelGGL(k_fe_lk, dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), d_prev, d_next, d_lv,
					   n_levels, n, d_prev_xy, d_next_xy, d_status, d_err, win_w, win_h, max_count, eps2, min_eig);
	return check_launch();
}
}  // namespace ebo

#ifdef EBO_EDGE_TIMING
// Phase clocks (instrumented build only): the 64 rows of the device table summed into out32.
extern "C" int ebo_debug_edge_clocks(unsigned long long* out32, int reset)
{
	static unsigned long long rows[64 * 32];
	if (hipDeviceSynchronize() != hipSuccess)
	{
		return -1;
	}
	if (out32)
	{
		if (hipMemcpyFromSymbol(rows, HIP_SYMBOL(ebo::g_edge_clk), sizeof(rows)) != hipSuccess)
		{
			return -1;
		}
		for (int k = 0; k < 32; ++k)
		{
			out32[k] = 0;
			for (int r = 0; r < 64; ++r)
			{
				out32[k] += rows[r * 32 + k];
			}
		}
	}
	if (reset)
	{
		for (auto& v : rows)
		{
			v = 0;
		}
		if (hipMemcpyToSymbol(HIP_SYMBOL(ebo::g_edge_clk), rows, sizeof(rows)) != hipSuccess)
		{
			return -1;
		}
	}
	return 0;
}
#endif
