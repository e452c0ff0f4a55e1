// eval_plan.h -- the shape of a variance evaluation's launch (k_eval3): workgroup size, workgroups per CU, LDS per
// workgroup, the LDS header and the image capacity behind it.  Header-only and free of HIP, so that the rule is a table
// the CPU test-suite pins (tests/cpp/eval_plan_test.cpp) and eval_launch_shape (ebo_api.cpp) only launches what the plan
// says.  The plan reads no environment: eval_launch_shape reads the A/B switches (ab_env.h) into the shape.  It follows
// the geometry and the number of flow slots only, never the data: a window evaluates to the same bits alone and inside
// any batch on the same side of kEvalManySlots.
//
// The LDS of one workgroup is  [ sums: 8 doubles per wave | box scratch: 4 ints per wave | image: cap_doubles ].
//
// k_eval3 is compiled for a number of waves per CU (16 at 128 VGPRs, 12 for the sigma < 1 instantiation), and what a launch
// of many units chooses is how to cut them into workgroups -- more, smaller workgroups overlap their barrier-separated
// passes better on the CU's one LDS, but each gets less of it, and a box that does not fit is counted in sequential
// sub-bands (every event warped again per sub-band).  By the canvas of the REGULAR patch:
//    canvas <= 32 KB (the reference's 20x20 patches, C3's 21x16): 128 lanes, waves / 2 workgroups per CU
//    larger (C2 30x22, C4 40x22):                                  256 lanes, waves / 4 workgroups per CU
// and every workgroup gets the budget divided by that count (rounded down to 1280 B, a multiple of the LDS allocation
// granule): every wave slot of the CU is filled, which a fixed 22 KB (seven workgroups, 14 of 16 waves) did not do.  The
// header is sized by the workgroup's waves, not for the largest workgroup: at 128 lanes that is 160 B instead of
// 1280 B, a seventh of what the eighth workgroup costs the image.
// With fewer than kEvalManySlots flow slots a 512-lane workgroup shortens the per-unit critical path; that branch keeps
// its 40 KB and the header of 160 doubles (its sums' reduction order and its capacity, so its bits, stay).
#pragma once

#include <stddef.h>

#include <algorithm>

namespace ebo
{
constexpr int kEvalManySlots = 1024;            // flow slots from which the many-units shapes apply
constexpr size_t kEvalLdsStep = 1280;           // LDS per workgroup is rounded down to this
constexpr size_t kEvalSmallCanvasBytes = 32 * 1024;
constexpr int kEvalFloorRows = 24;              // at least this many rows of the widest canvas, where the budget allows

// Doubles of the header of a workgroup of `waves` waves: eight sums per wave (seven used), then block_minmax's four ints
// per wave, rounded to 16 bytes.  header(16) = 160 is what k_solve_independent, the dump kernel and the edge loss keep.
constexpr int eval_sum_doubles(int waves)
{
	return waves * 8;
}
constexpr int eval_header_doubles(int waves)
{
	return eval_sum_doubles(waves) + static_cast<int>((static_cast<size_t>(waves) * 4 * sizeof(int) + 15) / 16 * 2);
}
constexpr int kEvalHeaderWavesMax = 16;
static_assert(eval_header_doubles(kEvalHeaderWavesMax) == 160, "the 16-wave header is the 160 doubles other kernels keep");

struct EvalShape
{
	int reg_rw = 0, reg_rh = 0;  // the regular patch
	int max_rw = 0;              // the widest patch (the last column of a grid absorbs the sensor's remainder)
	int flow_slots = 0;
	size_t lds_budget = 0;       // LDS of one CU
	int waves_per_cu = 0;        // what the kernel instantiation is compiled for
	// A/B overrides (ab_env.h; constant in the shipped build)
	int block = 0;               // EBO_EVAL_BLOCK: a multiple of 64 in [64, 512], 0 = the rule's
	size_t lds_kb = 0;           // EBO_LDS_KB: LDS per workgroup before the floor, 0 = the rule's
};

struct EvalPlan
{
	bool ok = false;             // false: one row of the widest canvas does not fit the budget
	int block = 0;
	int workgroups_per_cu = 0;   // resident workgroups the plan intends (LDS and wave slots)
	size_t lds_bytes = 0;        // dynamic LDS of one workgroup
	int header_waves = 0;        // waves the header is sized for
	int header_doubles = 0;
	int cap_doubles = 0;         // pixels of the image behind the header
};

inline EvalPlan plan_eval(const EvalShape& S)
{
	EvalPlan p;
	const bool many = S.flow_slots >= kEvalManySlots;
	const bool smallCanvas = static_cast<size_t>(9) * S.reg_rw * S.reg_rh * sizeof(double) <= kEvalSmallCanvasBytes;
	const int ruleBlock = many ? (smallCanvas ? 128 : 256) : 512;
	p.block = S.block > 0 ? S.block : ruleBlock;
	const int waves = (p.block + 63) / 64;
	// the header follows the workgroup that runs, the LDS the class of the geometry (a forced block keeps the class's bytes)
	p.header_waves = many ? waves : kEvalHeaderWavesMax;
	p.header_doubles = eval_header_doubles(p.header_waves);
	const size_t headerBytes = static_cast<size_t>(p.header_doubles) * sizeof(double);
	size_t bytes;
	if (S.lds_kb > 0)
	{
		bytes = std::min(std::max<size_t>(S.lds_kb, 4) * 1024, S.lds_budget);
	}
	else if (many)
	{
		const int groups = std::max(S.waves_per_cu / (ruleBlock / 64), 1);
		bytes = S.lds_budget / groups / kEvalLdsStep * kEvalLdsStep;
	}
	else
	{
		bytes = std::min<size_t>(40 * 1024, S.lds_budget);
	}
	// keep at least kEvalFloorRows rows of the widest canvas where that fits
	const size_t rowBytes = static_cast<size_t>(3) * S.max_rw * sizeof(double);
	bytes = std::min(std::max(bytes, kEvalFloorRows * rowBytes + headerBytes), S.lds_budget);
	if (bytes < headerBytes + rowBytes)
	{
		return p;
	}
	p.lds_bytes = bytes;
	p.cap_doubles = static_cast<int>((bytes - headerBytes) / sizeof(double));
	p.workgroups_per_cu = static_cast<int>(std::min<size_t>(S.lds_budget / bytes, static_cast<size_t>(std::max(S.waves_per_cu / waves, 1))));
	p.ok = true;
	return p;
}
}  // namespace ebo
