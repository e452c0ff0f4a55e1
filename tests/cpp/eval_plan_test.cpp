// The launch plan of the variance evaluation (csrc/eval_plan.h) on the CPU, swept over every patch geometry ebo_create
// admits (1 <= patch <= image <= kCoordMax: regular widths and heights, with the widest patch anywhere from the regular
// one to twice it less one, as the last column of a grid is), both wave caps k_eval3 is compiled for, and flow-slot
// counts on both sides of 1024:
//   (a) workgroups x LDS <= budget, a block of whole waves, at least one workgroup;
//   (b) one full row of the widest canvas fits, or the plan refuses -- and it refuses only then;
//   (c) the header holds the block's waves: 8 sums per wave, then 4 ints per wave, rounded to 16 bytes;
//   (d) capacity = (LDS - header) / 8;
//   (e) many slots: the rule's numbers -- C3 and the reference's 20x20 give 8 x 20 480 B at 16 waves, 6 x 26 880 B at
//       12; C2 and C4 4 x 40 960 B and 3 x 53 760 B;
//   (f) EBO_LDS_KB = 4 is floored at 24 rows of the widest canvas: exactly 1440 pixels on 20x20 patches, either side;
//   (g) fewer than 1024 slots: 512 lanes, 40 KB, the 160-double header, 4960 pixels -- the shape before the plan;
//   (h) the forced block sizes: the header follows the block, the LDS does not.
// Run by tests/test_eval_plan_cpu.py; prints "all passed".
#include "../../event-based-odomety_amd/csrc/eval_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace ebo;

namespace
{
constexpr size_t kBudget = 160 * 1024;
constexpr int kCoordMax = 32767;
int failures = 0;

#define CHECK(cond, ...)                                  \
	do                                                    \
	{                                                     \
		if (!(cond))                                      \
		{                                                 \
			if (++failures <= 20)                         \
			{                                             \
				std::printf("FAILED %s: ", #cond);        \
				std::printf(__VA_ARGS__);                 \
				std::printf("\n");                        \
			}                                             \
		}                                                 \
	} while (0)

EvalShape shape(int rw, int rh, int maxRw, int slots, int waves, int block = 0, size_t ldsKb = 0)
{
	EvalShape s;
	s.reg_rw = rw;
	s.reg_rh = rh;
	s.max_rw = maxRw;
	s.flow_slots = slots;
	s.lds_budget = kBudget;
	s.waves_per_cu = waves;
	s.block = block;
	s.lds_kb = ldsKb;
	return s;
}

void check_invariants(const EvalShape& s)
{
	const EvalPlan p = plan_eval(s);
	const size_t rowBytes = static_cast<size_t>(3) * s.max_rw * 8;
	if (!p.ok)
	{
		// refused only when the budget does not hold the header and one row
		CHECK(rowBytes + 8 * static_cast<size_t>(p.header_doubles) > kBudget, "refused rw %d rh %d max %d slots %d", s.reg_rw, s.reg_rh,
			  s.max_rw, s.flow_slots);
		CHECK(p.header_doubles > 0, "a refusal still names its header");
		return;
	}
	const int waves = p.block / 64;
	CHECK(p.block % 64 == 0 && p.block >= 64 && p.block <= 512, "block %d", p.block);
	CHECK(p.workgroups_per_cu >= 1, "workgroups %d", p.workgroups_per_cu);
	CHECK(static_cast<size_t>(p.workgroups_per_cu) * p.lds_bytes <= kBudget, "rw %d rh %d max %d slots %d waves %d: %d x %zu", s.reg_rw,
		  s.reg_rh, s.max_rw, s.flow_slots, s.waves_per_cu, p.workgroups_per_cu, p.lds_bytes);
	CHECK(p.workgroups_per_cu * waves <= std::max(s.waves_per_cu, waves), "more waves than the CU holds: %d x %d", p.workgroups_per_cu, waves);
	CHECK(p.cap_doubles >= 3 * s.max_rw, "a canvas row of %d pixels in %d", 3 * s.max_rw, p.cap_doubles);
	CHECK(p.header_waves >= waves, "header of %d waves, block of %d", p.header_waves, waves);
	CHECK(p.header_doubles == p.header_waves * 8 + (p.header_waves * 4 * 4 + 15) / 16 * 2, "header %d doubles for %d waves", p.header_doubles,
		  p.header_waves);
	CHECK(p.header_doubles % 2 == 0, "the image starts 16-byte aligned");
	CHECK(static_cast<size_t>(p.cap_doubles) == (p.lds_bytes - static_cast<size_t>(p.header_doubles) * 8) / 8, "capacity %d of %zu B", p.cap_doubles,
		  p.lds_bytes);
	CHECK(static_cast<size_t>(p.header_doubles + p.cap_doubles) * 8 <= p.lds_bytes, "header and image inside the LDS");
}

void expect(const char* name, const EvalShape& s, int block, int groups, size_t lds, int header, int cap)
{
	const EvalPlan p = plan_eval(s);
	CHECK(p.ok && p.block == block && p.workgroups_per_cu == groups && p.lds_bytes == lds && p.header_doubles == header && p.cap_doubles == cap,
		  "%s: block %d groups %d lds %zu header %d cap %d", name, p.block, p.workgroups_per_cu, p.lds_bytes, p.header_doubles, p.cap_doubles);
}
}  // namespace

int main()
{
	// the sweep: dense over small patches, then the sizes up to the largest sensor
	long swept = 0;
	for (int waves : {16, 12})
	{
		for (int slots : {1, 108, 1023, 1024, 1080, 32768, 1 << 20})
		{
			auto geometry = [&](int rw, int rh) {
				for (int maxRw : {rw, rw + 1, rw + rw / 2, 2 * rw - 1})
				{
					if (maxRw < rw || maxRw > kCoordMax)
					{
						continue;
					}
					check_invariants(shape(rw, rh, maxRw, slots, waves));
					check_invariants(shape(rw, rh, maxRw, slots, waves, 0, 4));
					++swept;
				}
			};
			for (int rw = 1; rw <= 96; ++rw)
			{
				for (int rh = 1; rh <= 96; ++rh)
				{
					geometry(rw, rh);
				}
			}
			for (int rw : {127, 128, 240, 346, 640, 1280, 2269, 2270, 3407, 3408, 6819, 6820, 6826, 6827, 13000, kCoordMax})
			{
				for (int rh : {1, 16, 180, 720, kCoordMax})
				{
					geometry(rw, rh);
				}
			}
			for (int block : {64, 128, 192, 256, 320, 384, 448, 512})
			{
				for (size_t kb : {size_t(0), size_t(1), size_t(4), size_t(22), size_t(64), size_t(160), size_t(1000)})
				{
					check_invariants(shape(20, 20, 20, slots, waves, block, kb));
					check_invariants(shape(21, 16, 31, slots, waves, block, kb));
					check_invariants(shape(40, 22, 40, slots, waves, block, kb));
				}
			}
		}
	}
	// (e) the rule's numbers
	expect("C3 x 128, 16 waves", shape(21, 16, 31, 32768, 16), 128, 8, 20480, 20, 2540);
	expect("20x20 x 10, 16 waves", shape(20, 20, 20, 1080, 16), 128, 8, 20480, 20, 2540);
	expect("C3, 12 waves", shape(21, 16, 31, 32768, 12), 128, 6, 26880, 20, 3340);
	expect("C2 x 256, 16 waves", shape(30, 22, 30, 16384, 16), 256, 4, 40960, 40, 5080);
	expect("C4 x 8, 16 waves", shape(40, 22, 40, 8192, 16), 256, 4, 40960, 40, 5080);
	expect("C4, 12 waves", shape(40, 22, 40, 8192, 12), 256, 3, 53760, 40, 6680);
	// the class boundary: a regular canvas of 32 KB (9 rw rh 8 = 32 768: rw rh = 455 is in, 456 out)
	expect("canvas 35x13", shape(35, 13, 35, 1024, 16), 128, 8, 20480, 20, 2540);
	expect("canvas 24x19", shape(24, 19, 24, 1024, 16), 256, 4, 40960, 40, 5080);
	// (f) the floor of a forced 4 KB: 24 rows of the widest canvas
	expect("20x20, 4 KB, few", shape(20, 20, 20, 108, 16, 0, 4), 512, 2, 24 * 60 * 8 + 1280, 160, 1440);
	expect("20x20, 4 KB, many", shape(20, 20, 20, 1080, 16, 0, 4), 128, 8, 24 * 60 * 8 + 160, 20, 1440);
	expect("C3, 4 KB, many", shape(21, 16, 31, 32768, 16, 0, 4), 128, 8, 24 * 93 * 8 + 160, 20, 24 * 93);
	// the floor also lifts the rule's own bytes where 24 rows ask for more (and costs resident workgroups)
	expect("50x9 patches", shape(50, 9, 99, 4096, 16), 128, 2, 24 * 297 * 8 + 160, 20, 24 * 297);
	// (g) fewer than 1024 slots: unchanged
	expect("20x20 x 1", shape(20, 20, 20, 108, 16), 512, 2, 40960, 160, 4960);
	expect("C3 x 1", shape(21, 16, 31, 256, 16), 512, 2, 40960, 160, 4960);
	expect("C4 x 0 slots", shape(40, 22, 40, 1023, 12), 512, 1, 40960, 160, 4960);
	// (h) forced blocks: the header follows, the bytes stay
	expect("C3, 64 lanes", shape(21, 16, 31, 32768, 16, 64), 64, 8, 20480, 10, 2550);
	expect("C3, 192 lanes", shape(21, 16, 31, 32768, 16, 192), 192, 5, 20480, 30, 2530);
	expect("C3, 512 lanes", shape(21, 16, 31, 32768, 16, 512), 512, 2, 20480, 80, 2480);
	expect("20x20 x 1, 128 lanes", shape(20, 20, 20, 108, 16, 128), 128, 4, 40960, 160, 4960);
	// the widest row the budget holds, and one pixel more
	{
		const int widest = static_cast<int>((kBudget - 320) / 8 / 3);  // (a canvas that wide is of the 256-lane class)
		CHECK(plan_eval(shape(widest, 1, widest, 4096, 16)).ok, "a row of %d pixels fits", 3 * widest);
		CHECK(!plan_eval(shape(widest + 1, 1, widest + 1, 4096, 16)).ok, "a row of %d pixels does not", 3 * widest + 3);
	}
	if (failures)
	{
		std::printf("%d checks failed\n", failures);
		return 1;
	}
	std::printf("swept %ld shapes\nall passed\n", swept);
	return 0;
}
