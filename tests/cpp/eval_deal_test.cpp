// The index arithmetic of k_eval3's bank deal (csrc/eval_deal.h, free of HIP) against a brute-force loop: for workgroups
// of 128, 256 and 512 lanes and unit sizes 1, 2, 127, 128, 129, 8 x block +- 1 and the admission bounds +- 1, the slots are
// a permutation of the lanes, deal_start is the running count of a plain walk over the slots, the forward map is a
// permutation of 0 .. n-1 with deal_position as its inverse, the dealt list is walked in exactly the wave-rounds of the
// canonical one (no hole, no added round), and the admission and capacity rules are what the header says.
#include "../../event-based-odomety_amd/csrc/eval_deal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                                  \
	do                                                    \
	{                                                     \
		if (!(cond))                                      \
		{                                                 \
			std::printf("FAILED %s: ", #cond);            \
			std::printf(__VA_ARGS__);                     \
			std::printf("\n");                            \
			if (++failures > 20)                          \
			{                                             \
				std::exit(1);                             \
			}                                             \
		}                                                 \
	} while (0)

static void check_maps(uint32_t n, int block)
{
	using namespace ebo;
	// the slots are a permutation of the lanes
	std::vector<int> laneOfSlot(block, -1);
	for (int lane = 0; lane < block; ++lane)
	{
		const int s = deal_slot(lane, block);
		CHECK(s >= 0 && s < block && laneOfSlot[s] < 0, "slot %d of lane %d (block %d)", s, lane, block);
		laneOfSlot[s] = lane;
	}
	// brute force: walk the slots in order; a slot's lane is live in round k when k * block + lane < n
	std::vector<uint32_t> start(block, 0);
	uint32_t run = 0;
	for (int s = 0; s < block; ++s)
	{
		const int lane = laneOfSlot[s];
		start[lane] = run;
		for (uint32_t k = 0; k * block + lane < n; ++k)
		{
			++run;
		}
	}
	CHECK(run == n, "slots hold %u of %u elements (block %d)", run, n, block);
	for (int lane = 0; lane < block; ++lane)
	{
		CHECK(deal_start(lane, n, block) == start[lane], "deal_start(%d, %u, %d) = %u, walk %u", lane, n, block,
			  deal_start(lane, n, block), start[lane]);
	}
	// the forward map is a permutation with deal_position as its inverse
	std::vector<char> seen(n, 0);
	for (uint32_t q = 0; q < n; ++q)
	{
		const uint32_t s = deal_sorted_index(q, n, block);
		CHECK(s < n && !seen[s], "position %u -> sorted %u (n %u, block %d)", q, s, n, block);
		if (s < n)
		{
			seen[s] = 1;
			CHECK(deal_position(s, n, block) == q, "inverse of %u is %u, not %u (n %u, block %d)", s, deal_position(s, n, block), q,
				  n, block);
		}
	}
	CHECK(deal_position(n, n, block) == n, "past the end (n %u, block %d)", n, block);
	// wave-rounds: the list has n positions walked as the canonical order is, so the live (wave, round) pairs are the same
	// by construction; what the layout must not do is leave a live lane without an element or give one to an idle lane
	for (int lane = 0; lane < block; ++lane)
	{
		const uint32_t live = n / block + (static_cast<uint32_t>(lane) < n % block ? 1u : 0u);
		const int next = deal_slot(lane, block) + 1 < block ? laneOfSlot[deal_slot(lane, block) + 1] : -1;
		const uint32_t end = next >= 0 ? deal_start(next, n, block) : n;
		CHECK(end - deal_start(lane, n, block) == live, "lane %d owns %u elements, is live in %u rounds (n %u, block %d)", lane,
			  end - deal_start(lane, n, block), live, n, block);
	}
	// the lanes of a 16-lane group are block / 16 slots apart
	for (int lane = 0; lane + 1 < block; ++lane)
	{
		if ((lane + 1) % kDealGroup != 0)
		{
			CHECK(deal_slot(lane + 1, block) - deal_slot(lane, block) == block / kDealGroup, "lanes %d, %d", lane, lane + 1);
		}
	}
}

int main()
{
	using namespace ebo;
	for (int block : {128, 256, 512})
	{
		const uint32_t lo = kDealMinRounds * block, hi = kDealMaxRounds * block;
		const uint32_t sizes[] = {1, 2, 127, 128, 129, 8u * block - 1, 8u * block, 8u * block + 1, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1};
		for (uint32_t n : sizes)
		{
			check_maps(n, block);
			const bool want = block <= kDealMaxBlock && n >= lo && n <= hi;
			CHECK(deal_admits(n, block, 1) == want, "admission of %u at %d", n, block);
			CHECK(!deal_admits(n, block, 2), "row tiles are not dealt (%u at %d)", n, block);
			// the list and the scratch: 16-bit indices, 17 counters of 32 bits per lane
			CHECK(deal_list_doubles(n) * 8 >= static_cast<int>(n) * 2 && deal_list_doubles(n) * 8 < static_cast<int>(n) * 2 + 8, "list bytes of %u", n);
			CHECK(deal_counter_doubles(block) * 8 >= kDealKeys * block * 4, "counter bytes at %d", block);
			CHECK(deal_scratch_doubles(n, block) == deal_counter_doubles(block) + deal_list_doubles(n), "scratch of %u at %d", n, block);
			const int list = deal_list_doubles(n), scratch = deal_scratch_doubles(n, block);
			for (int band : {1, scratch - 1, scratch, scratch + 1, 2000})
			{
				const int need = list + (band > scratch ? band : scratch);
				CHECK(deal_fits(n, block, need, band), "fits exactly (%u, %d, band %d)", n, block, band);
				CHECK(!deal_fits(n, block, need - 1, band), "one double short (%u, %d, band %d)", n, block, band);
			}
		}
		// the keys of a lane fit its 64-bit register
		CHECK(kDealMaxRounds * kDealKeyBits <= 64 && (1 << kDealKeyBits) >= kDealKeys, "key packing");
	}
	// the headline's shape: 128 lanes, 2542 pixels -- a mean unit of 781 events leaves 2346 pixels to its image
	CHECK(deal_fits(781, 128, 2542, 2346) && !deal_fits(781, 128, 2542, 2347), "the headline's capacity left");
	// exact fits at the shipped capacities (eval_plan.h; tests/deal_fit_cases.py): both ends of the admitted counts at 2540
	// (128 lanes), the upper end at 5080 (256 lanes), and the whole 90 x 66 canvas at its pitch of 91 in 6680, where the
	// list alone is the boundary; one event more is one double of list more
	CHECK(deal_admits(260, 128, 1) && deal_fits(260, 128, 2540, 45 * 55) && !deal_fits(261, 128, 2540, 45 * 55), "260 in 45 x 55");
	CHECK(deal_fits(257, 128, 2540, 45 * 55) && !deal_fits(260, 128, 2540, 45 * 56), "the quad's first count; a row more");
	CHECK(deal_admits(1536, 128, 1) && deal_fits(1536, 128, 2540, 49 * 44) && !deal_admits(1537, 128, 1), "1536 in 49 x 44");
	CHECK(deal_admits(3072, 256, 1) && deal_fits(3072, 256, 5080, 77 * 56) && !deal_fits(3072, 256, 5080, 77 * 56 + 1), "3072 in 77 x 56");
	CHECK(deal_fits(2696, 256, 6680, 91 * 66) && !deal_fits(2697, 256, 6680, 91 * 66), "the whole canvas at sigma < 1");
	CHECK(deal_fits(820, 128, 3340, 55 * 57) && !deal_fits(820, 128, 3340, 55 * 58), "820 in 55 x 57 at 3340");
	// two sub-bands: 2540 mod 91 = 83 doubles stay behind the 27 rows of a 91-pixel pitch
	CHECK(deal_fits(332, 128, 2540, 27 * 91) && !deal_fits(333, 128, 2540, 27 * 91), "behind a full sub-band");
	if (failures == 0)
	{
		std::printf("all passed\n");
	}
	return failures ? 1 : 0;
}
