// eval_deal.h -- the index arithmetic of k_eval3's bank deal (eval_unit3).  Header-only and free of
// HIP, so that the maps are pinned by a CPU test (tests/cpp/eval_deal_test.cpp) and the kernel only applies them.
//
// Both tap passes of an evaluation run lane = event with one fixed tap per LDS instruction, so what an instruction costs is
// decided by the residues of its lanes' first-tap words modulo the number of bank pairs one access group sees: 16 lanes
// over 16 bank pairs for ds_add_u64, 32 over 32 for ds_read_b64.  In the canonical order the residues are random and two
// thirds of the LDS cycles are conflicts.  The deal re-orders a unit's events ONCE per evaluation so that the lanes of a
// 16-lane group hold different residues:
//
//   key     the residue modulo 16 of the event's first-tap word relative to the box,
//           ((pyc - 3 - y0) * cols + (pxc - 3 - x0)) & 15; an event warp_event rejects has the key 16.
//   sort    a stable counting sort of the unit's n events by (key, lane, round), where the event at canonical position e is
//           held by lane e mod block in round e div block.  The order is unique: it follows from the unit's events, the
//           flow, the box and the block size alone.
//   layout  the dealt list has exactly n positions and is walked like the canonical one, position q by lane q mod block
//           in round q div block: the rounds, and the lanes live in the last one, are today's, so no wave-round is added
//           and no position is a hole.  Lane L owns the slot (L mod 16) * (block / 16) + L div 16, slots own consecutive
//           runs of the sorted order, one element per round the slot's lane is live in; position q takes the sorted
//           element deal_start(L) + q div block.  The lanes of a 16-lane group are block / 16 slots, about one key, apart.
//
// A unit is dealt where the fixed cost of the sort (17 counters per lane, a scan, four barriers) is spread over at least
// kDealMinRounds full rounds, its keys fit the lane's one 64-bit register (kDealMaxRounds of 5 bits), it has one row
// tile, its workgroup has at most kDealMaxBlock lanes, and the list fits behind the largest sub-band's image WITHOUT
// changing the sub-bands: the image keeps its place, pitch and rows, so the value sums keep their bits, and a unit
// whose box leaves no room is evaluated as before.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define EBO_DEAL_HD __host__ __device__
#else
#define EBO_DEAL_HD
#endif

namespace ebo
{
constexpr int kDealGroup = 16;               // lanes of one access group of ds_add_u64 = residues of the key
constexpr int kDealKeys = kDealGroup + 1;    // and the key of a rejected event, sorted last
constexpr int kDealKeyBits = 5;
constexpr int kDealMaxRounds = 12;           // keys of one lane: 12 x 5 bits in a 64-bit register pair
constexpr int kDealMinRounds = 2;            // full rounds below which the sort's fixed cost is not spread enough
constexpr int kDealMaxBlock = 256;           // the 512-lane workgroups of small launches are not dealt (their counters alone
                                             // would take 34 KB of the 40 KB, and a small launch is not bound by the LDS)

// by the unit's event count, the block size and the row tiles alone
inline EBO_DEAL_HD bool deal_admits(uint32_t n, int block, int tiles)
{
	return tiles == 1 && block % 64 == 0 && block <= kDealMaxBlock && n >= static_cast<uint32_t>(kDealMinRounds * block) &&
		   n <= static_cast<uint32_t>(kDealMaxRounds * block);
}
// doubles of the list: 16-bit canonical indices, one per position
inline EBO_DEAL_HD int deal_list_doubles(uint32_t n)
{
	return static_cast<int>((n + 3) / 4);
}
// doubles of the sort's scratch in the not yet zeroed image: kDealKeys 32-bit counters per lane, then the sorted indices
inline EBO_DEAL_HD int deal_counter_doubles(int block)
{
	return (kDealKeys * block + 1) / 2;
}
inline EBO_DEAL_HD int deal_scratch_doubles(uint32_t n, int block)
{
	return deal_counter_doubles(block) + deal_list_doubles(n);
}
// the list sits at the END of the image area of capDoubles; bandPixels: the largest sub-band's image
inline EBO_DEAL_HD bool deal_fits(uint32_t n, int block, int capDoubles, int bandPixels)
{
	const int list = deal_list_doubles(n);
	const int scratch = deal_scratch_doubles(n, block);
	return list + (bandPixels > scratch ? bandPixels : scratch) <= capDoubles;
}
inline EBO_DEAL_HD int deal_slot(int lane, int block)
{
	return (lane % kDealGroup) * (block / kDealGroup) + lane / kDealGroup;
}
// The first sorted element of lane `lane`'s slot: every slot before it holds n div block elements, and one more where
// its lane is live in the last round (lane' < n mod block).  Slot s' = a * per + b belongs to lane b * 16 + a; with
// n mod block = d * 16 + r the slots of row a that are live in the last round are b < d + (a < r).
inline EBO_DEAL_HD uint32_t deal_start(int lane, uint32_t n, int block)
{
	const uint32_t full = n / static_cast<uint32_t>(block), rem = n % static_cast<uint32_t>(block);
	const uint32_t a = static_cast<uint32_t>(lane % kDealGroup), b = static_cast<uint32_t>(lane / kDealGroup);
	const uint32_t d = rem / kDealGroup, r = rem % kDealGroup;
	const uint32_t rowLive = d + (a < r ? 1u : 0u);
	const uint32_t extra = a * d + (a < r ? a : r) + (b < rowLive ? b : rowLive);
	return static_cast<uint32_t>(deal_slot(lane, block)) * full + extra;
}
// forward map: the sorted element that list position q takes
inline EBO_DEAL_HD uint32_t deal_sorted_index(uint32_t q, uint32_t n, int block)
{
	return deal_start(static_cast<int>(q % static_cast<uint32_t>(block)), n, block) + q / static_cast<uint32_t>(block);
}
// inverse map: the list position of sorted element s (host side and tests: a search over the lanes)
inline uint32_t deal_position(uint32_t s, uint32_t n, int block)
{
	for (int lane = 0; lane < block; ++lane)
	{
		const uint32_t first = deal_start(lane, n, block);
		const uint32_t count = n / static_cast<uint32_t>(block) + (static_cast<uint32_t>(lane) < n % static_cast<uint32_t>(block) ? 1u : 0u);
		if (s >= first && s < first + count)
		{
			return (s - first) * static_cast<uint32_t>(block) + static_cast<uint32_t>(lane);
		}
	}
	return n;  // (s >= n)
}
}  // namespace ebo
