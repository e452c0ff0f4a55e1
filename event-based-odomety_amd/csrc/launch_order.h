// launch_order.h — the order in which a launch hands a batch's units to workgroups (free of HIP:
// tests/cpp/launch_order_test.cpp).
//
// One workgroup evaluates one unit and lives about as long as the unit has events; a batch's units differ by an
// order of magnitude (C3 x 128 windows: 150 .. 1861 events, mean 781).  Workgroups start in blockIdx order, so with
// blockIdx = unit index the last ones to start are a random mix and the launch ends with the chip draining for one
// heavy unit's lifetime.  Handed out heaviest first (longest processing time first) the last to start are the lightest.
// A unit is still evaluated by one workgroup of the same shape running the same code: the order changes no bit.
//
// The table: order[q] = unit that workgroup q takes.  key = n_ev of an active unit, 0 of any other (inactive and
// stray units return at once); descending key, ties by ascending unit index -- the result of a stable sort by key, and
// unique, so every loading path and every run gives the same table.  It depends on the loaded units only and is built
// once per load (ebo_windows.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ebo
{
enum LaunchOrderKind
{
	kOrderHeaviestFirst = 0,
	kOrderIndex = 1,         // the identity           (A/B build only: EBO_EVAL_ORDER=index)
	kOrderLightestFirst = 2  // ascending key           (A/B build only: EBO_EVAL_ORDER=light)
};

// n_ev and flags of unit i are read at n_ev + i * strideBytes and flags + i * strideBytes (two fields of an array of
// records, or two plain arrays with a stride of 4); activeBit is kUnitActive.  order[0 .. n), n < 2^32.
inline void fill_launch_order(const void* n_ev, const void* flags, size_t strideBytes, size_t n, uint32_t activeBit,
							  uint32_t* order, LaunchOrderKind kind = kOrderHeaviestFirst)
{
	if (kind == kOrderIndex)
	{
		for (size_t i = 0; i < n; ++i)
		{
			order[i] = static_cast<uint32_t>(i);
		}
		return;
	}
	const char* pn = static_cast<const char*>(n_ev);
	const char* pf = static_cast<const char*>(flags);
	std::vector<uint32_t> key(n);
	uint32_t maxKey = 0;
	for (size_t i = 0; i < n; ++i)
	{
		const uint32_t f = *reinterpret_cast<const uint32_t*>(pf + i * strideBytes);
		key[i] = (f & activeBit) ? *reinterpret_cast<const uint32_t*>(pn + i * strideBytes) : 0u;
		maxKey = std::max(maxKey, key[i]);
	}
	const bool descending = kind != kOrderLightestFirst;
	if (maxKey <= 8 * n + 1024)
	{
		// The keys are event counts of a patch, a few thousand at most: a stable counting sort, two passes over the
		// units and one over the counts (32 896 units of the bench's batch: 0.1 ms where a comparison sort took 2 ms --
		// a load pays this once, and a load is followed by ONE solve).  bin = maxKey - key for the descending order.
		std::vector<uint32_t> start(static_cast<size_t>(maxKey) + 2, 0u);
		for (size_t i = 0; i < n; ++i)
		{
			++start[(descending ? maxKey - key[i] : key[i]) + 1];
		}
		for (size_t b = 1; b < start.size(); ++b)
		{
			start[b] += start[b - 1];
		}
		for (size_t i = 0; i < n; ++i)  // ascending index inside a bin: stable
		{
			order[start[descending ? maxKey - key[i] : key[i]]++] = static_cast<uint32_t>(i);
		}
		return;
	}
	// few units with huge counts: (sort key, index) in one word -- the words are distinct, so a plain sort of them IS
	// the stable sort by key
	std::vector<uint64_t> keyed(n);
	for (size_t i = 0; i < n; ++i)
	{
		keyed[i] = (static_cast<uint64_t>(descending ? ~key[i] : key[i]) << 32) | static_cast<uint32_t>(i);
	}
	std::sort(keyed.begin(), keyed.end());
	for (size_t i = 0; i < n; ++i)
	{
		order[i] = static_cast<uint32_t>(keyed[i]);
	}
}
}  // namespace ebo
