// The launch-order table of csrc/launch_order.h as the host compiles it (free of HIP).  Reads from stdin
//   kind n            (kind: 0 heaviest first, 1 index, 2 lightest first)
//   n lines "n_ev flags"
// and prints the n entries of the table, one per line.  The records are laid out as the library's Unit is (28 bytes,
// n_ev at byte 4, flags at byte 20), so the strided reads are the ones the library makes.  With the argument `self` it
// runs its own checks over the edge cases and 40 000 random counts instead (what a sanitizer build runs) and prints
// "ok".  tests/test_launch_order_cpu.py compiles this, runs both forms and compares with numpy.
#include "../../event-based-odomety_amd/csrc/launch_order.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace
{
struct Rec  // the layout of ebo::Unit (ebo_internal.h)
{
	uint32_t ev_off;
	uint32_t n_ev;
	int16_t rx, ry, rw, rh;
	int32_t dt_win;
	uint32_t flags;
	uint32_t flow_idx;
};
static_assert(sizeof(Rec) == 28, "Unit layout");
constexpr uint32_t kActive = 1u, kStray = 2u;

std::vector<uint32_t> table(const std::vector<Rec>& r, int kind)
{
	std::vector<uint32_t> order(r.size(), 0xffffffffu);
	ebo::fill_launch_order(r.empty() ? nullptr : &r[0].n_ev, r.empty() ? nullptr : &r[0].flags, sizeof(Rec), r.size(), kActive,
						   order.data(), static_cast<ebo::LaunchOrderKind>(kind));
	return order;
}

uint32_t key(const Rec& r) { return (r.flags & kActive) ? r.n_ev : 0u; }

// a permutation; keys non-increasing (kind 0) / non-decreasing (2); equal keys in index order; kind 1 the identity
bool check(const std::vector<Rec>& r, int kind, const char* what)
{
	const std::vector<uint32_t> o = table(r, kind);
	std::vector<char> seen(r.size(), 0);
	for (size_t q = 0; q < o.size(); ++q)
	{
		if (o[q] >= r.size() || seen[o[q]])
		{
			std::fprintf(stderr, "%s kind %d: not a permutation at %zu\n", what, kind, q);
			return false;
		}
		seen[o[q]] = 1;
		if (kind == 1 && o[q] != q)
		{
			std::fprintf(stderr, "%s: the index order is not the identity at %zu\n", what, q);
			return false;
		}
		if (q && kind != 1)
		{
			const uint32_t a = key(r[o[q - 1]]), b = key(r[o[q]]);
			if ((kind == 0 ? a < b : a > b) || (a == b && o[q - 1] > o[q]))
			{
				std::fprintf(stderr, "%s kind %d: out of order at %zu\n", what, kind, q);
				return false;
			}
		}
	}
	return true;
}

Rec rec(uint32_t n, uint32_t flags)
{
	Rec r;
	std::memset(&r, 0, sizeof r);
	r.n_ev = n;
	r.flags = flags;
	return r;
}

int self_test()
{
	bool ok = true;
	for (int kind = 0; kind < 3; ++kind)
	{
		ok = check({}, kind, "n = 0") && ok;
		ok = check({rec(7, kActive)}, kind, "n = 1") && ok;
		ok = check(std::vector<Rec>(300, rec(64, kActive)), kind, "all equal") && ok;
		std::vector<Rec> sorted, mixed;
		for (uint32_t i = 0; i < 500; ++i)
		{
			sorted.push_back(rec(1000 - i, kActive));
		}
		ok = check(sorted, kind, "already sorted") && ok;
		// inactive units keep their n_ev (n_ev <= min_events) and a stray unit may hold many events: both key 0
		for (uint32_t i = 0; i < 257; ++i)
		{
			mixed.push_back(rec(i % 9 == 0 ? 5000 + i : i % 40, i % 9 == 0 ? kStray : (i % 40 > 12 ? kActive : 0u)));
		}
		ok = check(mixed, kind, "mixed") && ok;
		std::vector<Rec> big;
		uint64_t s = 0x9e3779b97f4a7c15ull;
		for (uint32_t i = 0; i < 40000; ++i)
		{
			s = s * 6364136223846793005ull + 1442695040888963407ull;
			const uint32_t n = static_cast<uint32_t>(s >> 33) % 2000;
			big.push_back(rec(n, (i % 257 == 256) ? kStray : (n > 30 ? kActive : 0u)));
		}
		ok = check(big, kind, "40000 random") && ok;
	}
	// inactive and stray units come last, in index order
	{
		const std::vector<Rec> r = {rec(900, kStray), rec(3, 0u), rec(40, kActive), rec(2000, kActive), rec(0, 0u), rec(40, kActive)};
		const uint32_t want[6] = {3, 2, 5, 0, 1, 4};
		const std::vector<uint32_t> o = table(r, 0);
		for (int i = 0; i < 6; ++i)
		{
			if (o[i] != want[i])
			{
				std::fprintf(stderr, "inactive / stray last: entry %d is %u, not %u\n", i, o[i], want[i]);
				ok = false;
			}
		}
	}
	std::puts(ok ? "ok" : "FAILED");
	return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc > 1 && std::strcmp(argv[1], "self") == 0)
	{
		return self_test();
	}
	int kind = 0;
	size_t n = 0;
	if (std::scanf("%d %zu", &kind, &n) != 2)
	{
		return 2;
	}
	std::vector<Rec> r(n);
	for (size_t i = 0; i < n; ++i)
	{
		unsigned a = 0, f = 0;
		if (std::scanf("%u %u", &a, &f) != 2)
		{
			return 2;
		}
		r[i] = rec(a, f);
	}
	for (uint32_t v : table(r, kind))
	{
		std::printf("%u\n", v);
	}
	return 0;
}
