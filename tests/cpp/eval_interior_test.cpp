// k_eval3's all-interior rule (csrc/eval_interior.h, free of HIP) against a brute-force loop that mirrors, event by event,
// what eval_unit3's passes ask of every event: warp_event (two convertible tests, four canvas tests), the sub-band's row
// test and the interior test that chooses the unpredicated tap loops.  A seeded sweep of units x flows x capacities x row
// tiles: rects of 1 .. 70 pixels a side (above 64 there is no table), events inside the rect and, in some units, one
// outside it (no table), flows from 0 to where boxes leave the canvas and a few that make coordinates unconvertible,
// capacities that hold the box in one sub-band, exactly, and in several.  Wherever the rule admits a unit, the brute force
// must find no rejected, no skipped and no non-interior event, and every tap address of the unpredicated loops inside the
// sub-band's image.  The share of clean cases the rule refuses (its slack) is printed, with no threshold on it.
#include "../../event-based-odomety_amd/csrc/box_extents.h"
#include "../../event-based-odomety_amd/csrc/eval_interior.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
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

struct Event
{
	int x, y, dt;
};

// warp_event's statements (ebo_kernels.hip), one rounding per operation
static bool warp_event(const Event& e, int rx, int ry, int rw, int rh, double scale, double m0, double m1, int& pxc, int& pyc)
{
	const double tau = static_cast<double>(e.dt) * scale;
	const double cx = static_cast<double>(e.x) + tau * m0;
	const double cy = static_cast<double>(e.y) + tau * m1;
	if (!(std::fabs(cx) < 1073741824.0) || !(std::fabs(cy) < 1073741824.0))
	{
		return false;
	}
	pxc = static_cast<int>(cx) - rx + rw;
	pyc = static_cast<int>(cy) - ry + rh;
	return !(pxc + 3 < 0 || pxc - 3 >= 3 * rw || pyc + 3 < 0 || pyc - 3 >= 3 * rh);
}

// k_unit_extents' slot of a unit (ebo_extents.inc): no table for a rect above 64 a side or an event outside the rect
static std::vector<int32_t> make_slot(const std::vector<Event>& ev, int rx, int ry, int rw, int rh)
{
	std::vector<int32_t> s(ebo::kExtStride);
	s[0] = ebo::kExtNone;
	s[1] = 0;
	for (int i = 0; i < 2 * ebo::kExtMaxSide; ++i)
	{
		s[ebo::kExtEntries + 2 * i] = ebo::kExtEmptyMin;
		s[ebo::kExtEntries + 2 * i + 1] = ebo::kExtEmptyMax;
	}
	if (rw > ebo::kExtMaxSide || rh > ebo::kExtMaxSide)
	{
		return s;
	}
	bool inside = true;
	for (const Event& e : ev)
	{
		const int cx = e.x - rx, cy = e.y - ry;
		if (cx < 0 || cx >= rw || cy < 0 || cy >= rh)
		{
			inside = false;
			continue;
		}
		for (int k : {cx, rw + cy})
		{
			int32_t& lo = s[ebo::kExtEntries + 2 * k];
			int32_t& hi = s[ebo::kExtEntries + 2 * k + 1];
			lo = std::min(lo, e.dt);
			hi = std::max(hi, e.dt);
		}
	}
	s[0] = inside ? ebo::kExtValid : ebo::kExtNone;
	return s;
}

struct Tally
{
	long cases = 0, admitted = 0, clean = 0, refusedClean = 0, empty = 0;
};

// one unit at one flow, capacity and number of row tiles: eval_unit3's scalars, the rule, and the brute force
static void check_case(const std::vector<Event>& ev, int rx, int ry, int rw, int rh, double scale, double m0, double m1,
					   int capDoubles, int tiles, Tally& t)
{
	const std::vector<int32_t> slot = make_slot(ev, rx, ry, rw, rh);
	int xmin = 0x7fffffff, xmax = -0x7fffffff, ymin = 0x7fffffff, ymax = -0x7fffffff;
	const bool tabled = ebo::box_from_slot(slot.data(), rx, ry, rw, rh, scale, m0, m1, xmin, xmax, ymin, ymax);
	long rejected = 0;
	if (!tabled)
	{
		xmin = ymin = 0x7fffffff;
		xmax = ymax = -0x7fffffff;
	}
	int exmin = 0x7fffffff, exmax = -0x7fffffff, eymin = 0x7fffffff, eymax = -0x7fffffff;
	for (const Event& e : ev)
	{
		int pxc, pyc;
		if (!warp_event(e, rx, ry, rw, rh, scale, m0, m1, pxc, pyc))
		{
			++rejected;
			continue;
		}
		exmin = std::min(exmin, pxc);
		exmax = std::max(exmax, pxc);
		eymin = std::min(eymin, pyc);
		eymax = std::max(eymax, pyc);
	}
	if (tabled)
	{
		// (box_extents.h's own promise, which the rule builds on)
		CHECK(rejected == 0 && xmin == exmin && xmax == exmax && ymin == eymin && ymax == eymax, "the table's box is not the event pass's");
	}
	else
	{
		xmin = exmin, xmax = exmax, ymin = eymin, ymax = eymax;
	}
	++t.cases;
	if (xmin > xmax)
	{
		++t.empty;  // eval_unit3 returns before the rule is asked
		return;
	}
	const int W3 = 3 * rw, H3 = 3 * rh;
	const int x0 = std::max(xmin - 3, 0), x1 = std::min(xmax + 3, W3 - 1);
	const int y0 = std::max(ymin - 3, 0), y1 = std::min(ymax + 3, H3 - 1);
	const int bw = x1 - x0 + 1;
	const int cols = ((bw | 1) <= capDoubles) ? (bw | 1) : bw;
	const int rowsAll = y1 - y0 + 1;
	const int maxRows = std::max(capDoubles / cols, 1);
	const bool rule = ebo::unit_all_interior(tabled, tiles, xmin, xmax, ymin, ymax, rw, rh, rowsAll, maxRows);

	// the brute force: every (row tile, sub-band) pass over every event, as the scatter and the gather walk them
	long skipped = 0, clipped = 0, passes = 0, outside = 0;
	const int R = (rowsAll + tiles - 1) / tiles;
	for (int tile = 0; tile < tiles; ++tile)
	{
		const int ty0 = y0 + tile * R, ty1 = std::min(ty0 + R, y1 + 1);
		for (int sy0 = ty0; sy0 < ty1; sy0 += maxRows)
		{
			const int srows = std::min(maxRows, ty1 - sy0);
			++passes;
			for (const Event& e : ev)
			{
				int pxc, pyc;
				if (!warp_event(e, rx, ry, rw, rh, scale, m0, m1, pxc, pyc))
				{
					continue;  // (counted above)
				}
				const int rowLo = pyc - 3 - sy0;
				if (rowLo + 6 < 0 || rowLo >= srows)
				{
					++skipped;
					continue;
				}
				const int colLo = pxc - 3 - x0;
				const bool interior = rowLo >= 0 && rowLo + 6 < srows && colLo >= 0 && colLo + 6 < bw;
				if (!interior)
				{
					++clipped;
				}
				// the words the unpredicated loops would touch
				const long first = static_cast<long>(rowLo) * cols + colLo, last = static_cast<long>(rowLo + 6) * cols + colLo + 6;
				if (first < 0 || last >= static_cast<long>(srows) * cols || static_cast<long>(srows) * cols > std::max(capDoubles, cols))
				{
					++outside;
				}
			}
		}
	}
	const bool clean = rejected == 0 && skipped == 0 && clipped == 0;
	t.clean += clean;
	if (rule)
	{
		++t.admitted;
		CHECK(rejected == 0 && skipped == 0 && clipped == 0 && outside == 0 && passes == 1,
			  "admitted, but rejected %ld skipped %ld clipped %ld outside %ld in %ld passes (rect %d x %d, flow %g %g, cap %d, tiles %d, box %d..%d x %d..%d)",
			  rejected, skipped, clipped, outside, passes, rw, rh, m0, m1, capDoubles, tiles, xmin, xmax, ymin, ymax);
	}
	else if (clean)
	{
		++t.refusedClean;
		CHECK(!tabled, "a clean unit with a table is refused (rect %d x %d, flow %g %g, cap %d, tiles %d)", rw, rh, m0, m1, capDoubles, tiles);
	}
}

// the rule's edges, one argument at a time
static void check_edges()
{
	using ebo::unit_all_interior;
	const int rw = 20, rh = 16;
	CHECK(unit_all_interior(true, 1, 3, 3 * rw - 4, 3, 3 * rh - 4, rw, rh, 40, 40), "the widest admitted box");
	CHECK(!unit_all_interior(false, 1, 3, 3 * rw - 4, 3, 3 * rh - 4, rw, rh, 40, 40), "no table");
	CHECK(!unit_all_interior(true, 2, 3, 3 * rw - 4, 3, 3 * rh - 4, rw, rh, 40, 40), "two row tiles");
	CHECK(!unit_all_interior(true, 1, 2, 3 * rw - 4, 3, 3 * rh - 4, rw, rh, 40, 40), "xmin 2");
	CHECK(!unit_all_interior(true, 1, 3, 3 * rw - 3, 3, 3 * rh - 4, rw, rh, 40, 40), "xmax 3 rw - 3");
	CHECK(!unit_all_interior(true, 1, 3, 3 * rw - 4, 2, 3 * rh - 4, rw, rh, 40, 40), "ymin 2");
	CHECK(!unit_all_interior(true, 1, 3, 3 * rw - 4, 3, 3 * rh - 3, rw, rh, 40, 40), "ymax 3 rh - 3");
	CHECK(!unit_all_interior(true, 1, 3, 3 * rw - 4, 3, 3 * rh - 4, rw, rh, 41, 40), "one row too many");
}

int main()
{
	check_edges();
	std::mt19937_64 rng(20);
	auto uni = [&](int lo, int hi) { return static_cast<int>(lo + rng() % static_cast<uint64_t>(hi - lo + 1)); };
	const double scale = 1e-3;
	Tally t;
	for (int unit = 0; unit < 400; ++unit)
	{
		const int rw = unit % 9 == 0 ? uni(60, 70) : uni(1, 40), rh = unit % 11 == 0 ? uni(60, 70) : uni(1, 40);
		const int rx = uni(0, 300), ry = uni(0, 200);
		const int n = uni(1, 300);
		const int span = unit % 5 == 0 ? 2000 : 25000;  // +- dt in microseconds
		std::vector<Event> ev(n);
		for (Event& e : ev)
		{
			e = {rx + uni(0, rw - 1), ry + uni(0, rh - 1), uni(-span, span)};
		}
		if (unit % 7 == 3)
		{
			ev[uni(0, n - 1)].x = rx + rw;  // one event outside the rect: no table
		}
		for (int f = 0; f < 12; ++f)
		{
			// magnitudes from 0 to 3 rw / tau_max and beyond: boxes grow until they leave the canvas
			const double reach = (f / 8.0) * 1.6 * std::max(rw, rh) / (span * scale);
			double m0 = reach * (uni(-1000, 1000) / 1000.0), m1 = reach * (uni(-1000, 1000) / 1000.0);
			if (f == 11)
			{
				m0 = unit % 2 ? 1e14 : m0;  // unconvertible coordinates
				m1 = unit % 2 ? m1 : -1e14;
			}
			// the capacities: the shipped plans' (eval_plan.h), the box in one sub-band exactly, one row short of it, a few rows
			int xmin, xmax, ymin, ymax;
			int caps[5] = {2542, 4960, 24 * 3 * rw, 0, 0};
			{
				// the box the case will have, for the two capacities cut to it
				int bxmin = 0x7fffffff, bxmax = -0x7fffffff, bymin = 0x7fffffff, bymax = -0x7fffffff;
				for (const Event& e : ev)
				{
					int pxc, pyc;
					if (warp_event(e, rx, ry, rw, rh, scale, m0, m1, pxc, pyc))
					{
						bxmin = std::min(bxmin, pxc), bxmax = std::max(bxmax, pxc), bymin = std::min(bymin, pyc), bymax = std::max(bymax, pyc);
					}
				}
				xmin = bxmin, xmax = bxmax, ymin = bymin, ymax = bymax;
			}
			int ncaps = 3;
			if (xmin <= xmax)
			{
				const int bw = std::min(xmax + 3, 3 * rw - 1) - std::max(xmin - 3, 0) + 1;
				const int rows = std::min(ymax + 3, 3 * rh - 1) - std::max(ymin - 3, 0) + 1;
				caps[3] = (bw | 1) * rows;      // rowsAll == maxRows
				caps[4] = (bw | 1) * rows - 1;  // rowsAll == maxRows + 1 (where there is more than one row)
				ncaps = 5;
			}
			for (int k = 0; k < ncaps; ++k)
			{
				check_case(ev, rx, ry, rw, rh, scale, m0, m1, std::max(caps[k], 1), 1, t);
			}
			check_case(ev, rx, ry, rw, rh, scale, m0, m1, 2542, 2, t);
		}
	}
	std::printf("%ld cases: %ld admitted, %ld clean by brute force, %ld empty; the rule refuses %ld clean cases = %.2f %% of the cases, "
				"%.2f %% of the clean ones (its slack: units without a table)\n",
				t.cases, t.admitted, t.clean, t.empty, t.refusedClean, 100.0 * t.refusedClean / std::max(t.cases, 1L),
				100.0 * t.refusedClean / std::max(t.clean, 1L));
	CHECK(t.cases >= 3000 && t.admitted > t.cases / 10 && t.admitted < t.cases, "the sweep is degenerate: %ld cases, %ld admitted", t.cases, t.admitted);
	if (failures)
	{
		std::printf("%d failure(s)\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
