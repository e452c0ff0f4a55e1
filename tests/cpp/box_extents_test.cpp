// box_extents_test.cpp — csrc/box_extents.h on the host: the bounding box of a unit's warped events taken from its
// per-column / per-row time extents against a brute-force loop over the events with warp_event's statements.
//   * whenever the rule admits the table, its box EQUALS the brute-force box;
//   * whenever brute force finds a rejected event (not convertible, or off the canvas), the rule refuses.
// Random units: rw, rh in 1 .. 64, 1 .. 2000 events, empty columns and rows, signed dt up to the int32 limits; flows
// positive, negative, zero on one axis, tiny, huge, +-inf and NaN, and flows sized to push the box onto the canvas
// border.  Built with -ffp-contract=off, as the kernels are.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../event-based-odomety_amd/csrc/box_extents.h"

using namespace ebo;

namespace
{
struct Ev
{
	int x, y, dt;
};

// k_unit_extents, serially
bool build_slot(const std::vector<Ev>& ev, int rx, int ry, int rw, int rh, std::vector<int32_t>& slot)
{
	slot.assign(kExtStride, 0);
	for (int i = kExtEntries; i < kExtStride; ++i)
	{
		slot[i] = (i & 1) ? kExtEmptyMax : kExtEmptyMin;
	}
	bool inside = rw <= kExtMaxSide && rh <= kExtMaxSide;
	int32_t* e = slot.data() + kExtEntries;
	for (const Ev& v : ev)
	{
		const int cx = v.x - rx, cy = v.y - ry;
		if (cx < 0 || cx >= rw || cy < 0 || cy >= rh)
		{
			inside = false;
			continue;
		}
		e[2 * cx] = std::min(e[2 * cx], v.dt);
		e[2 * cx + 1] = std::max(e[2 * cx + 1], v.dt);
		e[2 * (rw + cy)] = std::min(e[2 * (rw + cy)], v.dt);
		e[2 * (rw + cy) + 1] = std::max(e[2 * (rw + cy) + 1], v.dt);
	}
	slot[0] = inside ? kExtValid : kExtNone;
	return inside;
}

// warp_event (ebo_kernels.hip), statement for statement, over every event: the box of the accepted ones and the number
// of rejected ones
int brute(const std::vector<Ev>& ev, int rx, int ry, int rw, int rh, double scale, double m0, double m1, int& xmin, int& xmax,
		  int& ymin, int& ymax)
{
	xmin = ymin = 0x7fffffff;
	xmax = ymax = -0x7fffffff;
	int rejected = 0;
	for (const Ev& v : ev)
	{
		const double tau = static_cast<double>(v.dt) * scale;
		const double cx = static_cast<double>(v.x) + tau * m0;
		const double cy = static_cast<double>(v.y) + tau * m1;
		if (!(std::fabs(cx) < 1073741824.0) || !(std::fabs(cy) < 1073741824.0))
		{
			++rejected;
			continue;
		}
		const int bx = static_cast<int>(cx);
		const int by = static_cast<int>(cy);
		const int pxc = bx - rx + rw;
		const int pyc = by - ry + rh;
		if (pxc + 3 < 0 || pxc - 3 >= 3 * rw || pyc + 3 < 0 || pyc - 3 >= 3 * rh)
		{
			++rejected;
			continue;
		}
		xmin = std::min(xmin, pxc);
		xmax = std::max(xmax, pxc);
		ymin = std::min(ymin, pyc);
		ymax = std::max(ymax, pyc);
	}
	return rejected;
}

int g_fail = 0;
#define CHECK(cond, ...)                  \
	do                                    \
	{                                     \
		if (!(cond))                      \
		{                                 \
			if (++g_fail <= 20)           \
			{                             \
				std::printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
				std::printf(__VA_ARGS__); \
				std::printf("\n");        \
			}                             \
		}                                 \
	} while (0)
}  // namespace

int main()
{
	std::mt19937_64 rng(20240917);
	auto uni = [&](int lo, int hi) { return static_cast<int>(std::uniform_int_distribution<int64_t>(lo, hi)(rng)); };
	const double inf = std::numeric_limits<double>::infinity();
	const double nan = std::numeric_limits<double>::quiet_NaN();
	long admitted = 0, refused = 0, refusedClean = 0, withRejected = 0, cases = 0, emptyCols = 0;
	for (int unit = 0; unit < 400; ++unit)
	{
		const int rw = unit < 8 ? (unit & 1 ? 64 : 1) : uni(1, 64);
		const int rh = unit < 8 ? (unit & 2 ? 64 : 1) : uni(1, 64);
		const int rx = uni(-200, 16000), ry = uni(-200, 16000);
		const int n = unit < 16 ? 1 + unit % 3 : uni(1, 2000);
		// the time range of the unit: a few ms either side of the reference time for most, the int32 limits for some
		const int span = unit % 7 == 0 ? 0x7fffffff : uni(1, 40000);
		const int keepCols = uni(1, rw), keepRows = uni(1, rh);  // events land on a subset of the columns and rows
		std::vector<int> cols(keepCols), rows(keepRows);
		for (int& cidx : cols) cidx = uni(0, rw - 1);
		for (int& ridx : rows) ridx = uni(0, rh - 1);
		std::vector<Ev> ev(n);
		for (Ev& v : ev)
		{
			v.x = rx + cols[uni(0, keepCols - 1)];
			v.y = ry + rows[uni(0, keepRows - 1)];
			v.dt = span == 0x7fffffff ? uni(-0x7fffffff - 1, 0x7fffffff) : uni(-span, span);
			if (unit % 5 == 1)
			{
				v.dt = v.dt < -0x7fffffff ? 0x7fffffff : std::abs(v.dt);  // one-sided: the window's reference time at its end
			}
		}
		std::vector<int32_t> slot;
		const bool valid = build_slot(ev, rx, ry, rw, rh, slot);
		CHECK(valid, "unit %d: every event lies inside its rect", unit);
		for (int i = 0; i < rw; ++i)
		{
			emptyCols += slot[kExtEntries + 2 * i] > slot[kExtEntries + 2 * i + 1];
		}
		const double scale = unit % 3 == 0 ? 1e-6 : 1e-3;
		const double reach = static_cast<double>(span == 0x7fffffff ? 0x7fffffff : span) * scale;  // |tau| at the far end
		// flows: fixed kinds, then multiples of (patch size / reach) that carry the far events to and past the border
		std::vector<std::pair<double, double>> flows = {
			{0.0, 0.0}, {0.3, 0.2}, {-0.3, -0.7}, {0.4, -0.1}, {0.0, 0.5}, {-0.5, 0.0}, {1e-300, -1e-300}, {1e-12, 1e-9},
			{5e-324, 0.1}, {1e6, 1e6}, {-1e12, 3.0}, {1e300, -1e300}, {inf, 0.0}, {0.0, -inf}, {-inf, inf}, {nan, 0.1},
			{0.2, nan}, {nan, nan}, {-0.0, -0.0}};
		for (double k : {0.25, 0.9, 1.0, 1.04, 1.1, 1.5, 2.0, 3.0})
		{
			const double fx = k * rw / reach, fy = k * rh / reach;
			flows.push_back({fx, 0.1 * fy});
			flows.push_back({-fx, -0.1 * fy});
			flows.push_back({0.1 * fx, fy});
			flows.push_back({-0.1 * fx, -fy});
			flows.push_back({fx, -fy});
		}
		for (const auto& f : flows)
		{
			int bx0, bx1, by0, by1, tx0 = 0, tx1 = 0, ty0 = 0, ty1 = 0;
			const int rejected = brute(ev, rx, ry, rw, rh, scale, f.first, f.second, bx0, bx1, by0, by1);
			const bool ok = box_from_slot(slot.data(), rx, ry, rw, rh, scale, f.first, f.second, tx0, tx1, ty0, ty1);
			++cases;
			withRejected += rejected > 0;
			if (ok)
			{
				++admitted;
				CHECK(rejected == 0, "unit %d flow (%g, %g): admitted with %d rejected events", unit, f.first, f.second, rejected);
				CHECK(tx0 == bx0 && tx1 == bx1 && ty0 == by0 && ty1 == by1,
					  "unit %d (%dx%d, %d ev) flow (%g, %g): table [%d,%d]x[%d,%d] brute [%d,%d]x[%d,%d]", unit, rw, rh, n, f.first,
					  f.second, tx0, tx1, ty0, ty1, bx0, bx1, by0, by1);
			}
			else
			{
				++refused;
				refusedClean += rejected == 0;
			}
			CHECK(!(rejected > 0 && ok), "unit %d flow (%g, %g): %d rejected events but the rule admits", unit, f.first, f.second,
				  rejected);
		}
		// a slot without a table is refused at any flow
		slot[0] = kExtNone;
		int a, b, cidx, d;
		CHECK(!box_from_slot(slot.data(), rx, ry, rw, rh, scale, 0.0, 0.0, a, b, cidx, d), "unit %d: no table, yet admitted", unit);
	}
	// an event outside the rect, or a rect wider than the table: no table
	{
		std::vector<int32_t> slot;
		CHECK(!build_slot({{5, 5, 10}, {16, 5, 3}}, 0, 0, 16, 16, slot) && slot[0] == kExtNone, "event outside the rect");
		CHECK(!build_slot({{5, 5, 10}}, 0, 0, 65, 16, slot) && slot[0] == kExtNone, "rect wider than the table");
	}
	std::printf("%ld cases: %ld admitted, %ld refused (%ld of them with no rejected event), %ld with rejected events; %ld empty columns\n",
				cases, admitted, refused, refusedClean, withRejected, emptyCols);
	// the test must exercise both sides of the rule
	CHECK(admitted > cases / 4, "too few admitted cases");
	CHECK(withRejected > cases / 20, "too few cases with rejected events");
	CHECK(emptyCols > 0, "no empty column");
	if (g_fail)
	{
		std::printf("%d check(s) failed\n", g_fail);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
