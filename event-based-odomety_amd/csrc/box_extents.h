// box_extents.h — the bounding box of a unit's warped events from per-column and per-row time extents
// (free of HIP: tests/cpp/box_extents_test.cpp).
//
// k_eval3's image covers the bounding box of the centre taps of the unit's warped events.  For a fixed integer source
// column x the warped canvas column
//     trunc(fl(double(x) + fl(fl(double(dt) * scale) * m0))) - rx + rw
// is MONOTONE in dt -- non-decreasing or non-increasing by the sign of scale * m0 -- because every rounding and the
// truncation are monotone.  So the extreme warped columns of a unit are attained at the smallest and the largest dt of
// each source column, likewise the rows: 2 (rw + rh) candidates instead of a pass over the events.  The extents depend
// on the loaded events only, never on the flow: k_unit_extents builds them once per load (ebo_extents.inc).
//
// The two axes separate only while warp_event rejects no event of the unit (a rejected event drops out of BOTH axes'
// extremes).  box_admits is the test for that: every candidate convertible (then every event is: its coordinate lies
// between its column's two candidates) and the extremes inside the canvas grown by the three-tap margin warp_event
// allows.  Then each extreme is attained by a real, accepted event and the box EQUALS the event pass's.  Otherwise the
// event pass runs.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define EBO_BOX_HD __host__ __device__
#else
#define EBO_BOX_HD
#endif

namespace ebo
{
// One slot per unit in d_unit_ext (int32): status | pad | [dtMin, dtMax] of columns 0 .. rw-1 | of rows 0 .. rh-1.
// dt is the signed int as unpack yields it; an empty column or row holds (INT_MAX, INT_MIN).
constexpr int kExtMaxSide = 64;                    // units with rw or rh above it have no table
constexpr int kExtEntries = 2;                     // first entry's offset in the slot: pairs stay 8-byte aligned
constexpr int kExtStride = kExtEntries + 4 * kExtMaxSide;  // ints per slot
constexpr int32_t kExtNone = 0;                    // status: stray, too wide or tall, or an event outside the rect
constexpr int32_t kExtValid = 1;
constexpr int32_t kExtEmptyMin = 0x7fffffff;
constexpr int32_t kExtEmptyMax = -0x7fffffff - 1;

// warp_event's statements for one axis: source coordinate v, time offset dt, flow component m -> canvas coordinate p
// of the centre tap (origin / side: rx, rw or ry, rh).  false: not convertible.  Not fused: -ffp-contract=off.
inline EBO_BOX_HD bool box_candidate(int v, int dt, double scale, double m, int origin, int side, int& p)
{
	const double tau = static_cast<double>(dt) * scale;
	const double cc = static_cast<double>(v) + tau * m;
	const double mag = cc < 0.0 ? -cc : cc;
	if (!(mag < 1073741824.0))
	{
		return false;
	}
	p = static_cast<int>(cc) - origin + side;
	return true;
}

// One table entry's contribution: both ends of its time extent are warped and the smaller and the larger result
// taken, so the sign of scale * m never has to be looked at.
inline EBO_BOX_HD void box_entry(int v, int dtMin, int dtMax, double scale, double m, int origin, int side, int& lo,
								 int& hi, bool& ok)
{
	if (dtMin > dtMax)
	{
		return;  // no event in this column / row
	}
	int a, b;
	if (!box_candidate(v, dtMin, scale, m, origin, side, a) || !box_candidate(v, dtMax, scale, m, origin, side, b))
	{
		ok = false;
		return;
	}
	lo = a < lo ? a : lo;
	lo = b < lo ? b : lo;
	hi = a > hi ? a : hi;
	hi = b > hi ? b : hi;
}

// Under these bounds warp_event's canvas test (pxc + 3 < 0 || pxc - 3 >= 3 rw, likewise rows) rejects no event.
inline EBO_BOX_HD bool box_admits(bool ok, int xmin, int xmax, int ymin, int ymax, int rw, int rh)
{
	return ok && xmin >= -3 && xmax <= 3 * rw + 2 && ymin >= -3 && ymax <= 3 * rh + 2;
}

// The whole rule, serially (the kernels deal the entries over a wave's lanes: ebo_eval3.inc): the box of the unit
// whose slot is `slot` at flow (m0, m1), or false where the event pass has to run.
inline bool box_from_slot(const int32_t* slot, int rx, int ry, int rw, int rh, double scale, double m0, double m1,
						  int& xmin, int& xmax, int& ymin, int& ymax)
{
	if (slot[0] != kExtValid)
	{
		return false;
	}
	bool ok = true;
	xmin = ymin = kExtEmptyMin;
	xmax = ymax = kExtEmptyMax;
	const int32_t* e = slot + kExtEntries;
	for (int i = 0; i < rw; ++i)
	{
		box_entry(rx + i, e[2 * i], e[2 * i + 1], scale, m0, rx, rw, xmin, xmax, ok);
	}
	for (int j = 0; j < rh; ++j)
	{
		box_entry(ry + j, e[2 * (rw + j)], e[2 * (rw + j) + 1], scale, m1, ry, rh, ymin, ymax, ok);
	}
	return box_admits(ok, xmin, xmax, ymin, ymax, rw, rh);
}
}  // namespace ebo
