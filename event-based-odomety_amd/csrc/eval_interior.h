// eval_interior.h -- which units k_eval3 evaluates without a per-event reject, row or clip test (eval_unit3, DESIGN.md 4.1
// item 20).  Header-only and free of HIP, so that the rule is pinned by a CPU test against an event-by-event restatement
// (tests/cpp/eval_interior_test.cpp) and the kernel only applies it.
//
// Every event of the three event passes (the deal's key loop, the scatter, the gather) pays for warp_event's two
// `convertible` tests and four canvas tests, the sub-band's row test and the `interior` test that chooses between the
// unpredicated and the clipped tap loops.  For a unit the rule admits, all of them answer the same for every event, and the
// answer is known once the box is:
//
//   * no event is rejected.  The box came from the extents table, i.e. box_admits held (box_extents.h): every candidate is
//     convertible, so every event is (its coordinate lies between its column's two candidates), and the extremes lie inside
//     the canvas grown by the three-tap margin, so the canvas test rejects none.  Every event is then accepted, and
//     [xmin, xmax] x [ymin, ymax] is the exact range of the centre taps (pxc, pyc) of ALL the unit's events.
//   * the canvas does not cut the box.  xmin >= 3 and xmax <= 3 rw - 4 leave the clamps of x0 = max(xmin - 3, 0) and
//     x1 = min(xmax + 3, 3 rw - 1) idle: x0 = xmin - 3 and bw = x1 - x0 + 1 = xmax - xmin + 7.  So for every event
//     colLo = pxc - 3 - x0 = pxc - xmin >= 0 and colLo + 6 = pxc - xmin + 6 <= xmax - xmin + 6 = bw - 1.  Likewise
//     y0 = ymin - 3 and rowsAll = ymax - ymin + 7.
//   * one row tile and one sub-band.  tiles == 1 makes the tile [y0, y1]; rowsAll <= maxRows makes the sub-band loop run
//     once with sy0 = y0 and srows = rowsAll.  So for every event rowLo = pyc - 3 - sy0 = pyc - ymin >= 0 and
//     rowLo + 6 <= ymax - ymin + 6 = srows - 1: the row test (rowLo + 6 < 0 || rowLo >= srows) skips none, and
//     interior = rowLo >= 0 && rowLo + 6 < srows && colLo >= 0 && colLo + 6 < bw is true for every event.
//
// The unpredicated tap loops then touch words [rowLo * cols + colLo, (rowLo + 6) * cols + colLo + 6] with cols >= bw, all
// below srows * cols <= capDoubles.  A unit whose box comes from the event pass is never admitted: that pass does not
// know whether an event was rejected.
#pragma once

#ifdef __HIPCC__
#define EBO_INTERIOR_HD __host__ __device__
#else
#define EBO_INTERIOR_HD
#endif

namespace ebo
{
// tabled: the box [xmin, xmax] x [ymin, ymax] came from the extents table (box_from_extents / box_from_slot returned
// true); tiles: row tiles of the launch; rw, rh: the unit's rect (the canvas is 3 rw x 3 rh); rowsAll, maxRows: the rows
// of the box's image and the rows one sub-band holds, as eval_unit3 has them.
inline EBO_INTERIOR_HD bool unit_all_interior(bool tabled, int tiles, int xmin, int xmax, int ymin, int ymax, int rw, int rh,
											   int rowsAll, int maxRows)
{
	return tabled && tiles == 1 && xmin >= 3 && xmax <= 3 * rw - 4 && ymin >= 3 && ymax <= 3 * rh - 4 && rowsAll <= maxRows;
}
}  // namespace ebo
