// count_plan.h -- which kernel draws an integer count image (ebo_count_image*: the reference's final loop,
// integrateEvents, the float-field compensateEvents) for a given shape, with its grid, block, LDS and geometry.
// Header-only and free of HIP, so that the choice is a table the CPU test-suite pins (tests/cpp/count_plan_test.cpp,
// tests/test_count_plan.py) and launch_count_image (ebo_kernels.hip) only launches what the plan says.  The plan reads
// no environment: count_device (ebo_api.cpp) reads the A/B switches (ab_env.h) into the shape.
//
// The default paths, tried in this order:
//   kCountTiles      k_count_tiles (+ k_count_stray)   warped (mode 1), enough (tile, window) workgroups
//   kCountUnits      k_count_units<U16>                 warped, several bands and enough (band, window) workgroups
//   kCountWindowLds  k_count_window_lds<U16, MODE>      warped / field (modes 1, 2), <= 4 bands, >= 64 workgroups
//   kCountSorted     k_csort_hist<MODE>, k_csort_scan,  warped / field with >= 8 M events in the launch
//                    k_csort_scatter, k_csort_count<U16>
//   kCountBands      k_count_bands<U16>                 un-warped image (mode 0)
//   kCountScatter    k_count_scatter + k_counts_to_f64  everything else (global int atomics)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace ebo
{
constexpr int kSortChunk = 4096;  // events per workgroup step of the sorted-bands passes (256 lanes x 16)

enum CountKind
{
	kCountTiles,
	kCountUnits,
	kCountWindowLds,
	kCountSorted,
	kCountBands,
	kCountScatter,
};

struct CountShape
{
	int mode = 0;                    // EBO_COUNT_*
	int image_w = 0, image_h = 0;
	int patch_w = 0, patch_h = 0;
	int npx = 0, npy = 0;
	int windows = 0;
	int units = 0;                   // patch units + stray units of all windows
	uint64_t max_window_events = 0;  // the largest window's events
	size_t total_events = 0;         // all windows' events (packed back to back: the extent of the event buffer)
	bool any_stray = false;          // some window has events outside the sensor
	// A/B overrides (ab_env.h; constant in the shipped build)
	int impl = -1;                   // EBO_COUNT_IMPL: -1 auto, 0 global atomics, 1 whole-window LDS, 2 patch-row bands,
	                                 // 3 sorted bands, 4 unit waves, 5 tiles
	int lds_kb = 0;                  // EBO_COUNT_LDS_KB (<= 160): LDS per band / tile workgroup, 0 = the path's default
	size_t tile_w = 0, tile_h = 0;   // EBO_COUNT_TILE_W / _H: tile pitch, both > 0 to force
	int block = 0;                   // EBO_COUNT_BLOCK: tile workgroup size (a multiple of 64 in [64, 1024]), 0 = default
	int col_tiles = 0;               // EBO_COUNT_COLTILES: 1 = no column tiles in the patch-row bands
};

struct CountPlan
{
	CountKind kind = kCountScatter;
	bool u16 = false;                // 16-bit counters, two per dword (fewer than 65536 events per window)
	unsigned grid_x = 0, grid_y = 1; // the main kernel's grid
	int block = 256;
	size_t lds = 0;                  // dynamic LDS bytes of the main kernel
	// kCountTiles: tile pitch and grid, counter bytes of a full tile, k_count_stray after it
	int tile_w = 0, tile_h = 0, tiles_x = 0, tiles_y = 0, tile_bytes = 0;
	bool stray = false;
	// kCountUnits, kCountWindowLds, kCountSorted: row bands of the image
	int rows_per_band = 0, bands = 0;
	// kCountBands: patch rows per band, regular bands, column tiles
	int prb = 0, n_regular = 0, col_tiles = 0;
	// kCountSorted: bins (windows x bands), event chunks per window, LDS of the histogram and scatter passes, and
	// the entries of the destination list (two halves of total_events each)
	int bins = 0;
	unsigned chunks = 0;
	size_t lds_hist = 0, lds_scatter = 0;
	size_t list_events = 0;
	// kCountScatter: workgroups of the int32 -> f64 conversion
	int convert_blocks = 0;
};

inline CountPlan plan_count_image(const CountShape& S)
{
	CountPlan p;
	// Unit waves over 2-D tiles (impl 5, k_count_tiles): the default for images warped by per-patch
	// flows (mode 1) that do not fit one workgroup's counters, in launches with enough workgroups.
	// Tile grid: the split (counters + unit headers <= 76 KB: two workgroups per CU, so that one's
	// store phase overlaps the other's event phase) that minimises the expected number of tiles a
	// unit visits.
	if ((S.impl == 5 || (S.impl < 0 && S.mode == 1)) && S.mode == 1 && S.units > 0)
	{
		const int b = 2;  // 16-bit counters; a workgroup that cannot prove them safe counts its tile in two 32-bit halves
		const int Pn = S.npx * S.npy;
		const size_t ctlBytes = static_cast<size_t>(Pn + 1) * 16 + 16;  // one 16-byte header per unit the tile may select
		// 76 KB per workgroup (two 1024-lane workgroups per CU) -- except for small sensors, whose whole counter
		// image is little more than that: there four 512-lane workgroups of <= 38 KB per CU overlap their
		// select / wait / store phases better than two large ones (C2, 240x180: 58.8 -> 60.7 % of 8 TB/s; the
		// same split costs C3 and C4 7-10 points: their units straddle the smaller tiles' borders)
		const bool smallSensor = static_cast<size_t>(S.image_w) * S.image_h * b <= 100 * 1024;
		const size_t budgetAll = static_cast<size_t>(S.lds_kb > 0 ? S.lds_kb : (smallSensor ? 38 : 76)) * 1024;
		const size_t budget = budgetAll > ctlBytes + 4096 ? budgetAll - ctlBytes : 4096;
		const int W = S.image_w, H = S.image_h;
		int bestX = 0, bestY = 0, bestW = 0, bestH = 0;
		size_t bestBytes = 0;
		double bestCost = 1e300;
		// EQUAL tiles (balance beats alignment to the patch grid: whole-patch tiles with a larger last
		// tile measured 3-4 points of HBM fraction worse at C3 and C4), even width (two 16-bit
		// counters of a dword never straddle rows), cost = expected tiles a unit visits
		const int pw = S.patch_w, ph = S.patch_h;
		int coarseTiles = 1 << 30;
		for (int tx = 1; tx <= 16 && ctlBytes <= 48 * 1024; ++tx)
		{
			int tw = (W + tx - 1) / tx;
			tw += tw & 1;
			if (tx > 1 && tw * (tx - 1) >= W)
			{
				continue;  // a coarser split covers the image with the same tile width
			}
			const int thMax = static_cast<int>(std::min<size_t>(budget / (static_cast<size_t>(tw) * b), static_cast<size_t>(H)));
			if (thMax < 8)
			{
				continue;
			}
			const int tyMin = (H + thMax - 1) / thMax;
			coarseTiles = std::min(coarseTiles, tx * tyMin);
			const double Rx = 0.5 * pw + 12.0, Ry = 0.5 * ph + 12.0;
			// more, smaller tiles than the LDS asks for when the launch would not fill the chip (two
			// 1024-lane workgroups per CU = 512): the visits a finer split adds against the CUs it wakes
			for (int ty = tyMin; ty <= H / 8; ty = (ty < 4 ? ty + 1 : ty * 2))
			{
				const int th = (H + ty - 1) / ty;
				if (th * (ty - 1) > H)
				{
					continue;  // fewer tiles of this height cover the image: the last ones would start below it
				}
				const double visits = (tx > 1 ? (tw + 2 * Rx) / tw : 1.0) * (ty > 1 ? (th + 2 * Ry) / th : 1.0);
				const double idle = std::max(1.0, 512.0 / (static_cast<double>(S.windows) * tx * ty));
				const double cost = visits * idle;
				if (cost < bestCost - 1e-9)
				{
					bestCost = cost;
					bestX = tx;
					bestY = ty;
					bestW = tw;
					bestH = th;
					bestBytes = (static_cast<size_t>(tw) * th * b + 15) & ~size_t(15);
				}
				if (idle <= 1.0)
				{
					break;  // the chip is full: finer only costs visits
				}
			}
		}
		// eligibility as before the finer splits existed: the coarsest split the LDS allows must already
		// give the launch 64 workgroups (single windows and tiny batches stay with impl 0 / 1)
		// (A/B build: force the tile pitch, e.g. whole patch rows / columns)
		if (S.tile_w > 0 && S.tile_h > 0)
		{
			bestW = static_cast<int>(S.tile_w);
			bestH = static_cast<int>(S.tile_h);
			bestX = (W + bestW - 1) / bestW;
			bestY = (H + bestH - 1) / bestH;
			// the last tile of a row / column takes what is left: size the counters for the largest tile
			const int lastW = W - (bestX - 1) * bestW, lastH = H - (bestY - 1) * bestH;
			bestBytes = (static_cast<size_t>(std::max(bestW, lastW) + 1) * std::max(bestH, lastH) * b + 15) & ~size_t(15);
		}
		const long coarse = static_cast<long>(S.windows) * coarseTiles;
		if (bestX > 0 && (S.impl == 5 || (coarseTiles > 1 && coarse >= 64)))
		{
			const size_t lds = bestBytes + ctlBytes;
			if (lds <= 160 * 1024)
			{
				const int groups = (S.windows + 7) / 8;
				p.kind = kCountTiles;
				p.grid_x = static_cast<unsigned>(groups * bestX * bestY * 8);
				p.block = S.block > 0 ? S.block : (budgetAll <= 38 * 1024 ? 512 : 1024);
				p.lds = lds;
				p.tile_w = bestW;
				p.tile_h = bestH;
				p.tiles_x = bestX;
				p.tiles_y = bestY;
				p.tile_bytes = static_cast<int>(bestBytes);
				p.stray = S.any_stray;
				return p;
			}
		}
	}
	// Unit waves (impl 4, k_count_units): the default for images warped by per-patch flows that
	// need SEVERAL bands, in launches with enough (band, window) workgroups -- C3 x 128 windows
	// 0.179 -> 0.122 ms against impl 1, C4 x 32 0.311 -> 0.231 ms against impl 3; with one band
	// (C2) impl 1 is as fast, small launches are better off with global atomics.
	if ((S.impl == 4 || S.impl < 0) && S.mode == 1 && S.units > 0)
	{
		const bool u16 = S.max_window_events < 65536;
		const int Pn = S.npx * S.npy;
		const size_t ctlBytes = static_cast<size_t>(Pn + 3) * 4 + 16;
		// 76 KB: two workgroups per CU, so that one's store phase overlaps the other's event phase
		// (C3: 0.122 -> 0.101 ms against 128 KB bands, C4: 0.228 -> 0.211 ms)
		const size_t ldsWant = static_cast<size_t>(S.lds_kb > 0 ? S.lds_kb : 76) * 1024;
		const size_t ldsBytes = std::min(ldsWant, static_cast<size_t>(160 * 1024 - 1024) - std::min(ctlBytes, static_cast<size_t>(64 * 1024)));
		const size_t pxPerBand = u16 ? ldsBytes / 2 : ldsBytes / 4;
		const int rowsMax = static_cast<int>(std::min<size_t>(pxPerBand / S.image_w, S.image_h));
		if (rowsMax > 0 && ctlBytes <= 64 * 1024)
		{
			// bands of EQUAL height (C2: 86 KB of counters are two bands of 90 rows, not 158 + 22:
			// 0.235 -> 0.176 ms, and better than the single 86 KB band of impl 1, 0.194 ms, which
			// leaves room for one workgroup per CU only)
			const int bands = (S.image_h + rowsMax - 1) / rowsMax;
			const int rowsPerBand = (S.image_h + bands - 1) / bands;
			const bool want4 = S.impl == 4 || (bands > 1 && bands <= 64 && static_cast<long>(S.windows) * bands >= 64);
			const size_t lds = ((static_cast<size_t>(rowsPerBand) * S.image_w * (u16 ? 2 : 4) + 15) & ~size_t(15)) + ctlBytes;
			if (want4 && lds <= 160 * 1024)
			{
				const int groups = (S.windows + 7) / 8;
				p.kind = kCountUnits;
				p.u16 = u16;
				p.grid_x = static_cast<unsigned>(groups * bands * 8);
				p.block = 1024;
				p.lds = lds;
				p.rows_per_band = rowsPerBand;
				p.bands = bands;
				return p;
			}
		}
	}
	// LDS-privatised path when the image splits into few row bands and there are
	// enough (band, window) workgroups to occupy the chip; else global int atomics.
	if (S.mode != 0)
	{
		const bool u16 = S.max_window_events < 65536;
		const int Pn = S.npx * S.npy;
		// unit table behind the counters: flows [P][2] f64 (mode 1) + dt_win [P + 1] i32
		const size_t tblBytes = (S.mode == 1 ? static_cast<size_t>(Pn) * 16 : 0) + static_cast<size_t>(Pn + 1) * 4 + 16;
		const size_t ldsWant = static_cast<size_t>(S.lds_kb > 0 ? S.lds_kb : 128) * 1024;
		const size_t ldsBytes = std::min(ldsWant, static_cast<size_t>(160 * 1024 - 1024) - std::min(tblBytes, static_cast<size_t>(96 * 1024)));
		const size_t pxPerBand = u16 ? ldsBytes / 2 : ldsBytes / 4;
		const int rowsPerBand = static_cast<int>(std::min<size_t>(pxPerBand / S.image_w, S.image_h));
		const int bands = rowsPerBand > 0 ? (S.image_h + rowsPerBand - 1) / rowsPerBand : 1 << 30;
		const bool tableFits = tblBytes <= 64 * 1024;  // finer grids: the other implementations
		const bool want = tableFits && (S.impl == 1 || (S.impl < 0 && bands <= 4 && S.windows * bands >= 64));
		if (want && rowsPerBand > 0 && S.units > 0)
		{
			// (<= 160 KB: the counters take at most ldsBytes, the table at most 64 KB of the rest)
			const int groups = (S.windows + 7) / 8;  // 8 windows (one per XCD) x bands slots each
			p.kind = kCountWindowLds;
			p.u16 = u16;
			p.grid_x = static_cast<unsigned>(groups * bands * 8);
			p.block = 1024;
			p.lds = ((static_cast<size_t>(rowsPerBand) * S.image_w * (u16 ? 2 : 4) + 15) & ~size_t(15)) + tblBytes;
			p.rows_per_band = rowsPerBand;
			p.bands = bands;
			return p;
		}
	}
	// Sorted bands (impl 3): warped images of sensors too large for the whole-window LDS image.
	// Three passes over the events pay off once the launch holds several million of them
	// (C4 x 32 windows: 0.53 ms against 0.83 ms of global atomics; C4 x 2: 0.064 against 0.058).
	const bool manyEvents = static_cast<size_t>(S.windows) * S.max_window_events >= (size_t(8) << 20);
	if ((S.impl == 3 || (S.impl < 0 && manyEvents)) && S.units > 0 && S.mode != 0)
	{
		const bool u16 = S.max_window_events < 65536;
		const size_t ldsBytes = static_cast<size_t>(S.lds_kb > 0 ? S.lds_kb : 24) * 1024;
		const size_t rowBytes = static_cast<size_t>(S.image_w) * (u16 ? 2 : 4);
		const int rowsPerBand = static_cast<int>(std::min<size_t>(std::max<size_t>(ldsBytes / rowBytes, 1), S.image_h));
		const int bands = (S.image_h + rowsPerBand - 1) / rowsPerBand;
		const size_t lds = (static_cast<size_t>(rowsPerBand) * rowBytes + 3) & ~size_t(3);
		if (lds <= 160 * 1024 - 512 && bands <= 4096)
		{
			p.kind = kCountSorted;
			p.u16 = u16;
			p.grid_x = static_cast<unsigned>(bands);
			p.grid_y = static_cast<unsigned>(S.windows);
			p.block = 512;
			p.lds = lds;
			p.rows_per_band = rowsPerBand;
			p.bands = bands;
			p.bins = bands * S.windows;
			p.chunks = std::max(static_cast<unsigned>((S.max_window_events + kSortChunk - 1) / kSortChunk), 1u);
			p.lds_hist = static_cast<size_t>(bands) * sizeof(unsigned int);
			p.lds_scatter = 4 * p.lds_hist + kSortChunk * (sizeof(unsigned int) + sizeof(unsigned short));
			p.list_events = S.total_events;
			return p;
		}
	}
	// Patch-row bands (impl 2): any image size, no event read twice.  The default for the
	// un-warped image, whose events never leave their band (4.3 TB/s at C2, 3.9 at C3, 2.7 at C4).
	if ((S.impl == 2 || S.impl < 0) && S.mode == 0 && S.units > 0)
	{
		const bool u16 = S.max_window_events < 65536;
		const size_t rowBytes = static_cast<size_t>(S.image_w) * (u16 ? 2 : 4);
		size_t ldsBytes = static_cast<size_t>(S.lds_kb) * 1024;
		if (S.lds_kb <= 0)
		{
			// un-warped image, measured: ONE patch row per band when it is up to 24 KB of counters
			// (C2 10.5 KB: 63 -> 67 % of HBM against two rows; C3 22 KB: 71 %), column tiles of
			// ~16 KB above that (C4: 64 -> 68 % against 24 KB tiles); several rows only when a
			// patch row is tiny
			const size_t patchRowBytes = static_cast<size_t>(S.patch_h) * rowBytes;
			ldsBytes = patchRowBytes > 24 * 1024 ? 16 * 1024 : std::max<size_t>(patchRowBytes, 12 * 1024);
		}
		const int prb = std::max(1, static_cast<int>(ldsBytes / rowBytes) / S.patch_h);
		const int bandRows = prb * S.patch_h;
		// One patch row already above the target (large sensors; C4: 22 rows x 1280 x 4 B = 112 KB,
		// one workgroup per CU): cut it into column tiles of whole patches.
		int colTiles = 1;
		size_t tileRowBytes = rowBytes;
		if (static_cast<size_t>(S.patch_h) * rowBytes > ldsBytes && S.npx > 1)
		{
			const size_t pxBytes = u16 ? 2 : 4;
			const int unitsPerTile = std::max<int>(1, static_cast<int>(ldsBytes / (static_cast<size_t>(bandRows) * pxBytes)) / S.patch_w);
			colTiles = (S.npx + unitsPerTile - 1) / unitsPerTile;
			const int perTile = (S.npx + colTiles - 1) / colTiles;  // as the kernel divides them
			const int lastLo = std::min((colTiles - 1) * perTile, S.npx - 1);
			const int widest = std::max(perTile * S.patch_w, S.image_w - lastLo * S.patch_w);
			tileRowBytes = static_cast<size_t>(widest) * pxBytes;
		}
		if (S.col_tiles == 1)  // A/B: 1 = off
		{
			colTiles = 1;
			tileRowBytes = rowBytes;
		}
		const size_t lds = (static_cast<size_t>(bandRows) * tileRowBytes + 3) & ~size_t(3);
		if (lds <= 160 * 1024 - 512)
		{
			const int nRegular = (S.npy - 1 + prb - 1) / prb;
			const int tallest = S.image_h - (S.npy - 1) * S.patch_h;
			const int nSub = (tallest + bandRows - 1) / bandRows;
			p.kind = kCountBands;
			p.u16 = u16;
			p.grid_x = static_cast<unsigned>((nRegular + nSub) * colTiles);
			p.grid_y = static_cast<unsigned>(S.windows);
			p.block = 512;
			p.lds = lds;
			p.prb = prb;
			p.n_regular = nRegular;
			p.col_tiles = colTiles;
			return p;
		}
	}
	// Global int atomics into the int32 scratch image, then one conversion pass to f64.
	const size_t n = static_cast<size_t>(S.windows) * S.image_w * S.image_h;
	p.kind = kCountScatter;
	p.grid_x = static_cast<unsigned>(S.units);
	p.block = 256;
	p.convert_blocks = static_cast<int>(std::min<size_t>((n + 255) / 256, 2048));
	return p;
}
}  // namespace ebo
