// The count-image launch plan (csrc/count_plan.h) on the CPU: (a) the full plan of a written-down list of shapes
// against a table, (b) over a grid of modes, sensors, batch sizes and window sizes with default knobs, the kernels
// reached are exactly the ones launch_count_image (csrc/ebo_kernels.hip) can launch, (c) every plan fits the device:
// LDS <= 160 KB, grid > 0, a block of whole waves <= 1024 lanes, every tile of a tile grid starts inside the image.  Run by
// tests/test_count_plan.py.
//   count_plan_test          check (a), (b), (c); prints "all passed"
//   count_plan_test --print  the rows of (a) as the current code plans them (to renew the table on purpose)
#include "../../event-based-odomety_amd/csrc/count_plan.h"

#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace ebo;

namespace
{
struct Geometry
{
	const char* name;
	int w, h, pw, ph;
};

CountShape shape(const Geometry& g, int mode, int windows, uint64_t eventsPerWindow, bool stray = false, int impl = -1,
				 int ldsKb = 0)
{
	CountShape s;
	s.mode = mode;
	s.image_w = g.w;
	s.image_h = g.h;
	s.patch_w = g.pw;
	s.patch_h = g.ph;
	s.npx = g.w / g.pw;
	s.npy = g.h / g.ph;
	s.windows = windows;
	s.units = windows * (s.npx * s.npy + 1);
	s.max_window_events = eventsPerWindow;
	s.total_events = static_cast<size_t>(windows) * eventsPerWindow;
	s.any_stray = stray;
	s.impl = impl;
	s.lds_kb = ldsKb;
	return s;
}

const char* kindName(CountKind k)
{
	switch (k)
	{
	case kCountTiles: return "tiles";
	case kCountUnits: return "units";
	case kCountWindowLds: return "window_lds";
	case kCountSorted: return "sorted";
	case kCountBands: return "bands";
	case kCountScatter: return "scatter";
	}
	return "?";
}

std::string row(const char* label, const CountShape& s)
{
	const CountPlan p = plan_count_image(s);
	char buf[512];
	std::snprintf(buf, sizeof buf,
				  "%s m%d impl%d lds_kb%d: %s u16=%d grid=%u,%u block=%d lds=%zu tile=%d,%d,%d,%d,%d stray=%d band=%d,%d "
				  "prb=%d,%d,%d sort=%d,%u,%zu,%zu,%zu conv=%d",
				  label, s.mode, s.impl, s.lds_kb, kindName(p.kind), p.u16, p.grid_x, p.grid_y, p.block, p.lds, p.tile_w,
				  p.tile_h, p.tiles_x, p.tiles_y, p.tile_bytes, p.stray, p.rows_per_band, p.bands, p.prb, p.n_regular,
				  p.col_tiles, p.bins, p.chunks, p.lds_hist, p.lds_scatter, p.list_events, p.convert_blocks);
	return buf;
}

// The kernels launch_count_image launches for a plan, with their template arguments.
std::vector<std::string> kernels(const CountShape& s, const CountPlan& p)
{
	const std::string u = p.u16 ? "true" : "false", m = std::to_string(s.mode);
	switch (p.kind)
	{
	case kCountTiles:
		return p.stray ? std::vector<std::string>{"k_count_tiles", "k_count_stray"} : std::vector<std::string>{"k_count_tiles"};
	case kCountUnits: return {"k_count_units<" + u + ">"};
	case kCountWindowLds: return {"k_count_window_lds<" + u + "," + m + ">"};
	case kCountSorted:
		return {"k_csort_hist<" + m + ">", "k_csort_scan", "k_csort_scatter", "k_csort_count<" + u + ">"};
	case kCountBands: return {"k_count_bands<" + u + ">"};
	case kCountScatter:
		return p.grid_x > 0 ? std::vector<std::string>{"k_count_scatter", "k_counts_to_f64"} : std::vector<std::string>{"k_counts_to_f64"};
	}
	return {};
}

// Every kernel launch_count_image can launch: the count family of libebo_hip.so.
const std::set<std::string> kLaunchable = {
	"k_count_tiles", "k_count_stray", "k_count_units<true>", "k_count_units<false>", "k_count_window_lds<true,1>",
	"k_count_window_lds<false,1>", "k_count_window_lds<true,2>", "k_count_window_lds<false,2>", "k_csort_hist<1>",
	"k_csort_hist<2>", "k_csort_scan", "k_csort_scatter", "k_csort_count<true>", "k_csort_count<false>",
	"k_count_bands<true>", "k_count_bands<false>", "k_count_scatter", "k_counts_to_f64",
};

// BASELINE.md's configurations (synth.CONFIGS)
const Geometry kC0{"C0", 240, 180, 20, 20}, kC1{"C1", 240, 180, 240, 180}, kC2{"C2", 240, 180, 30, 22},
	kC3{"C3", 346, 260, 21, 16}, kC4{"C4", 1280, 720, 40, 22};

// A shape with every A/B knob a GPU test of tests/test_gpu_count_edges.py sets; the forced tile pitch and block go into
// the row's label (row() prints EBO_COUNT_LDS_KB only).
CountShape edge(const Geometry& g, int mode, int windows, uint64_t n, bool stray, int impl, int ldsKb = 0, int tileW = 0,
				int tileH = 0, int block = 0)
{
	CountShape s = shape(g, mode, windows, n, stray, impl, ldsKb);
	s.tile_w = static_cast<size_t>(tileW);
	s.tile_h = static_cast<size_t>(tileH);
	s.block = block;
	return s;
}

struct EdgeRow
{
	std::string label;
	CountShape s;
};

// count_cases.py's sensors
const Geometry kTieSmall{"ties 241x181/8x6", 241, 181, 8, 6}, kTieWide{"ties 16383x8/32x4", 16383, 8, 32, 4},
	kTieTall{"ties 8x16383/4x32", 8, 16383, 4, 32}, kFine{"ties 240x180/3x3", 240, 180, 3, 3},
	kPile{"64x48/16x12", 64, 48, 16, 12}, kStore{"store 61x43/20x21", 61, 43, 20, 21};

// The store forms: 61 x 43 pixels (odd: the second of three windows starts 8 bytes off a 16-byte boundary) in bands of an
// odd number of rows -- band 0 has an odd pixel count and an aligned start, band 1 an odd start -- on every path that
// stores rows from packed counters: impl 1 and 3 (warped, field), 4 (warped), 2 (un-warped).
std::vector<EdgeRow> storeRows()
{
	std::vector<EdgeRow> rows;
	for (int mode : {1, 2})
	{
		rows.push_back({kStore.name, edge(kStore, mode, 3, 5299, true, 1, 3)});
		rows.push_back({kStore.name, edge(kStore, mode, 3, 5299, true, 3, 3)});
	}
	rows.push_back({kStore.name, edge(kStore, 1, 3, 5299, true, 4, 2)});
	rows.push_back({kStore.name, edge(kStore, 0, 3, 5299, false, 2, 3)});
	return rows;
}

std::vector<EdgeRow> edgeRows()
{
	std::vector<EdgeRow> rows;
	auto add = [&](const std::string& label, const CountShape& s) { rows.push_back({label, s}); };
	auto tiled = [](const char* name, int tw, int th, int block) {
		return std::string(name) + " tile" + std::to_string(tw) + "x" + std::to_string(th) + " block" + std::to_string(block);
	};
	// the tie ladders on every forced path: warped 0, 1, 3, 4, 5 (and 5 with 8 x 8 tiles, one-patch tiles and 64-lane
	// workgroups), field 0, 1, 3
	struct Tie
	{
		const Geometry* g;
		int windows;
		uint64_t n;
	};
	for (const Tie& t : {Tie{&kTieSmall, 3, 674}, Tie{&kTieWide, 2, 338}, Tie{&kTieTall, 2, 338}})
	{
		for (int impl : {0, 1, 3, 4, 5})
		{
			add(t.g->name, edge(*t.g, 1, t.windows, t.n, false, impl));
		}
		for (int impl : {0, 1, 3})
		{
			add(t.g->name, edge(*t.g, 2, t.windows, t.n, false, impl));
		}
	}
	add(tiled(kTieSmall.name, 8, 8, 0), edge(kTieSmall, 1, 3, 674, false, 5, 0, 8, 8));
	add(tiled(kTieSmall.name, 8, 6, 64), edge(kTieSmall, 1, 3, 674, false, 5, 0, 8, 6, 64));
	// ... on the plan the shipped library makes by itself: tiles, unit waves, the whole-window LDS image
	add("ties C2x24", edge(kC2, 1, 24, 182, false, -1));
	add("ties fine x32", edge(kFine, 1, 32, 98, false, -1));
	add("ties C2x64 field", edge(kC2, 2, 64, 66, false, -1));
	// the seams: row bands of 25 / 25 / 23 rows (impl 1, 3, 4 at 12 KB), the tiles impl 5 chooses for 8 windows (30 x 23),
	// tiles of 8 x 8 and of one patch
	add("seams C2x3 0x25", edge(kC2, 1, 3, 380, false, 1, 12));
	add("seams C2x3 0x25", edge(kC2, 1, 3, 380, false, 3, 12));
	add("seams C2x3 0x23", edge(kC2, 1, 3, 380, false, 4, 12));
	add("seams C2x8 30x23", edge(kC2, 1, 8, 380, false, 5));
	add(tiled("seams C2x10", 8, 8, 0), edge(kC2, 1, 10, 380, false, 5, 0, 8, 8));
	add(tiled("seams C2x3", 30, 22, 0), edge(kC2, 1, 3, 380, false, 5, 0, 30, 22));
	// pile-ups on one pixel: 65535 events in a window (16-bit counters full), 65536 and more (32-bit); 1 KB bands
	for (uint64_t n : {65535u, 65536u, 70000u})
	{
		for (int impl : {0, 1, 3, 4, 5})
		{
			add("pileup " + std::to_string(n), edge(kPile, 1, 1, n, false, impl, 1));
		}
		for (int impl : {0, 1, 3})
		{
			add("pileup " + std::to_string(n), edge(kPile, 2, 1, n, false, impl, 1));
		}
		add("pileup " + std::to_string(n), edge(kPile, 0, 1, n, false, 2, 1));
	}
	// k_count_tiles's 16-bit rule: the target pixel inside a tile (16 x 12) and on a tile's first column and row (24 x 18)
	for (uint64_t n : {65531u, 65540u, 65534u})
	{
		add(tiled("tile limit", 16, 12, 0) + " " + std::to_string(n), edge(kPile, 1, 1, n, false, 5, 0, 16, 12));
		add(tiled("tile limit", 24, 18, 0) + " " + std::to_string(n), edge(kPile, 1, 1, n, false, 5, 0, 24, 18));
	}
	// test_count_image_more_than_65535_events_per_window in the warped and field modes
	for (int impl : {1, 2, 5})
	{
		add("wide C2x1 90000", shape(kC2, 1, 1, 90000, false, impl));
		add("wide C2x1 90000", shape(kC2, 2, 1, 90000, false, impl));
	}
	// the store forms (storeRows)
	for (const EdgeRow& e : storeRows())
	{
		rows.push_back(e);
	}
	return rows;
}

std::vector<std::string> goldenRows()
{
	std::vector<std::string> rows;
	auto add = [&](const std::string& label, const CountShape& s) { rows.push_back(row(label.c_str(), s)); };
	// bench.py's count_extra workloads
	for (int mode : {1, 0})
	{
		add("bench C2x1536", shape(kC2, mode, 1536, 50000));
		add("bench C3x512", shape(kC3, mode, 512, 200000));
		add("bench C4x72", shape(kC4, mode, 72, 1000000));
	}
	// the unit-wave default with 32-bit counters and its neighbours
	for (int windows : {13, 21, 22})
	{
		for (int mode : {1, 2})
		{
			add("C3x" + std::to_string(windows) + " 200k", shape(kC3, mode, windows, 200000));
		}
	}
	for (uint64_t n : {65535u, 65536u})
	{
		for (int mode : {0, 1, 2})
		{
			add("C3x21 " + std::to_string(n), shape(kC3, mode, 21, n));
			add("C2x1 " + std::to_string(n), shape(kC2, mode, 1, n));
		}
	}
	// tests/test_gpu_count.py: test_count_image_implementations (every impl x mode)
	struct Impl
	{
		const Geometry* g;
		int windows;
		uint64_t n;
	};
	for (const Impl& t : {Impl{&kC0, 1, 15000}, Impl{&kC2, 70, 9000}, Impl{&kC3, 3, 70000}, Impl{&kC4, 2, 60000}})
	{
		for (int impl : {0, 1, 2, 3, 4, 5, -1})
		{
			for (int mode : {0, 1, 2})
			{
				add(std::string("impls ") + t.g->name + "x" + std::to_string(t.windows), shape(*t.g, mode, t.windows, t.n, true, impl));
			}
		}
	}
	// ... test_count_image_more_than_65535_events_per_window
	for (int impl : {1, 2, 5})
	{
		add("wide C2x1 90000", shape(kC2, 0, 1, 90000, false, impl));
	}
	// ... test_patch_row_bands_any_band_size_and_large_flows (the forced bands, integrated), and its warped case on the
	// default plan
	for (int kb : {12, 24, 150})
	{
		add("bands C2x5", shape(kC2, 0, 5, 20000, true, 2, kb));
	}
	add("large flows C2x5", shape(kC2, 1, 5, 20000, true));
	// ... test_patch_of_an_event_from_its_coordinates
	const Geometry odd[] = {{"16383x24/2x24", 16383, 24, 2, 24}, {"16383x24/3x5", 16383, 24, 3, 5},
							{"16000x20/127x1", 16000, 20, 127, 1}, {"9000x30/8999x7", 9000, 30, 8999, 7},
							{"40x16383/1x16383", 40, 16383, 1, 16383}, {"64x48/1x1", 64, 48, 1, 1}};
	for (const Geometry& g : odd)
	{
		for (int impl : {1, 3, 4, -1})
		{
			add(g.name, shape(g, 1, 1, 6000, true, impl));
		}
	}
	// ... test_tiled_count_image_odd_sizes_and_wide_counters (impl 5, then impl 0)
	struct Tiled
	{
		Geometry g;
		uint64_t n;
		int kb;
	};
	for (const Tiled& t : {Tiled{{"347x261", 347, 261, 21, 16}, 30000, 16}, Tiled{{"347x261", 347, 261, 21, 16}, 70000, 24},
						   Tiled{{"64x48", 64, 48, 7, 5}, 4000, 1}, Tiled{{"1280x720", 1280, 720, 40, 22}, 200000, 0},
						   Tiled{{"346x260", 346, 260, 21, 16}, 50000, 0}, Tiled{{"240x180", 240, 180, 30, 22}, 20000, 40}})
	{
		add(std::string("tiled ") + t.g.name, shape(t.g, 1, 3, t.n, true, 5, t.kb));
		add(std::string("tiled ") + t.g.name, shape(t.g, 1, 3, t.n, true, 0, t.kb));
	}
	// tests/test_gpu_fullsize.py, tests/test_gpu_parity.py, tests/test_gpu_graph.py
	for (int mode : {0, 1})
	{
		add("fullsize C2", shape(kC2, mode, 1, 50000));
		add("fullsize C3", shape(kC3, mode, 1, 200000));
		add("fullsize C4", shape(kC4, mode, 1, 1000000));
		add("parity strays C0", shape(kC0, mode, 1, 405, true));
		add("parity C0x3", shape(kC0, mode, 3, 15000));
	}
	add("fullsize halves C2x2", shape(kC2, 0, 2, 25000));
	add("fullsize halves C3x2", shape(kC3, 0, 2, 100000));
	add("fullsize halves C4x2", shape(kC4, 0, 2, 500000));
	for (int mode : {0, 1, 2})
	{
		add("bit exact C0", shape(kC0, mode, 1, 15000));
		add("bit exact C2", shape(kC2, mode, 1, 50000));
		add("bit exact C4", shape(kC4, mode, 1, 300000));
	}
	add("half integer C0", shape(kC0, 1, 1, 36));
	add("batch C0x3", shape(kC0, 1, 3, 9000));
	add("graph C2x4", shape(kC2, 1, 4, 20000));
	// tests/test_gpu_count_edges.py (the cases of tests/count_cases.py)
	for (const EdgeRow& e : edgeRows())
	{
		add(e.label, e.s);
	}
	return rows;
}

// (a): the table, from the plan of the change that moved the choice out of launch_count_image (default knobs
// and the forced paths that survived the retirement of the unreachable kernels unchanged)
const char* const kGolden[] = {
#include "count_plan_golden.inc"
};

int failures = 0;

void fail(const std::string& what)
{
	std::printf("FAIL %s\n", what.c_str());
	++failures;
}
}  // namespace

int main(int argc, char** argv)
{
	const std::vector<std::string> rows = goldenRows();
	if (argc > 1 && std::strcmp(argv[1], "--print") == 0)
	{
		for (const std::string& r : rows)
		{
			std::printf("\"%s\",\n", r.c_str());
		}
		return 0;
	}
	// (a)
	const size_t nGolden = sizeof(kGolden) / sizeof(kGolden[0]);
	if (nGolden != rows.size())
	{
		fail("golden table has " + std::to_string(nGolden) + " rows, the list " + std::to_string(rows.size()));
	}
	for (size_t i = 0; i < std::min(nGolden, rows.size()); ++i)
	{
		if (rows[i] != kGolden[i])
		{
			fail("row " + std::to_string(i) + ":\n  plan   " + rows[i] + "\n  golden " + kGolden[i]);
		}
	}
	// (b) and (c)
	const Geometry grid[] = {kC0, kC1, kC2, kC3, kC4,
							 {"347x261", 347, 261, 21, 16}, {"64x48/7x5", 64, 48, 7, 5}, {"64x48/1x1", 64, 48, 1, 1},
							 {"1x1", 1, 1, 1, 1}, {"16383x24/2x24", 16383, 24, 2, 24}, {"16000x20/127x1", 16000, 20, 127, 1},
							 {"9000x30/8999x7", 9000, 30, 8999, 7}, {"40x16383/1x16383", 40, 16383, 1, 16383},
							 {"3x16383/3x7", 3, 16383, 3, 7}, {"4096x4096/64x64", 4096, 4096, 64, 64},
							 {"16383x16383/128x128", 16383, 16383, 128, 128}};
	const int windows[] = {1, 2, 3, 4, 7, 8, 9, 13, 16, 21, 22, 31, 32, 63, 64, 65, 100, 128, 256, 512, 1024, 1536, 2048};
	const uint64_t events[] = {1000, 4000, 9000, 15000, 50000, 65535, 65536, 70000, 200000, 1000000, 4000000, 8000000};
	std::set<std::string> reached;
	size_t nPlans = 0;
	for (const Geometry& g : grid)
	{
		for (int mode = 0; mode <= 2; ++mode)
		{
			for (int wn : windows)
			{
				for (uint64_t n : events)
				{
					if (static_cast<double>(wn) * n > 4294967295.0)
					{
						continue;  // event offsets are 32-bit
					}
					for (bool stray : {false, true})
					{
						// the default plan, and (warped) the tiles forced: small batches make them split finest
						for (int impl : {-1, 5})
						{
							if (impl == 5 && (mode != 1 || stray))
							{
								continue;
							}
							const CountShape s = shape(g, mode, wn, n, stray, impl);
							const CountPlan p = plan_count_image(s);
							++nPlans;
							if (impl < 0)
							{
								for (const std::string& k : kernels(s, p))
								{
									reached.insert(k);
								}
							}
							// every tile of the grid starts inside the image (the last one may be empty), and the grid covers it
							const bool tilesOk = p.kind != kCountTiles ||
												 (p.tile_w > 0 && p.tile_h > 0 && (p.tiles_x - 1) * p.tile_w < g.w &&
												  p.tiles_x * p.tile_w >= g.w && (p.tiles_y - 1) * p.tile_h <= g.h &&
												  p.tiles_y * p.tile_h >= g.h);
							const bool ok = p.lds <= 160 * 1024 && p.grid_x > 0 && p.grid_y > 0 && p.block >= 64 &&
											p.block <= 1024 && p.block % 64 == 0 && p.lds_hist <= 160 * 1024 &&
											p.lds_scatter <= 160 * 1024 && (p.kind != kCountScatter || p.convert_blocks > 0) &&
											tilesOk;
							if (!ok)
							{
								fail("invariant: " + row(g.name, s));
							}
						}
					}
				}
			}
		}
	}
	for (const std::string& k : kLaunchable)
	{
		if (!reached.count(k))
		{
			fail("launchable but never planned: " + k);
		}
	}
	for (const std::string& k : reached)
	{
		if (!kLaunchable.count(k))
		{
			fail("planned but not launchable: " + k);
		}
	}
	// (d) the store-form shapes give every path a band with an odd pixel count at an aligned start, a band with an odd
	// start, and a second window at an odd pixel offset
	std::set<int> storeImpls;
	for (const EdgeRow& e : storeRows())
	{
		const CountPlan p = plan_count_image(e.s);
		const CountKind want = e.s.impl == 1 ? kCountWindowLds : e.s.impl == 2 ? kCountBands : e.s.impl == 3 ? kCountSorted : kCountUnits;
		const int bandRows = p.kind == kCountBands ? p.prb * e.s.patch_h : p.rows_per_band;
		const int nBands = p.kind == kCountBands ? p.n_regular + 1 : p.bands;
		const bool ok = p.kind == want && p.u16 && e.s.windows > 1 && (e.s.image_w * e.s.image_h) % 2 == 1 &&
						(bandRows * e.s.image_w) % 2 == 1 && nBands >= 2 && bandRows < e.s.image_h &&
						(p.kind != kCountBands || p.col_tiles == 1);
		if (!ok)
		{
			fail("store forms: " + row(e.label.c_str(), e.s));
		}
		storeImpls.insert(e.s.impl);
	}
	if (storeImpls != std::set<int>{1, 2, 3, 4})
	{
		fail("store forms: not every implementation has a shape");
	}
	std::printf("%zu golden rows, %zu plans, %zu kernels reached\n", rows.size(), nPlans, reached.size());
	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
