// The count-image launch plan (csrc/count_plan.h) on the CPU: (a) the full plan of a written-down list of shapes
// against a table, (b) over a grid of modes, sensors, batch sizes and window sizes with default knobs, the kernels
// reached are exactly the ones launch_count_image (csrc/ebo_kernels.hip) can launch, (c) every plan fits the device:
// LDS <= 160 KB, grid > 0, a block of whole waves <= 1024 lanes.  Run by tests/test_count_plan.py.
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
						const CountShape s = shape(g, mode, wn, n, stray);
						const CountPlan p = plan_count_image(s);
						++nPlans;
						for (const std::string& k : kernels(s, p))
						{
							reached.insert(k);
						}
						const bool ok = p.lds <= 160 * 1024 && p.grid_x > 0 && p.grid_y > 0 && p.block >= 64 &&
										p.block <= 1024 && p.block % 64 == 0 && p.lds_hist <= 160 * 1024 &&
										p.lds_scatter <= 160 * 1024 && (p.kind != kCountScatter || p.convert_blocks > 0);
						if (!ok)
						{
							fail("invariant: " + row(g.name, s));
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
	std::printf("%zu golden rows, %zu plans, %zu kernels reached\n", rows.size(), nPlans, reached.size());
	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
