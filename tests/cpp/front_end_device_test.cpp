// FeatureDetector::useDeviceFrontEnd() driven through newImage on the three DAVIS fixture frames, with the
// replayer's events fed between them, against (a) ebo_good_features called directly with the reference's mask and
// maxCorners_, (b) the flow results the CPU restatement computed for the same frames, and (c) a second detector whose
// hooks are filled from those precomputed results.  Built and run by tests/test_gpu_front_end.py:
//   front_end_device_test frame0.pgm frame1.pgm frame2.pgm events.txt ref.txt
// ref.txt: per frame k "corners n x y ...", "grad <file of 2 x h x w doubles>", and for k > 0 "flow n (px py nx ny
// status) ..." for the corners of frames k-1 and k tracked from frame k-1 to frame k.
#include <feature_tracker/feature_detector.h>

#include <cmath>
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT_TRUE(c)                                                         \
	do                                                                         \
	{                                                                          \
		if (!(c))                                                              \
		{                                                                      \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
			++g_fail;                                                          \
		}                                                                      \
	} while (0)

static common::Image8 readPgm(const std::string& path)
{
	std::ifstream f(path, std::ios::binary);
	std::string magic;
	int w = 0, h = 0, maxv = 0;
	f >> magic >> w >> h >> maxv;
	f.get();
	common::Image8 img(h, w);
	f.read(reinterpret_cast<char*>(img.data.data()), static_cast<std::streamsize>(w) * h);
	if (magic != "P5" || maxv != 255 || !f)
	{
		throw std::runtime_error("bad PGM " + path);
	}
	return img;
}

struct Flow
{
	float nx, ny;
	int status;
};
struct Ref
{
	std::vector<tracker::Corners> corners;        // per frame
	std::vector<std::string> grads;               // per frame: file of gradX then gradY
	std::vector<std::map<std::pair<float, float>, Flow>> flow;  // per frame (0: empty)
};

static Ref readRef(const std::string& path)
{
	Ref r;
	std::ifstream f(path);
	std::string line;
	while (std::getline(f, line))
	{
		std::istringstream in(line);
		std::string kind;
		int n = 0;
		in >> kind;
		if (kind == "corners")
		{
			in >> n;
			tracker::Corners c;
			for (int k = 0; k < n; ++k)
			{
				float x, y;
				in >> x >> y;
				c.push_back(tracker::Corner(x, y));
			}
			r.corners.push_back(c);
			r.flow.emplace_back();
		}
		else if (kind == "grad")
		{
			std::string g;
			in >> g;
			r.grads.push_back(g);
		}
		else if (kind == "flow")
		{
			in >> n;
			for (int k = 0; k < n; ++k)
			{
				float px, py;
				Flow fl;
				in >> px >> py >> fl.nx >> fl.ny >> fl.status;
				r.flow.back()[{px, py}] = fl;
			}
		}
	}
	return r;
}

static std::vector<common::EventSample> readEvents(const std::string& path)
{
	std::vector<common::EventSample> ev;
	std::ifstream f(path);
	double t;
	int x, y, p;
	while (f >> t >> x >> y >> p)
	{
		common::Event e;
		e.point = common::Point2i(x, y);
		e.sign = p > 0 ? common::POSITIVE : common::NEGATIVE;
		ev.emplace_back(e, common::timestamp_t(static_cast<int64_t>(std::llround(t * 1e6))));
	}
	return ev;
}

// newImage on the three frames, the events after the first one, the second one fed between frames 1 and 2
static void runSequence(tracker::FeatureDetector& d, const std::vector<common::Image8>& frames,
						const std::vector<common::EventSample>& ev, int* frameOut, void (*afterFrame)(tracker::FeatureDetector&, int))
{
	for (int k = 0; k < 3; ++k)
	{
		*frameOut = k;
		d.newImage(common::ImageSample(frames[k], common::timestamp_t(1000 + 40000 * k)));
		if (afterFrame)
		{
			afterFrame(d, k);
		}
		if (k < static_cast<int>(ev.size()))
		{
			common::EventSample e = ev[k];
			e.timestamp = common::timestamp_t(1000 + 40000 * k + 20000);
			d.addEvent(e);
			d.updatePatches(e);
		}
	}
}

static Ref g_ref;
static std::vector<common::Image8> g_frames;

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static tracker::Corner initPoint(const tracker::Patch& p)
{
	const tracker::Rect2d r = p.getInitPatch();
	return tracker::Corner(r.x + (r.width - 1) / 2., r.y + (r.height - 1) / 2.);
}

static std::set<tracker::TrackId> g_initBefore;  // device run: track ids initialised by an earlier frame
static std::set<tracker::TrackId> g_archivedBefore;

// after frame k of the device run: the patches flowed at this frame carry the restatement's flow (status 1:
// initialised with warp -(next - corner) and flowDir atan2; status 0: archived as lost)
static void checkFlow(tracker::FeatureDetector& d, int k)
{
	int checked = 0;
	for (const auto& p : d.getPatches())
	{
		if (k == 0)
		{
			EXPECT_TRUE(!p.isInit());
		}
		if (!p.isInit() || g_initBefore.count(p.getTrackId()))
		{
			continue;
		}
		const tracker::Corner c0 = initPoint(p);
		auto it = g_ref.flow[k].find({static_cast<float>(c0.x), static_cast<float>(c0.y)});
		EXPECT_TRUE(it != g_ref.flow[k].end());
		if (it == g_ref.flow[k].end())
		{
			continue;
		}
		EXPECT_TRUE(it->second.status == 1);
		const double dx = it->second.nx - static_cast<float>(c0.x), dy = it->second.ny - static_cast<float>(c0.y);
		EXPECT_TRUE(near(p.getWarp().data()[2], -dx, 1e-3) && near(p.getWarp().data()[3], -dy, 1e-3));
		EXPECT_TRUE(near(p.getFlowDir(), std::atan2(dy, dx), 2e-3 / std::max(1e-3, std::hypot(dx, dy))));
		g_initBefore.insert(p.getTrackId());
		++checked;
	}
	EXPECT_TRUE(k != 1 || checked > 0);  // frame 1 flows the patches of frames 0 and 1 (later frames: only new ones)
	int zeroStatus = 0;
	for (const auto& p : d.getArchivedPatches())
	{
		if (g_archivedBefore.count(p.getTrackId()))
		{
			continue;
		}
		g_archivedBefore.insert(p.getTrackId());
		const tracker::Corner c0 = initPoint(p);
		auto it = g_ref.flow[k].find({static_cast<float>(c0.x), static_cast<float>(c0.y)});
		EXPECT_TRUE(p.isLost());
		zeroStatus += (it != g_ref.flow[k].end() && it->second.status == 0) ? 1 : 0;
	}
	// a patch flowed at this frame with status 0 is not tracked any more
	for (const auto& p : d.getPatches())
	{
		auto it = g_ref.flow[k].find({static_cast<float>(initPoint(p).x), static_cast<float>(initPoint(p).y)});
		EXPECT_TRUE(p.isInit() || it == g_ref.flow[k].end() || it->second.status != 0);
	}
	std::printf("frame %d: %d patches flowed, %d archived with status 0\n", k, checked, zeroStatus);
}

static int g_frame = 0;

int main(int argc, char** argv)
{
	if (argc != 6)
	{
		std::printf("usage: front_end_device_test f0.pgm f1.pgm f2.pgm events.txt ref.txt\n");
		return 2;
	}
	for (int k = 0; k < 3; ++k)
	{
		g_frames.push_back(readPgm(argv[1 + k]));
	}
	const std::vector<common::EventSample> ev = readEvents(argv[4]);
	g_ref = readRef(argv[5]);
	EXPECT_TRUE(g_ref.corners.size() == 3 && g_ref.grads.size() == 3);

	tracker::DetectorParams params;
	params.patchExtent = 5;
	params.errorPolicy = tracker::DetectorParams::ERRORS_THROW;

	// (a) detectFeatures == ebo_good_features with the reference's mask_ and maxCorners_
	tracker::FeatureDetector dev(params);
	dev.useDeviceFrontEnd();
	{
		const int w = 240, h = 180, e = params.patchExtent;
		const int maxCorners = w * h / ((2 * e + 1) * (2 * e + 1));
		std::vector<uint8_t> mask(static_cast<size_t>(w) * h, 0);
		for (int y = e; y < h - e; ++y)
		{
			for (int x = e; x < w - e; ++x)
			{
				mask[static_cast<size_t>(y) * w + x] = 1;
			}
		}
		for (int k = 0; k < 3; ++k)
		{
			std::vector<float> xy(2 * maxCorners);
			int n = 0;
			EXPECT_TRUE(ebo_good_features(dev.handle(), g_frames[k].data.data(), mask.data(), maxCorners, params.qualityLevel,
										  params.minDistance, params.blockSize, 0.04, xy.data(), &n) == EBO_OK);
			const tracker::Corners c = dev.detectFeatures(g_frames[k]);
			EXPECT_TRUE(static_cast<int>(c.size()) == n && n > 10);
			EXPECT_TRUE(c.size() == g_ref.corners[k].size());
			for (int i = 0; i < n && i < static_cast<int>(c.size()); ++i)
			{
				EXPECT_TRUE(c[i].x == xy[2 * i] && c[i].y == xy[2 * i + 1]);
				if (i < static_cast<int>(g_ref.corners[k].size()))
				{
					EXPECT_TRUE(c[i].x == g_ref.corners[k][i].x && c[i].y == g_ref.corners[k][i].y);
				}
			}
		}
	}

	// (b) the device run through newImage
	runSequence(dev, g_frames, ev, &g_frame, checkFlow);

	// (c) the same sequence with hooks filled from the restatement's results
	tracker::FeatureDetector host(params);
	tracker::FrontEndHooks hk;
	hk.detectFeatures = [](const common::Image8&) { return g_ref.corners[g_frame]; };
	hk.gradients = [](const common::Image8&, tracker::Mat64& gx, tracker::Mat64& gy) {
		gx = tracker::Mat64(180, 240);
		gy = tracker::Mat64(180, 240);
		std::ifstream f(g_ref.grads[g_frame], std::ios::binary);
		f.read(reinterpret_cast<char*>(gx.ptr()), 240 * 180 * 8);
		f.read(reinterpret_cast<char*>(gy.ptr()), 240 * 180 * 8);
		if (!f)
		{
			throw std::runtime_error("gradient file");
		}
	};
	hk.flowBatch = [](const std::vector<float>& prev, std::vector<float>& next, std::vector<uint8_t>& status) {
		next.assign(prev.size(), 0.f);
		status.assign(prev.size() / 2, 0);
		for (size_t i = 0; i < prev.size() / 2; ++i)
		{
			auto it = g_ref.flow[g_frame].find({prev[2 * i], prev[2 * i + 1]});
			if (it == g_ref.flow[g_frame].end())
			{
				throw std::runtime_error("no precomputed flow for a point");
			}
			next[2 * i] = it->second.nx;
			next[2 * i + 1] = it->second.ny;
			status[i] = static_cast<uint8_t>(it->second.status);
		}
	};
	host.setFrontEndHooks(hk);
	runSequence(host, g_frames, ev, &g_frame, nullptr);

	const tracker::Patches& a = dev.getPatches();
	const tracker::Patches& b = host.getPatches();
	EXPECT_TRUE(a.size() == b.size() && !a.empty());
	EXPECT_TRUE(dev.getArchivedPatches().size() == host.getArchivedPatches().size());
	auto ib = b.begin();
	for (auto ia = a.begin(); ia != a.end() && ib != b.end(); ++ia, ++ib)
	{
		EXPECT_TRUE(ia->getTrackId() == ib->getTrackId() && ia->isInit() == ib->isInit() && ia->isLost() == ib->isLost());
		for (int q = 0; q < 4; ++q)
		{
			EXPECT_TRUE(near(ia->getWarp().data()[q], ib->getWarp().data()[q], 1e-3));
		}
		EXPECT_TRUE(near(ia->getFlowDir(), ib->getFlowDir(), 1e-2));
	}
	int lost = 0;
	for (const auto& p : dev.getArchivedPatches())
	{
		lost += p.isLost() ? 1 : 0;
	}
	std::printf("patches %zu, archived %zu (lost %d)\n", a.size(), dev.getArchivedPatches().size(), lost);
	if (g_fail)
	{
		std::printf("front_end_device_test: %d FAILED\n", g_fail);
		return 1;
	}
	std::printf("front_end_device_test: ok\n");
	return 0;
}
