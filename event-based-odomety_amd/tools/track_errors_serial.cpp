// track_errors_serial.cpp — the track-evaluation rules of include/ebo.h (V1-V9) compiled for the host: the device's own
// text (csrc/ebo_trackerr.inc) with the 64 lanes of a reduction run one after the other on one thread.  The serial
// timing baseline of tools/time_track_errors.py and the CPU check of that text (tests/test_trackerr_cpu.py).  Not part
// of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I include -o track_errors_serial track_errors_serial.cpp
//   track_errors_serial <problem.bin> <result.bin> <repeats>
//       problem.bin, raw: int64 n_tracks, n_taus, n_est, n_gt; int64 est_off [n_tracks + 1], gt_off [n_tracks + 1],
//         est_t [n_est], gt_t [n_gt]; float64 taus [n_taus], est_xy [n_est][2], gt_xy [n_gt][2].
//       result.bin: per (track, tau) float64 err_mean, err_rmse, err_max, then int64 age_us, t_first_us, n_inliers,
//         n_comparable, first, cut, status; then float64 sample errors [n_est] (V8).
//       Prints one JSON line with the median milliseconds of `repeats` evaluations of ALL units.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ebo.h"
#include "../csrc/ebo_relpose.h"
#include "../csrc/ebo_trackerr.h"

using namespace ebo;
using std::fabs;
using std::sqrt;
#define EBO_RELPOSE_RULES_ONLY
#include "../csrc/ebo_relpose.inc"
#include "../csrc/ebo_trackerr.inc"

namespace
{
std::vector<char> readAll(const char* path)
{
	std::vector<char> v;
	FILE* f = std::fopen(path, "rb");
	if (!f)
	{
		std::fprintf(stderr, "cannot open %s\n", path);
		std::exit(2);
	}
	char buf[65536];
	size_t n;
	while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0)
	{
		v.insert(v.end(), buf, buf + n);
	}
	std::fclose(f);
	return v;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 4)
	{
		std::fprintf(stderr, "usage: %s <problem.bin> <result.bin> <repeats>\n", argv[0]);
		return 2;
	}
	const std::vector<char> in = readAll(argv[1]);
	const int repeats = std::atoi(argv[3]);
	int64_t head[4] = {0, 0, 0, 0};
	if (in.size() < sizeof(head) || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	std::memcpy(head, in.data(), sizeof(head));
	const int64_t K = head[0], J = head[1], NE = head[2], NG = head[3];
	if (K < 0 || K > kTeMaxTracks || J < 0 || J > kTeMaxTaus || NE < 0 || NG < 0 || NE > INT32_MAX || NG > INT32_MAX ||
		in.size() != 8 * static_cast<size_t>(4 + 2 * (K + 1) + NE + NG + J + 2 * NE + 2 * NG))
	{
		std::fprintf(stderr, "a track or threshold count out of range or sizes that are not those of the file\n");
		return 2;
	}
	// every array is 8-byte data at an 8-byte offset of the vector's storage
	const int64_t* estOff = reinterpret_cast<const int64_t*>(in.data()) + 4;
	const int64_t* gtOff = estOff + (K + 1);
	const int64_t* estT = gtOff + (K + 1);
	const int64_t* gtT = estT + NE;
	const double* taus = reinterpret_cast<const double*>(gtT + NG);
	const double* estXy = taus + J;
	const double* gtXy = estXy + 2 * NE;
	for (int64_t k = 0; k < K; ++k)
	{
		if (estOff[0] != 0 || gtOff[0] != 0 || estOff[k + 1] < estOff[k] || gtOff[k + 1] < gtOff[k] || estOff[k + 1] > NE ||
			gtOff[k + 1] > NG || estOff[k + 1] - estOff[k] > kTeMaxTrackSamples || gtOff[k + 1] - gtOff[k] > kTeMaxTrackSamples)
		{
			std::fprintf(stderr, "offsets that decrease, do not start at 0 or leave the arrays, or a track beyond 2^24 samples\n");
			return 2;
		}
	}
	std::vector<ebo_track_error_result> res(static_cast<size_t>(K * J));
	std::vector<double> per(static_cast<size_t>(NE), 0.0);
	std::vector<double> ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		const auto t0 = std::chrono::steady_clock::now();
		for (int64_t k = 0; k < K; ++k)
		{
			for (int64_t j = 0; j < J; ++j)
			{
				TeView v;
				v.nEst = static_cast<int>(estOff[k + 1] - estOff[k]);
				v.nGt = static_cast<int>(gtOff[k + 1] - gtOff[k]);
				v.estT = estT + estOff[k];
				v.estXy = estXy + 2 * estOff[k];
				v.gtT = gtT + gtOff[k];
				v.gtXy = gtXy + 2 * gtOff[k];
				v.tau = taus[j];
				v.sampleErr = j == 0 ? per.data() + estOff[k] : nullptr;
				te_unit(v, &res[static_cast<size_t>(k * J + j)]);
			}
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	FILE* fo = std::fopen(argv[2], "wb");
	bool ok = fo != nullptr;
	size_t inliers = 0;
	for (const ebo_track_error_result& r : res)
	{
		const double d[3] = {r.err_mean, r.err_rmse, r.err_max};
		const int64_t i[7] = {r.age_us, r.t_first_us, r.n_inliers, r.n_comparable, r.first, r.cut, r.status};
		ok = ok && std::fwrite(d, sizeof(double), 3, fo) == 3 && std::fwrite(i, sizeof(int64_t), 7, fo) == 7;
		inliers += static_cast<size_t>(r.n_inliers);
	}
	ok = ok && std::fwrite(per.data(), sizeof(double), per.size(), fo) == per.size();
	if (!ok)
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"units\": %zu, \"inliers\": %zu, \"ms_median\": %.4f, \"repeats\": %d}\n", res.size(), inliers, ms[ms.size() / 2], repeats);
	return 0;
}
