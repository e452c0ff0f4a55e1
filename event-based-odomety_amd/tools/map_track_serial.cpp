// map_track_serial.cpp — the map-tracking rules of include/ebo.h (E1-E9) compiled for the host: the device's own text
// (csrc/ebo_maptrack.inc) with the 256 lanes of a sum run one after the other on one thread, unit after unit.  The serial
// timing baseline of tools/time_map_track.py and the CPU check of that text (tests/test_maptrack_cpu.py).  Not part of
// the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o map_track_serial map_track_serial.cpp
//   map_track_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: w, h, n_images, n_points, n_units, z_min, fx, fy, cx, cy, then ebo_solver_opts in its
//         order without mode (max_num_iterations, use_nonmonotonic, function_tolerance, gradient_tolerance,
//         parameter_tolerance, initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal,
//         max_lm_diagonal, max_consecutive_nonmonotonic, max_consecutive_invalid, jacobi_scaling): a head of 24; then
//         images [n_images][h][w], points [n_points][3], unit_image [n_units], poses [n_units][12].
//       result.f64, per unit: pose [12], termination, iterations, num_evals_jac, num_evals_cost, visible_start,
//         visible_final, initial_cost, final_cost, scale, trace [max_num_iterations + 1][4].
//       Prints one JSON line with the median milliseconds of `repeats` runs over all units.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../csrc/ebo_maptrack.h"

using namespace ebo;
using std::fabs;
using std::floor;
using std::sqrt;
#define EBO_MAPTRACK_RULES_ONLY
#include "../csrc/ebo_maptrack.inc"

namespace
{
std::vector<double> readAll(const char* path)
{
	std::vector<double> v;
	FILE* f = std::fopen(path, "rb");
	if (!f)
	{
		std::fprintf(stderr, "cannot open %s\n", path);
		std::exit(2);
	}
	double buf[1024];
	size_t n;
	while ((n = std::fread(buf, sizeof(double), 1024, f)) > 0)
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
		std::fprintf(stderr, "usage: %s <problem.f64> <result.f64> <repeats>\n", argv[0]);
		return 2;
	}
	const std::vector<double> in = readAll(argv[1]);
	const int repeats = std::atoi(argv[3]);
	constexpr size_t kHead = 24;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	MtCall k{};
	k.w = static_cast<int>(in[0]);
	k.h = static_cast<int>(in[1]);
	k.n_images = static_cast<int>(in[2]);
	k.n_points = static_cast<int>(in[3]);
	const int nUnits = static_cast<int>(in[4]);
	k.z_min = in[5];
	k.fx = in[6], k.fy = in[7], k.cx = in[8], k.cy = in[9];
	ebo_solver_opts o;
	mt_default_opts(o);
	o.max_num_iterations = static_cast<int>(in[10]);
	o.use_nonmonotonic = static_cast<int>(in[11]);
	o.function_tolerance = in[12];
	o.gradient_tolerance = in[13];
	o.parameter_tolerance = in[14];
	o.initial_radius = in[15];
	o.max_radius = in[16];
	o.min_radius = in[17];
	o.min_relative_decrease = in[18];
	o.min_lm_diagonal = in[19];
	o.max_lm_diagonal = in[20];
	o.max_consecutive_nonmonotonic = static_cast<int>(in[21]);
	o.max_consecutive_invalid = static_cast<int>(in[22]);
	o.jacobi_scaling = static_cast<int>(in[23]);
	if (k.w < 2 || k.h < 2 || k.n_images < 0 || k.n_points < 0 || k.n_points > kMtMaxPoints || nUnits < 0 || nUnits > kMtMaxUnits ||
		o.max_num_iterations < 0 || o.max_num_iterations > kMtMaxIterations)
	{
		std::fprintf(stderr, "sizes outside the limits\n");
		return 2;
	}
	const size_t np = static_cast<size_t>(k.w) * k.h;
	const size_t want = kHead + k.n_images * np + 3 * static_cast<size_t>(k.n_points) + 13 * static_cast<size_t>(nUnits);
	if (in.size() != want)
	{
		std::fprintf(stderr, "the file has %zu doubles, its head asks for %zu\n", in.size(), want);
		return 2;
	}
	const double* at = in.data() + kHead;
	k.images = at;
	at += k.n_images * np;
	k.points = at;
	at += 3 * static_cast<size_t>(k.n_points);
	std::vector<int> unitImage(nUnits);
	for (int u = 0; u < nUnits; ++u)
	{
		unitImage[u] = static_cast<int>(at[u]);
	}
	at += nUnits;
	const std::vector<double> poses0(at, at + 12 * static_cast<size_t>(nUnits));

	const size_t rows = static_cast<size_t>(o.max_num_iterations) + 1;
	const size_t perUnit = 12 + 9 + 4 * rows;
	std::vector<double> out(perUnit * nUnits), poses;
	const std::unique_ptr<MtShared> sh(new MtShared);
	std::vector<double> ms;
	long long iterations = 0;
	for (int rep = 0; rep < repeats; ++rep)
	{
		poses = poses0;
		iterations = 0;
		const auto t0 = std::chrono::steady_clock::now();
		for (int u = 0; u < nUnits; ++u)
		{
			double* o_u = out.data() + perUnit * u;
			mt_solve(k, unitImage[u], poses.data() + 12 * static_cast<size_t>(u), o, *sh, o_u + 21);
			ebo_map_track_result r;
			mt_result(sh->st, r);
			std::copy(poses.begin() + 12 * u, poses.begin() + 12 * (u + 1), o_u);
			const double f[9] = {static_cast<double>(r.termination),    static_cast<double>(r.iterations),
								 static_cast<double>(r.num_evals_jac),  static_cast<double>(r.num_evals_cost),
								 static_cast<double>(r.visible_start),  static_cast<double>(r.visible_final),
								 r.initial_cost,                        r.final_cost,
								 r.scale};
			std::copy(f, f + 9, o_u + 12);
			iterations += r.iterations;
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"units\": %d, \"points\": %d, \"images\": %d, \"iterations\": %lld, \"ms_median\": %.4f, \"repeats\": %d}\n", nUnits,
				k.n_points, k.n_images, iterations, ms[ms.size() / 2], repeats);
	return 0;
}
