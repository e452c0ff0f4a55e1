// bundle_adjust_serial.cpp — the bundle-adjustment rules of include/ebo.h (B1-B9) compiled for the host: the device's
// own text (csrc/ebo_bundle.inc) with the 256 lanes of a phase run one after the other on one thread.  The serial
// timing baseline of tools/time_bundle_adjust.py and the CPU check of that text (tests/test_bundle_cpu.py).  Not part
// of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o bundle_adjust_serial bundle_adjust_serial.cpp
//   bundle_adjust_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: F, P, N, fix_points, max_num_iterations, use_nonmonotonic, function_tolerance,
//         gradient_tolerance, parameter_tolerance, huber, camera (fx fy cx cy k1 k2 k3 p1 p2), poses [F][12], fixed [F],
//         points [P][3], frame [N], point [N], uv [N][2]; observations in (point, frame) order.  Then the rest of
//         ebo_solver_opts in its order: initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal,
//         max_lm_diagonal, max_consecutive_nonmonotonic, max_consecutive_invalid, jacobi_scaling.  A file that ends
//         after uv takes ebo_default_ba_opts' for these nine; mode, which the solve never reads, is never carried.
//       result.f64: iterations, num_evals_cost, num_evals_jac, termination, initial_cost, final_cost, poses, points,
//         trace [max_num_iterations + 1][4].  Prints one JSON line with the median milliseconds of `repeats` solves.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/ebo_bundle.h"

using namespace ebo;
using std::fabs;
using std::sqrt;
#define EBO_BUNDLE_RULES_ONLY
#include "../csrc/ebo_bundle.inc"

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
	constexpr size_t kHead = 19, kTail = 9;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	const int F = static_cast<int>(in[0]), P = static_cast<int>(in[1]), N = static_cast<int>(in[2]);
	const size_t upToUv = kHead + 13 * static_cast<size_t>(F) + 3 * static_cast<size_t>(P) + 4 * static_cast<size_t>(N);
	if (F < 0 || F > kBaMaxFrames || P < 0 || P > kBaMaxPoints || N < 0 || N > kBaMaxObs || (in.size() != upToUv && in.size() != upToUv + kTail))
	{
		std::fprintf(stderr, "sizes over the limits or not those of the file\n");
		return 2;
	}
	ebo_solver_opts o;
	ba_default_opts(o);
	o.max_num_iterations = static_cast<int>(in[4]);
	o.use_nonmonotonic = static_cast<int>(in[5]);
	o.function_tolerance = in[6];
	o.gradient_tolerance = in[7];
	o.parameter_tolerance = in[8];
	if (in.size() == upToUv + kTail)
	{
		const double* t = in.data() + upToUv;
		o.initial_radius = t[0];
		o.max_radius = t[1];
		o.min_radius = t[2];
		o.min_relative_decrease = t[3];
		o.min_lm_diagonal = t[4];
		o.max_lm_diagonal = t[5];
		o.max_consecutive_nonmonotonic = static_cast<int>(t[6]);
		o.max_consecutive_invalid = static_cast<int>(t[7]);
		o.jacobi_scaling = static_cast<int>(t[8]);
	}
	const double huber = in[9];
	ebo_camera cam;
	cam.fx = in[10], cam.fy = in[11], cam.cx = in[12], cam.cy = in[13], cam.k1 = in[14], cam.k2 = in[15], cam.k3 = in[16], cam.p1 = in[17],
	cam.p2 = in[18];
	if (o.max_num_iterations < 0)
	{
		std::fprintf(stderr, "a negative iteration count\n");
		return 2;
	}
	const double* at = in.data() + kHead;
	const std::vector<double> poses0(at, at + 12 * F);
	at += 12 * F;
	std::vector<unsigned char> fixed(F);
	for (int k = 0; k < F; ++k)
	{
		fixed[k] = at[k] != 0.0;
	}
	at += F;
	const std::vector<double> points0(at, at + 3 * P);
	at += 3 * P;
	std::vector<int> of(N), op(N);
	for (int i = 0; i < N; ++i)
	{
		of[i] = static_cast<int>(at[i]);
		op[i] = static_cast<int>(at[N + i]);
	}
	at += 2 * N;
	const std::vector<double> uv(at, at + 2 * N);

	std::vector<double> poses, points, trace(4 * (static_cast<size_t>(o.max_num_iterations) + 1));
	std::vector<double> work(ba_work_doubles(F, P, N));
	std::vector<int> iwork(ba_work_ints(F, P, static_cast<size_t>(F) * P, 1));
	std::vector<double> S(ba_reduced_doubles(kBaMaxFrames)), vec(kBaMaxDim), sol(kBaMaxDim), part(kBaLanes);
	BaState st{};
	std::vector<double> ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		poses = poses0;
		points = points0;
		const auto t0 = std::chrono::steady_clock::now();
		BaView v{};
		v.F = F, v.P = P, v.N = N, v.fixPoints = in[3] != 0.0;
		v.fixed = fixed.data();
		v.of = of.data();
		v.op = op.data();
		v.uv = uv.data();
		v.outPose = poses.data();
		v.outPt = points.data();
		double* w = work.data();
		auto take = [&](size_t n) {
			double* p = w;
			w += n;
			return p;
		};
		v.xPose = take(12 * F), v.cPose = take(12 * F), v.xPt = take(3 * P), v.cPt = take(3 * P);
		v.res = take(2 * N), v.Jc = take(12 * N), v.Jp = take(6 * N), v.W = take(18 * N), v.Y = take(18 * N);
		v.U = take(42 * F), v.V = take(12 * P), v.Vinv = take(9 * P), v.scale = take(6 * F + 3 * P), v.step = take(6 * F + 3 * P);
		v.red = take(N + 12 * F + 3 * P);
		v.table = iwork.data();
		v.pstart = v.table + static_cast<size_t>(F) * P;
		v.fslot = v.pstart + P + 1;
		v.flist = v.fslot + F;
		ba_solve(v, cam, huber, o, st, S.data(), vec.data(), sol.data(), part.data(), trace.data());
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::vector<double> out = {static_cast<double>(st.iterations), static_cast<double>(st.evalsCost), static_cast<double>(st.evalsJac),
							   static_cast<double>(st.termination), st.initialCost, st.minCost};
	out.insert(out.end(), poses.begin(), poses.end());
	out.insert(out.end(), points.begin(), points.end());
	out.insert(out.end(), trace.begin(), trace.end());
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	char cost[40] = "null";  // a cost that is not finite has no JSON number
	if (std::isfinite(st.minCost))
	{
		std::snprintf(cost, sizeof cost, "%.17g", st.minCost);
	}
	std::printf("{\"frames\": %d, \"points\": %d, \"observations\": %d, \"iterations\": %d, \"termination\": %d, \"final_cost\": %s, "
				"\"ms_median\": %.4f, \"repeats\": %d}\n",
				F, P, N, st.iterations, st.termination, cost, ms[ms.size() / 2], repeats);
	return 0;
}
