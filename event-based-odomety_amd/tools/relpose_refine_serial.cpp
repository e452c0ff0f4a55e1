// relpose_refine_serial.cpp — the relative-pose refinement rules of include/ebo.h (R1-R8) compiled for the host: the
// device's own text (csrc/ebo_relpose.inc) with the 64 lanes of a sum run one after the other on one thread.  The
// serial timing baseline of tools/time_relative_refine.py and the CPU check of that text
// (tests/test_relpose_refine_cpu.py).  Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I include -o relpose_refine_serial relpose_refine_serial.cpp
//   relpose_refine_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: n_pairs, the 14 fields of ebo_solver_opts in its order (mode is not carried),
//         offsets [n_pairs + 1], n_inliers [n_pairs], models [n_pairs][12], f1 [total][3], f2 [total][3],
//         inlier_idx [total] (pair p's list starts at offsets[p]; entries past its n_inliers are not read).
//       result.f64: per pair iterations, num_evals_cost, num_evals_jac, termination, initial_cost, final_cost,
//         model [12]; then the traces [n_pairs][max_num_iterations + 1][4].
//       Prints one JSON line with the median milliseconds of `repeats` solves of ALL pairs.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/ebo_bundle.h"
#include "../csrc/ebo_relpose.h"

using namespace ebo;
using std::fabs;
using std::sqrt;
#define EBO_RELPOSE_RULES_ONLY
#include "../csrc/ebo_relpose.inc"

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
	constexpr size_t kHead = 15;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	const int P = static_cast<int>(in[0]);
	ebo_solver_opts o;
	ba_default_opts(o);
	o.max_num_iterations = static_cast<int>(in[1]);
	o.use_nonmonotonic = static_cast<int>(in[2]);
	o.function_tolerance = in[3];
	o.gradient_tolerance = in[4];
	o.parameter_tolerance = in[5];
	o.initial_radius = in[6];
	o.max_radius = in[7];
	o.min_radius = in[8];
	o.min_relative_decrease = in[9];
	o.min_lm_diagonal = in[10];
	o.max_lm_diagonal = in[11];
	o.max_consecutive_nonmonotonic = static_cast<int>(in[12]);
	o.max_consecutive_invalid = static_cast<int>(in[13]);
	o.jacobi_scaling = static_cast<int>(in[14]);
	if (P < 0 || P > kRpMaxPairs || o.max_num_iterations < 0 || in.size() < kHead + 2 * static_cast<size_t>(P) + 1)
	{
		std::fprintf(stderr, "a pair count outside [0, 65535], a negative iteration count or a short file\n");
		return 2;
	}
	const double* at = in.data() + kHead;
	std::vector<int> offsets(P + 1), count(P);
	for (int p = 0; p <= P; ++p)
	{
		offsets[p] = static_cast<int>(at[p]);
	}
	at += P + 1;
	for (int p = 0; p < P; ++p)
	{
		count[p] = static_cast<int>(at[p]);
		const int size = offsets[p + 1] - offsets[p];
		if (offsets[0] != 0 || size < 0 || size > kRpMaxPoints || count[p] < 0 || count[p] > size)
		{
			std::fprintf(stderr, "offsets or inlier counts out of order\n");
			return 2;
		}
	}
	at += P;
	const size_t total = static_cast<size_t>(offsets[P]);
	if (in.size() != kHead + 2 * static_cast<size_t>(P) + 1 + 12 * static_cast<size_t>(P) + 7 * total)
	{
		std::fprintf(stderr, "sizes are not those of the file\n");
		return 2;
	}
	const std::vector<double> models0(at, at + 12 * static_cast<size_t>(P));
	at += 12 * static_cast<size_t>(P);
	const std::vector<double> f1(at, at + 3 * total), f2(at + 3 * total, at + 6 * total);
	at += 6 * total;
	std::vector<int> idx(total);
	for (size_t i = 0; i < total; ++i)
	{
		idx[i] = static_cast<int>(at[i]);
	}
	const size_t rows = static_cast<size_t>(o.max_num_iterations) + 1;
	std::vector<double> models, trace(4 * rows * P), work(rp_work_doubles(total));
	std::vector<ebo_summary> summ(P);
	std::vector<double> ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		models = models0;
		const auto t0 = std::chrono::steady_clock::now();
		for (int p = 0; p < P; ++p)
		{
			const size_t a = static_cast<size_t>(offsets[p]);
			RpView v;
			v.n = offsets[p + 1] - offsets[p];
			v.m = count[p];
			v.f1 = f1.data() + 3 * a;
			v.f2 = f2.data() + 3 * a;
			v.idx = idx.data() + a;
			v.work = work.data() + kRpRowDoubles * a;
			rp_solve(v, o, models.data() + 12 * static_cast<size_t>(p), &summ[p], trace.data() + 4 * rows * p);
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::vector<double> out;
	int iterations = 0;
	for (int p = 0; p < P; ++p)
	{
		const ebo_summary& s = summ[p];
		const double head[6] = {static_cast<double>(s.iterations), static_cast<double>(s.num_evals_cost), static_cast<double>(s.num_evals_jac),
								static_cast<double>(s.termination), s.initial_cost, s.final_cost};
		out.insert(out.end(), head, head + 6);
		out.insert(out.end(), models.begin() + 12 * static_cast<size_t>(p), models.begin() + 12 * static_cast<size_t>(p) + 12);
		iterations += s.iterations;
	}
	out.insert(out.end(), trace.begin(), trace.end());
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"pairs\": %d, \"correspondences\": %zu, \"iterations\": %d, \"ms_median\": %.4f, \"repeats\": %d}\n", P, total, iterations,
				ms[ms.size() / 2], repeats);
	return 0;
}
