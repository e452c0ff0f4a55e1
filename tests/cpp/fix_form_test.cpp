// The tap-encoding rule of csrc/fix_form.h, as the host applies it (free of HIP).  For every "norm kexp guardExp"
// triple on the command line (norm as a C99 hex float) prints one line: ok, and the bit patterns of the two prefactors.
// tests/test_subnormal_taps_cpu.py compiles this, runs it and checks the lines against its own statement of the rule.
#include "../../event-based-odomety_amd/csrc/fix_form.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
	for (int i = 1; i + 2 < argc; i += 3)
	{
		const double norm = std::strtod(argv[i], nullptr);
		const int kexp = std::atoi(argv[i + 1]);
		const int guard = std::atoi(argv[i + 2]);
		const double px = ebo::fix_pre_x(norm), py = ebo::fix_pre_y(kexp);
		uint64_t bx, by;
		std::memcpy(&bx, &px, 8);
		std::memcpy(&by, &py, 8);
		std::printf("%d %016llx %016llx\n", ebo::fix_subnormal_ok(norm, kexp, guard) ? 1 : 0, static_cast<unsigned long long>(bx),
					static_cast<unsigned long long>(by));
	}
	return 0;
}
