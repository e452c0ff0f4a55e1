// The strided deal of csrc/order_deal.h as the host compiles it (free of HIP).  For every n in [argv[1], argv[2]] prints
// one line "n stride inverse".  tests/test_bucket_ref_cpu.py compiles this, runs it and compares the lines with the
// restatement of tests/bucket_ref.py.
#include "../../event-based-odomety_amd/csrc/order_deal.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
	if (argc < 3)
	{
		return 2;
	}
	const uint32_t lo = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
	const uint32_t hi = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
	for (uint32_t n = lo; n <= hi; ++n)
	{
		const uint32_t st = ebo::order_stride(n);
		std::printf("%u %u %u\n", n, st, ebo::order_inverse(st, n));
	}
	return 0;
}
