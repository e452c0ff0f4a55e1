// The owner type of the context's device and pinned buffers (csrc/dev_buf.h) on the CPU, with a memory policy that
// counts its allocations and releases and can be told to fail its k-th allocation.  Every scenario ends with no
// live allocation.  Built plain and under AddressSanitizer + UBSan; run by tests/test_dev_buf_cpu.py.
#include "../../event-based-odomety_amd/csrc/dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

using namespace ebo;

namespace
{
struct FakeMem
{
	static int allocs, releases, fail_at;  // fail_at: the k-th allocation from now fails (1 = the next); 0 = none
	static size_t last_bytes;
	static void* allocate(size_t bytes)
	{
		if (fail_at > 0 && --fail_at == 0)
		{
			return nullptr;
		}
		++allocs;
		last_bytes = bytes;
		return std::malloc(bytes);
	}
	static void release(void* p)
	{
		++releases;
		std::free(p);
	}
	static int live() { return allocs - releases; }
	static void restart() { allocs = releases = fail_at = 0; }
};
int FakeMem::allocs = 0, FakeMem::releases = 0, FakeMem::fail_at = 0;
size_t FakeMem::last_bytes = 0;

template <class T>
using Buf = DevBuf<T, FakeMem>;

int failures = 0;
const char* scenario = "";
void begin(const char* name)
{
	scenario = name;
	FakeMem::restart();
}
void end()
{
	if (FakeMem::live() != 0)
	{
		std::printf("FAIL %s: %d allocations live at the end\n", scenario, FakeMem::live());
		++failures;
	}
}
#define CHECK(cond)                                                         \
	do                                                                      \
	{                                                                       \
		if (!(cond))                                                        \
		{                                                                   \
			std::printf("FAIL %s: %s (line %d)\n", scenario, #cond, __LINE__); \
			++failures;                                                     \
		}                                                                   \
	} while (0)

void fits_and_grows()
{
	begin("a buffer that fits keeps its pointer; growth releases one and makes one");
	{
		Buf<double> b;
		CHECK(b.get() == nullptr && b.cap() == 0);
		CHECK(b.ensure(0) == Grow::kOk && FakeMem::allocs == 0);
		CHECK(b.ensure(100) == Grow::kOk);
		CHECK(b.cap() == 100 && FakeMem::last_bytes == 100 * sizeof(double));  // capacity in elements
		double* const p = b.get();
		p[99] = 1.0;
		CHECK(b.ensure(100) == Grow::kOk && b.ensure(7) == Grow::kOk && b.ensure(100, false) == Grow::kOk);
		CHECK(b.get() == p && b.cap() == 100 && FakeMem::allocs == 1 && FakeMem::releases == 0);
		CHECK(static_cast<double*>(b) == p);
		CHECK(b.ensure(101) == Grow::kOk);
		CHECK(b.cap() == 101 && FakeMem::allocs == 2 && FakeMem::releases == 1);
		b.get()[100] = 2.0;
		Buf<void> bytes;  // void and char count bytes
		CHECK(bytes.ensure(33) == Grow::kOk && FakeMem::last_bytes == 33 && bytes.cap() == 33);
		Buf<char> chars;
		CHECK(chars.ensure(5) == Grow::kOk && FakeMem::last_bytes == 5);
		bytes.reset();
		CHECK(bytes.get() == nullptr && bytes.cap() == 0 && FakeMem::releases == 2);
		bytes.reset();
		CHECK(FakeMem::releases == 2);
	}
	CHECK(FakeMem::allocs == 4 && FakeMem::releases == 4);  // the destructors released the other two
	end();
}

void failed_growth()
{
	begin("a failed growth leaves {nullptr, 0} and the next ensure works");
	{
		Buf<int> b;
		CHECK(b.ensure(10) == Grow::kOk);
		FakeMem::fail_at = 1;
		CHECK(b.ensure(20) == Grow::kFailed);
		CHECK(b.get() == nullptr && b.cap() == 0);
		CHECK(FakeMem::allocs == 1 && FakeMem::releases == 1);  // released first, as when it succeeds
		CHECK(b.ensure(20) == Grow::kOk && b.cap() == 20);
		b.get()[19] = 3;
		FakeMem::fail_at = 1;
		Buf<int> fresh;
		CHECK(fresh.ensure(1) == Grow::kFailed && fresh.get() == nullptr && fresh.cap() == 0);
	}
	end();
}

void refusal()
{
	begin("allocation not allowed: a buffer that is too small is refused and untouched");
	{
		Buf<double> b;
		CHECK(b.ensure(1, false) == Grow::kRefused && b.get() == nullptr && b.cap() == 0 && FakeMem::allocs == 0);
		CHECK(b.ensure(8) == Grow::kOk);
		double* const p = b.get();
		CHECK(b.ensure(9, false) == Grow::kRefused);
		CHECK(b.get() == p && b.cap() == 8 && FakeMem::allocs == 1 && FakeMem::releases == 0);
		CHECK(b.ensure(8, false) == Grow::kOk);
		CHECK(Grow::kRefused != Grow::kFailed);
	}
	end();
}

void move_and_swap()
{
	begin("move and swap transfer ownership once");
	{
		Buf<char> a;
		CHECK(a.ensure(16) == Grow::kOk);
		char* const pa = a.get();
		Buf<char> b(std::move(a));
		CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 16);
		Buf<char> c;
		CHECK(c.ensure(4) == Grow::kOk);
		char* const pc = c.get();
		c = std::move(b);  // c's own block is released, b's moves in
		CHECK(c.get() == pa && c.cap() == 16 && b.get() == nullptr && b.cap() == 0);
		CHECK(FakeMem::allocs == 2 && FakeMem::releases == 1);
		(void)pc;
		// the collective growth of the exchange buffer: a local takes the new block, the ranks agree, swap
		Buf<char> fresh;
		CHECK(fresh.ensure(64) == Grow::kOk);
		char* const pf = fresh.get();
		c.swap(fresh);
		CHECK(c.get() == pf && c.cap() == 64 && fresh.get() == pa && fresh.cap() == 16);
		CHECK(FakeMem::allocs == 3 && FakeMem::releases == 1);
	}
	CHECK(FakeMem::allocs == 3 && FakeMem::releases == 3);
	end();
}

// the pinned staging of an evaluation round: flows [nf][2], results [nf][3], mode tables [4][nf]
Grow staging(Buf<double>& flows, Buf<double>& out, Buf<unsigned char>& modes, size_t nf, bool mayAllocate = true)
{
	return ensure3(flows, nf * 2, out, nf * 3, modes, nf * 4, mayAllocate);
}

void three_blocks()
{
	for (int failAt = 0; failAt <= 3; ++failAt)
	{
		begin("three blocks with one logical size: all or nothing");
		{
			Buf<double> flows, out;
			Buf<unsigned char> modes;
			CHECK(staging(flows, out, modes, 10) == Grow::kOk);
			CHECK(flows.cap() == 20 && out.cap() == 30 && modes.cap() == 40 && FakeMem::allocs == 3);
			double* const pf = flows.get();
			CHECK(staging(flows, out, modes, 10) == Grow::kOk && staging(flows, out, modes, 3) == Grow::kOk);
			CHECK(flows.get() == pf && FakeMem::allocs == 3 && FakeMem::releases == 0);
			CHECK(staging(flows, out, modes, 11, false) == Grow::kRefused);
			CHECK(flows.get() == pf && flows.cap() == 20 && out.cap() == 30 && modes.cap() == 40 && FakeMem::releases == 0);
			FakeMem::fail_at = failAt;
			const Grow g = staging(flows, out, modes, 11);
			if (failAt == 0)
			{
				CHECK(g == Grow::kOk && flows.cap() == 22 && out.cap() == 33 && modes.cap() == 44);
				CHECK(FakeMem::allocs == 6 && FakeMem::releases == 3);
			}
			else
			{
				CHECK(g == Grow::kFailed);
				CHECK(!flows.get() && !out.get() && !modes.get() && flows.cap() == 0 && out.cap() == 0 && modes.cap() == 0);
				CHECK(FakeMem::live() == 0);  // nothing is left allocated after a failure part-way
				CHECK(staging(flows, out, modes, 11) == Grow::kOk && out.cap() == 33);
			}
		}
		end();
	}
}
}  // namespace

int main()
{
	fits_and_grows();
	failed_growth();
	refusal();
	move_and_swap();
	three_blocks();
	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
