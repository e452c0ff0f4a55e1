// Microbenchmark: does gfx950 multiply f64 into SUBNORMAL results at the rate of normal ones?
// The gate of DESIGN.md section 4.1 item 14 (a tap's fixed-point word as the bit pattern of a subnormal product).
// The kernels' occupancy: 256 workgroups of 1024 lanes = 16 waves per CU, four per SIMD.  Three straight-line loops of
// 49 independent operations per trip on the same 7 + 7 register inputs (the outer product of two axes' weights):
//   (a) fma(wx, wy, 1.5) and a 32-bit subtract on the high dword     -- the biased form of fix_tap
//   (b) wx * wy with the inputs scaled so that every product is subnormal
//   (c) wx * wy with normal products                                   -- the same kernel as (b), other arguments
// Every loop stores one xor of its results at the end.  Three repeats of each, interleaved.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off subnormal_mul.hip -o subnormal_mul
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int kThreads = 1024;
constexpr int kBlocks = 256;
constexpr int kTrips = 4096;

// the inputs may have changed (they have not): the products are not loop invariant
__device__ __forceinline__ void touch(double& x) { asm volatile("" : "+v"(x)); }
// the result is needed (by nobody): the operation is not dead
__device__ __forceinline__ void use(unsigned long long x) { asm volatile("" : : "v"(x)); }

template <bool BIASED>
__device__ __forceinline__ unsigned long long tap(double wx, double wy, double bias, int biasHi)
{
	if (BIASED)
	{
		const double b = fma(wx, wy, bias);
		unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - biasHi);
		asm volatile("" : "+v"(hi));  // ONE 32-bit subtract, as keep32 in ebo_kernels.hip
		return (static_cast<unsigned long long>(hi) << 32) | static_cast<unsigned int>(__double2loint(b));
	}
	return static_cast<unsigned long long>(__double_as_longlong(wx * wy));
}

template <bool BIASED>
__global__ __launch_bounds__(kThreads) void k_taps(unsigned long long* out, double sx, double sy, double bias, int trips)
{
	double wx[7], wy[7];
#pragma unroll
	for (int i = 0; i < 7; ++i)
	{
		// weights of the size the kernels see (norm = 1 / (2 pi) at sigma 1, outer taps e^-4.5 of the centre), per lane
		wx[i] = sx * (0.159 * exp(-0.5 * (i - 3.3) * (i - 3.3)) + 1e-6 * threadIdx.x);
		wy[i] = sy * (exp(-0.5 * (i - 2.6) * (i - 2.6)) + 1e-6 * threadIdx.x);
	}
	const int biasHi = __double2hiint(bias);
	for (int t = 0; t < trips; ++t)
	{
#pragma unroll
		for (int i = 0; i < 7; ++i)
		{
			touch(wx[i]);
			touch(wy[i]);
		}
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				const unsigned long long q = tap<BIASED>(wx[i], wy[j], bias, biasHi);
				use(q);  // (one register pair, as ds_add_u64 takes it)
			}
		}
	}
	// (fresh inputs for the compiler: the loop's last results are not kept for this)
#pragma unroll
	for (int i = 0; i < 7; ++i)
	{
		touch(wx[i]);
		touch(wy[i]);
	}
	unsigned long long x = 0;
#pragma unroll
	for (int j = 0; j < 7; ++j)
	{
#pragma unroll
		for (int i = 0; i < 7; ++i)
		{
			x ^= tap<BIASED>(wx[i], wy[j], bias, biasHi);
		}
	}
	out[blockIdx.x * kThreads + threadIdx.x] = x;
}

template <typename K>
double run(K kern, unsigned long long* out, double sx, double sy, double bias)
{
	hipEvent_t e0, e1;
	CHECK(hipEventCreate(&e0));
	CHECK(hipEventCreate(&e1));
	CHECK(hipEventRecord(e0));
	hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kThreads), 0, 0, out, sx, sy, bias, kTrips);
	CHECK(hipEventRecord(e1));
	CHECK(hipEventSynchronize(e1));
	float ms;
	CHECK(hipEventElapsedTime(&ms, e0, e1));
	CHECK(hipEventDestroy(e0));
	CHECK(hipEventDestroy(e1));
	// one SIMD issues the operations of its four waves one after the other: time per wave-level operation on a SIMD
	return double(ms) * 1e6 / (double(kTrips) * 49.0 * (kThreads / 64 / 4));
}

int main()
{
	unsigned long long* out = nullptr;
	CHECK(hipMalloc(&out, size_t(kBlocks) * kThreads * sizeof(unsigned long long)));
	const double sub = std::ldexp(1.0, -511);
	// warm-up: code objects loaded, clocks up
	for (int r = 0; r < 2; ++r)
	{
		run(k_taps<true>, out, 1.0, 1.0, 1.5);
		run(k_taps<false>, out, sub, sub, 0.0);
		run(k_taps<false>, out, 1.0, 1.0, 0.0);
	}
	double a[3], b[3], c[3];
	for (int r = 0; r < 3; ++r)
	{
		a[r] = run(k_taps<true>, out, 1.0, 1.0, 1.5);
		b[r] = run(k_taps<false>, out, sub, sub, 0.0);
		c[r] = run(k_taps<false>, out, 1.0, 1.0, 0.0);
	}
	CHECK(hipDeviceSynchronize());
	// the subnormal products are what the encoding says: one lane's xor, read back, is neither 0 nor a normal number's bits
	unsigned long long h = 0;
	run(k_taps<false>, out, sub, sub, 0.0);
	CHECK(hipMemcpy(&h, out, sizeof h, hipMemcpyDeviceToHost));
	printf("# %d workgroups x %d lanes (16 waves per CU), %d trips x 49 operations per lane; ns per wave-level operation on a SIMD\n",
		   kBlocks, kThreads, kTrips);
	printf("# (4 clocks at 2.4 GHz = 1.67 ns)\n");
	printf("%-44s %8s %8s %8s\n", "loop", "run 1", "run 2", "run 3");
	printf("%-44s %8.3f %8.3f %8.3f\n", "(a) v_fma_f64 + 32-bit subtract", a[0], a[1], a[2]);
	printf("%-44s %8.3f %8.3f %8.3f\n", "(b) v_mul_f64, subnormal products", b[0], b[1], b[2]);
	printf("%-44s %8.3f %8.3f %8.3f\n", "(c) v_mul_f64, normal products", c[0], c[1], c[2]);
	const double cSpread = *std::max_element(c, c + 3) - *std::min_element(c, c + 3);
	const double bMed = std::max(std::min(b[0], b[1]), std::min(std::max(b[0], b[1]), b[2]));
	const double cMed = std::max(std::min(c[0], c[1]), std::min(std::max(c[0], c[1]), c[2]));
	printf("median (b) - median (c) = %+.3f ns, spread of (c) = %.3f ns: %s\n", bMed - cMed, cSpread,
		   bMed - cMed > cSpread ? "SLOWER (subnormal results are assisted)" : "same rate");
	printf("xor of lane 0's 49 subnormal products: 0x%016llx (high dword below 0x00100000: subnormal)\n", h);
	CHECK(hipFree(out));
	return 0;
}
