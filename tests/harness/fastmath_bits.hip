// Test harness of tests/test_gpu_fastmath_bits.py: evaluates a device library function and its range-specialised form of
// bayesssm_amd/csrc/fastmath.hip.h on the same arguments and returns both results as bit patterns.
// Built with the flags of bayesssm_amd/csrc/Makefile (-ffp-contract=off included).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "rng.h"

using namespace bssm;

__device__ __forceinline__ uint64_t bits(double x) { return (uint64_t)__double_as_longlong(x); }
__device__ __forceinline__ double val(uint64_t b) { return __longlong_as_double((long long)b); }

// fn: 0 exp / exp_nonpos, 1 sqrt / sqrt_pos_normal, 2 sincospi / sincospi_0_2 (lib, fast = sine; lib2, fast2 = cosine),
//     3 the generic u01_from_bits / u01_from_bits_dev (in = the 64 random bits)
__global__ void k_fastmath_bits(int fn, const uint64_t* __restrict__ in, long long n, uint64_t* __restrict__ lib,
                                uint64_t* __restrict__ fast, uint64_t* __restrict__ lib2, uint64_t* __restrict__ fast2)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const uint64_t b = in[i];
        const double x = val(b);
        uint64_t l = 0, f = 0, l2 = 0, f2 = 0;
        if (fn == 0) { l = bits(exp(x)); f = bits(exp_nonpos(x)); }
        else if (fn == 1) { l = bits(sqrt(x)); f = bits(sqrt_pos_normal(x)); }
        else if (fn == 2) {
            double s, c, s2, c2;
            sincospi(x, &s, &c); sincospi_0_2(x, &s2, &c2);
            l = bits(s); l2 = bits(c); f = bits(s2); f2 = bits(c2);
        } else {
            l = bits(((double)(b >> 11) + 0.5) * 0x1.0p-53);
            f = bits(u01_from_bits_dev((uint32_t)b, (uint32_t)(b >> 32)));
        }
        lib[i] = l; fast[i] = f; lib2[i] = l2; fast2[i] = f2;
    }
}

// returns 0, or the HIP error code of the first call that failed
extern "C" int fastmath_bits(int fn, const uint64_t* in, long long n, uint64_t* lib, uint64_t* fast, uint64_t* lib2, uint64_t* fast2)
{
    if (n <= 0 || fn < 0 || fn > 3) return -1;
    const size_t bytes = (size_t)n * sizeof(uint64_t);
    uint64_t* d = nullptr;
    hipError_t e = hipMalloc(&d, 5 * bytes);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(k_fastmath_bits, dim3(blocks), dim3(256), 0, 0, fn, d, n, d + n, d + 2 * n, d + 3 * n, d + 4 * n);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    uint64_t* outs[4] = {lib, fast, lib2, fast2};
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpy(outs[k], d + (size_t)(k + 1) * n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return (int)e;
}
