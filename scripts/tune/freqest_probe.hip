// freqest_probe.hip -- what binds freqest_rows?  The kernel source as shipped
// (freqest_kernels.h) with the per-pair function swapped at compile time:
//   VARIANT 0 the product; 1 loads only (one xor per pair); 2 no extremes;
//   3 32-bit sums (wrong, cost only); 4 termI by v_dot2_i32_i16.
// One row of 2^28 samples, 30 warm-up and 50 timed launches between HIP events:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DVARIANT=v scripts/tune/freqest_probe.hip -o probe_v
//   ./probe_v [L] [workgroups per CU]
// Results: profiles/tuning/freqest_probe.txt.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "../../srcdsp_amd/csrc/freqest_pair.h"
namespace srcdsp {
#if VARIANT == 1
__device__ inline void probe_pair(FreqAcc &s, uint32_t a, uint32_t b) { s.hi ^= (int)(a ^ b); }
#elif VARIANT == 2  // terms and 64-bit sums, no extremes
__device__ inline void probe_pair(FreqAcc &s, uint32_t a, uint32_t b) {
    const int ar = (int16_t)(a & 0xffffu), ai = (int32_t)a >> 16;
    const int br = (int16_t)(b & 0xffffu), bi = (int32_t)b >> 16;
    const int ti = (int)((unsigned)(ar * br) + (unsigned)(ai * bi));
    const int tq = ai * br - ar * bi;
    s.si += ti; s.sq += tq;
}
#elif VARIANT == 3  // terms, 32-bit sums (wrong, cost only), extremes
__device__ inline void probe_pair(FreqAcc &s, uint32_t a, uint32_t b) {
    const int ar = (int16_t)(a & 0xffffu), ai = (int32_t)a >> 16;
    const int br = (int16_t)(b & 0xffffu), bi = (int32_t)b >> 16;
    const int ti = (int)((unsigned)(ar * br) + (unsigned)(ai * bi));
    const int tq = ai * br - ar * bi;
    s.si = (int64_t)(int32_t)((uint32_t)s.si + (uint32_t)ti); s.sq = (int64_t)(int32_t)((uint32_t)s.sq + (uint32_t)tq);
    const int mx = ti > tq ? ti : tq, mn = ti < tq ? ti : tq;
    s.hi = mx > s.hi ? mx : s.hi; s.lo = mn < s.lo ? mn : s.lo;
}
#elif VARIANT == 4  // dot2 for termI
__device__ inline void probe_pair(FreqAcc &s, uint32_t a, uint32_t b) {
    typedef short s2 __attribute__((ext_vector_type(2)));
    const int ar = (int16_t)(a & 0xffffu), ai = (int32_t)a >> 16;
    const int br = (int16_t)(b & 0xffffu), bi = (int32_t)b >> 16;
    const int ti = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, a), __builtin_bit_cast(s2, b), 0, false);
    const int tq = ai * br - ar * bi;
    s.si += ti; s.sq += tq;
    const int mx = ti > tq ? ti : tq, mn = ti < tq ? ti : tq;
    s.hi = mx > s.hi ? mx : s.hi; s.lo = mn < s.lo ? mn : s.lo;
}
#endif
}
#if VARIANT != 0
#define freqest_pair probe_pair
#endif
#include "../../srcdsp_amd/csrc/freqest_kernels.h"
using namespace srcdsp;
#define CK(e) do { hipError_t r = (e); if (r != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r)); return 1; } } while (0)
int main(int argc, char **argv) {
    const long n = 1L << 28, L = argc > 1 ? atol(argv[1]) : 1;
    const int wgpc = argc > 2 ? atoi(argv[2]) : 8;
    uint32_t *x; long long *slab, *res;
    CK(hipMalloc(&x, 4 * n)); CK(hipMemset(x, 0x5a, 4 * n));
    const long pairs = n - L, ntiles = (pairs + kFreqTile - 1) / kFreqTile;
    long bpr = 256L * wgpc; if (bpr > ntiles) bpr = ntiles;
    const long tpw = (ntiles + bpr - 1) / bpr; bpr = (ntiles + tpw - 1) / tpw;
    CK(hipMalloc(&slab, 32 * bpr)); CK(hipMalloc(&res, 32));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 30; ++i) hipLaunchKernelGGL(freqest_rows, dim3(bpr), dim3(kFreqLanes), 0, 0, x, 0L, nullptr, n, L, (int)bpr, tpw, slab, res);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    const int reps = 50;
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(freqest_rows, dim3(bpr), dim3(kFreqLanes), 0, 0, x, 0L, nullptr, n, L, (int)bpr, tpw, slab, res);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    printf("variant %d L %ld wg/cu %d bpr %ld: %.4f ms per launch, %.3f TB/s\n", VARIANT, L, wgpc, bpr, ms / reps, 4.0 * n / (ms / reps * 1e-3) / 1e12);
    return 0;
}
