// freqest_pair.h -- the per-pair arithmetic of estimateFreq<int16_t, L>
// (dsptl_miscellaneous.h:43-58), written once for host and device: the kernel
// (freqest_kernels.h), the join srcdsp_demod_acquire_batched (demod.hip) and
// the host program tests/cpp/freqest_host.cpp all compile this one source.
// The two int terms as the reference forms them, termI with the two's
// complement wrap its x86 build computes at x[i] = x[i + L] = (-32768, -32768)
// (DESIGN 9), and the extremes of the terms, from which the exactness bound is
// taken (freqest_exact).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace srcdsp {

// the running sums and the extremes of the terms (both start at 0: a zero
// term changes neither)
struct FreqAcc {
    int64_t si = 0, sq = 0;
    int32_t hi = 0, lo = 0;
};

// One pair, a = x[i], b = x[i + L], packed (re, im) words
// (dsptl_miscellaneous.h:52-53).  Each product fits int; termQ cannot
// overflow; termI does at a = b = (-32768, -32768) only, where the sum is
// taken in unsigned (the wrap to -2^31).
__host__ __device__ inline void freqest_pair(FreqAcc &s, uint32_t a, uint32_t b) {
    const int ar = (int16_t)(a & 0xffffu), ai = (int32_t)a >> 16;
    const int br = (int16_t)(b & 0xffffu), bi = (int32_t)b >> 16;
    const int ti = (int)((unsigned)(ar * br) + (unsigned)(ai * bi));
    const int tq = ai * br - ar * bi;
    s.si += ti;
    s.sq += tq;
    const int mx = ti > tq ? ti : tq, mn = ti < tq ? ti : tq;
    s.hi = mx > s.hi ? mx : s.hi;
    s.lo = mn < s.lo ? mn : s.lo;
}

__host__ __device__ inline void freqest_merge(FreqAcc &s, const FreqAcc &o) {
    s.si += o.si;
    s.sq += o.sq;
    s.hi = o.hi > s.hi ? o.hi : s.hi;
    s.lo = o.lo < s.lo ? o.lo : s.lo;
}

// T, the largest |term| of a call (|-2^31| = 2^31), from the extremes
__host__ __device__ inline uint64_t freqest_bound(int64_t hi, int64_t lo) { return (uint64_t)(hi > -lo ? hi : -lo); }

// 1 iff pairs * T < 2^53: no partial sum of the reference's double
// accumulation exceeded 2^53 in magnitude, so none was rounded and the float
// is the reference's bit for bit.  pairs < 2^31 and T <= 2^31: no overflow.
__host__ __device__ inline int freqest_exact(uint64_t pairs, uint64_t T) { return pairs * T < (1ull << 53) ? 1 : 0; }

// the host form of a row (srcdsp_demod_acquire_batched, tests/cpp/freqest_host.cpp)
inline FreqAcc freqest_row_host(const uint32_t *x, size_t n, size_t L) {
    FreqAcc s;
    for (size_t i = 0; i + L < n; ++i) freqest_pair(s, x[i], x[i + L]);
    return s;
}

}  // namespace srcdsp
