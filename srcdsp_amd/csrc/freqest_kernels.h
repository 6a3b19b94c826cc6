// freqest_kernels.h -- estimateFreq<int16_t, L> (dsptl_miscellaneous.h:43-58)
// as an order-free integer reduction: the lag-L autocorrelation
//   sumI + j sumQ = sum over i < n - L of x[i] * conj(x[i + L])
// taken in 64-bit integers, the atan2 left to the host.
//
// The per-pair arithmetic is freqest_pair (freqest_pair.h), one source for
// host and device.
//
// freqest_rows reduces C rows in one launch; the single-row call is the bank at
// one row.  A row of n samples has n - L pairs, cut into tiles of kFreqTile
// pairs; every row is given `bpr` workgroups, each a contiguous run of tiles.
// A lane reads 4 samples with one 16-byte load (4-byte aligned: a row may start
// at any sample) and their partners at + L with a second one, which finds the
// line the first load of this or a neighbouring lane brought in: HBM sees the
// buffer once.  A load that would pass the end of the row is replaced by
// guarded single loads that give zero words, and a pair with a zero word adds
// nothing to either sum or to the extremes, so neither a pair nor a load
// leaves the row.  Lanes accumulate in 64 bits, waves reduce by shuffles, the
// workgroup through LDS; a row with one workgroup writes its result row, any
// other its slab, which freqest_finish sums.  Every word is written on every
// call.
#pragma once
#include "freqest_pair.h"

namespace srcdsp {

constexpr int kFreqLanes = 256;   // lanes per workgroup
constexpr int kFreqVec = 4;       // samples per load (16 bytes)
constexpr int kFreqUnroll = 4;    // loads of a lane in flight per tile
constexpr int kFreqTile = kFreqLanes * kFreqVec * kFreqUnroll;  // pairs per tile: 4096
constexpr int kFreqWgPerCu = 8;   // persistent workgroups per compute unit
constexpr int kFreqWords = 4;     // int64 words of a result row / a slab: sumI, sumQ, hi, lo

struct __attribute__((packed, aligned(4))) FreqVec {
    uint32_t w[kFreqVec];
};

// samples i .. i + 3 of a row of n; words past the row's end read as zero
__device__ __forceinline__ void freqest_load(const uint32_t *__restrict__ row, long i, long n, uint32_t (&w)[kFreqVec]) {
    if (i + kFreqVec <= n) {
        const FreqVec v = *(const FreqVec *)(row + i);
#pragma unroll
        for (int e = 0; e < kFreqVec; ++e) w[e] = v.w[e];
    } else {
#pragma unroll
        for (int e = 0; e < kFreqVec; ++e) w[e] = i + e < n ? row[i + e] : 0u;
    }
}

__device__ __forceinline__ FreqAcc freqest_wave_sum(FreqAcc s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        FreqAcc o;
        o.si = __shfl_down((long long)s.si, d, 64);
        o.sq = __shfl_down((long long)s.sq, d, 64);
        o.hi = __shfl_down(s.hi, d, 64);
        o.lo = __shfl_down(s.lo, d, 64);
        freqest_merge(s, o);
    }
    return s;
}

__device__ __forceinline__ void freqest_store(long long *__restrict__ p, const FreqAcc &s) {
    p[0] = s.si;
    p[1] = s.sq;
    p[2] = s.hi;
    p[3] = s.lo;
}

// grid: channels * bpr workgroups; n > L.  Row c starts at in + c * in_stride +
// (row_off ? row_off[c] : 0).  Workgroup b of a row takes tiles
// [b * tiles_per_wg, (b + 1) * tiles_per_wg) of its ceil((n - L) / kFreqTile).
__global__ __launch_bounds__(kFreqLanes) void freqest_rows(const uint32_t *__restrict__ in, long in_stride,
                                                           const long *__restrict__ row_off, long n, long L, int bpr,
                                                           long tiles_per_wg, long long *__restrict__ slab,
                                                           long long *__restrict__ res) {
    __shared__ long long part[kFreqLanes / 64][kFreqWords];
    const int lane = threadIdx.x;
    const long c = blockIdx.x / (unsigned)bpr, b = blockIdx.x % (unsigned)bpr;
    const uint32_t *__restrict__ row = in + c * in_stride + (row_off ? row_off[c] : 0);
    const long pairs = n - L;
    const long ntiles = (pairs + kFreqTile - 1) / kFreqTile;
    const long t0 = b * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    FreqAcc s;
    for (long t = t0; t < t1; ++t) {
        uint32_t a[kFreqUnroll][kFreqVec], p[kFreqUnroll][kFreqVec];
#pragma unroll
        for (int u = 0; u < kFreqUnroll; ++u) {
            const long i = t * kFreqTile + ((long)u * kFreqLanes + lane) * kFreqVec;
            if (i < pairs) {
                freqest_load(row, i, n, a[u]);
                freqest_load(row, i + L, n, p[u]);
            } else {
#pragma unroll
                for (int e = 0; e < kFreqVec; ++e) a[u][e] = p[u][e] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kFreqUnroll; ++u)
#pragma unroll
            for (int e = 0; e < kFreqVec; ++e) freqest_pair(s, a[u][e], p[u][e]);
    }
    s = freqest_wave_sum(s);
    if ((lane & 63) == 0) freqest_store(part[lane >> 6], s);
    __syncthreads();
    if (lane != 0) return;
    for (int w = 1; w < kFreqLanes / 64; ++w) {
        FreqAcc o;
        o.si = part[w][0];
        o.sq = part[w][1];
        o.hi = (int32_t)part[w][2];
        o.lo = (int32_t)part[w][3];
        freqest_merge(s, o);
    }
    freqest_store(bpr == 1 ? res + kFreqWords * c : slab + kFreqWords * (long)blockIdx.x, s);
}

// grid: channels workgroups of one wave; row c's bpr slabs into its result row
__global__ __launch_bounds__(64) void freqest_finish(const long long *__restrict__ slab, int bpr,
                                                     long long *__restrict__ res) {
    const long c = blockIdx.x;
    FreqAcc s;
    for (int b = threadIdx.x; b < bpr; b += 64) {
        const long long *p = slab + kFreqWords * (c * bpr + b);
        FreqAcc o;
        o.si = p[0];
        o.sq = p[1];
        o.hi = (int32_t)p[2];
        o.lo = (int32_t)p[3];
        freqest_merge(s, o);
    }
    s = freqest_wave_sum(s);
    if (threadIdx.x == 0) freqest_store(res + kFreqWords * c, s);
}

}  // namespace srcdsp
