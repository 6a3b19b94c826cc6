// decim_tile_kernels.h -- the decimators off the persistent kernels' shapes:
// decim_tile (any tap count at M = 1..6, 8, 16, one tile per workgroup) and
// decim_generic (any variant / M / N, one output per thread).  See decim.hip
// for the semantics.
#pragma once
#include "fir_device.h"

namespace srcdsp {

// ================================================================ generic
template <int KV, bool FMA>
__global__ void decim_generic(DecimLaunch a, unsigned M) {
    const int ch = blockIdx.y;
    const int N = a.ntaps, H = N - 1;
    const long n_out = a.n_out, n_in = a.n_in;
    if (blockIdx.x == 0) {
        if constexpr (KV == KV_CF32 || KV == KV_CI32_I32) {
            write_history((const uint2 *)a.in + ch * a.in_stride, n_in, (const uint2 *)a.hist_in[ch],
                          (uint2 *)a.hist_out[ch], H);
        } else {
            write_history((const uint32_t *)a.in + ch * a.in_stride, n_in, (const uint32_t *)a.hist_in[ch],
                          (uint32_t *)a.hist_out[ch], H);
        }
    }
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += (long)gridDim.x * blockDim.x) {
        const long j = o * (long)M;
        if constexpr (KV == KV_CF32) {
            const float2 *in = (const float2 *)a.in + ch * a.in_stride;
            const float2 *hist = (const float2 *)a.hist_in[ch];
            const float *c = (const float *)a.coef;
            float yr = 0.f, yi = 0.f;
            for (int k = 0; k < N; ++k) {
                float2 x = fetch(in, hist, j - k, n_in, H);
                yr = mac<FMA>(c[k], x.x, yr);
                yi = mac<FMA>(c[k], x.y, yi);
            }
            ((float2 *)a.out + ch * a.out_stride)[o] = make_float2(q16f(yr, a.shift), q16f(yi, a.shift));
        } else if constexpr (KV == KV_F32_REAL) {
            const float *in = (const float *)a.in + ch * a.in_stride;
            const float *hist = (const float *)a.hist_in[ch];
            const float *c = (const float *)a.coef;
            float y = 0.f;
            for (int k = 0; k < N; ++k) y = mac<FMA>(c[k], fetch(in, hist, j - k, n_in, H), y);
            ((float2 *)a.out + ch * a.out_stride)[o] = make_float2(q16f(y, a.shift), 0.f);
        } else if constexpr (KV == KV_CI32_I32) {
            const int2 *in = (const int2 *)a.in + ch * a.in_stride;
            const int2 *hist = (const int2 *)a.hist_in[ch];
            const int32_t *c = (const int32_t *)a.coef;
            uint32_t yr = 0, yi = 0;
            for (int k = 0; k < N; ++k) {
                int2 x = fetch(in, hist, j - k, n_in, H);
                yr += (uint32_t)c[k] * (uint32_t)x.x;
                yi += (uint32_t)c[k] * (uint32_t)x.y;
            }
            ((uint32_t *)a.out + ch * a.out_stride)[o] =
                pack16(limit16((int32_t)yr, a.shift), limit16((int32_t)yi, a.shift));
        } else {  // KV_CI16_I32, KV_CI16_I16
            const uint32_t *in = (const uint32_t *)a.in + ch * a.in_stride;
            const uint32_t *hist = (const uint32_t *)a.hist_in[ch];
            const int32_t *c = (const int32_t *)a.coef;
            uint32_t yr = 0, yi = 0;
            for (int k = 0; k < N; ++k) {
                uint32_t w = fetch(in, hist, j - k, n_in, H);
                uint32_t pr = (uint32_t)c[k] * (uint32_t)sext16(w);
                uint32_t pi = (uint32_t)c[k] * (uint32_t)sext16_hi(w);
                if constexpr (KV == KV_CI16_I16) {  // std::operator*(short, complex<short>): int16 wrap
                    pr = (uint32_t)sext16(pr);
                    pi = (uint32_t)sext16(pi);
                }
                yr += pr;
                yi += pi;
            }
            ((uint32_t *)a.out + ch * a.out_stride)[o] =
                pack16(limit16((int32_t)yr, a.shift), limit16((int32_t)yi, a.shift));
        }
    }
}

// Tiled decimator for any tap count (<= kDtMaxTaps) at M in {2, 4, 8}
// (dnsampling_filters.h:129-172 off the headline's 127/128-tap M=4 shape),
// complex<float> (KV_CF32; P = 1: fma chain, 0: mul+add) or complex<int16_t>
// with int32 (KV_CI16_I32; P = 0: |c| < 2^23 as v_mad_i32_i24, 1: full 32-bit
// products) or int16 taps (KV_CI16_I16, P = 2: products wrapped to int16).
// A lane owns R = 16/M consecutive outputs, i.e. one 16-sample block b = lane
// of the tile's input image; output r, tap k reads sample r*M - k of the
// lane's block frame.  Taps run in chunks of 16 (one SGPR s_load each); chunk
// c touches blocks b-c ("cur") and b-c-1 ("nxt"), so three 16-sample register
// windows rotate over the chunks (the next chunk's window is read from LDS
// while this one's MACs run).  Each output is one sequential chain in
// ascending k; taps past N are skipped, never multiplied by zero (0 * inf
// would differ).  ci16 samples are split into int32 (re, im) while staging,
// so the image has the cf32 layout: LDS blocks are 8 granules + one pad
// granule and the lanes' ds_read_b128 are conflict-free.  One tile per
// workgroup; the image holds ceil(N/16) halo blocks before the tile.
constexpr int kDtBlock = 256, kDtMaxTaps = 1024;
// samples per lane block: a multiple of M and of 4 (an even number of 16-B
// granules, so the padded block stride RM/2 + 1 is odd: conflict-free reads)
__host__ __device__ constexpr int dt_rm(int M) { return M <= 2 || M == 4 ? 8 : (M == 3 || M == 6 ? 12 : (M == 5 ? 20 : 16)); }
__host__ __device__ constexpr int dt_bs(int M) { return dt_rm(M) / 2 + 1; }  // LDS granules per block

template <int KV, int M, int P>
__global__ __launch_bounds__(kDtBlock) void decim_tile(DecimLaunch a) {
    constexpr int RM = dt_rm(M), BS = dt_bs(M);
    static_assert(RM % M == 0 && RM % 4 == 0, "block geometry");
    static_assert(KV == KV_CF32 || KV == KV_CI16_I32 || KV == KV_CI16_I16, "sample kinds");
    constexpr bool CF = KV == KV_CF32;
    typedef typename std::conditional<CF, float2, int2>::type X2;
    typedef typename std::conditional<CF, float2, uint32_t>::type SIn;
    constexpr int R = RM / M, TO = kDtBlock * R;
    extern __shared__ float4 dimg[];
    const int ch = blockIdx.y;
    const SIn *in = (const SIn *)a.in + ch * a.in_stride;
    const SIn *hist = (const SIn *)a.hist_in[ch];
    const long n_in = a.n_in;
    const int N = a.ntaps, H = N - 1;
    const int NCH = (N + RM - 1) / RM;  // tap chunks = halo blocks
    const int t = threadIdx.x;
    const long tile = blockIdx.x;
    if (tile == 0) write_history(in, n_in, hist, (SIn *)a.hist_out[ch], H);
    // image block i holds samples s0 + 16 i .. s0 + 16 i + 15, as (re, im) pairs
    const long s0 = tile * (long)TO * M - (long)NCH * RM;
    const int NG = (NCH + kDtBlock) * (RM / 2);  // 2-sample granules
    auto put = [&](int g, float4 v) { dimg[(g / (RM / 2)) * BS + g % (RM / 2)] = v; };
    auto split = [&](uint32_t w0, uint32_t w1) {
        return make_float4(__int_as_float(sext16(w0)), __int_as_float(sext16_hi(w0)), __int_as_float(sext16(w1)),
                           __int_as_float(sext16_hi(w1)));
    };
    // the tile's own span (every tile but the launch's last lies inside the
    // input): all RM/2 granule loads of a lane issued before any lands in LDS
    const int G0 = NCH * (RM / 2);
    const bool body_in = (tile + 1) * (long)TO * M <= n_in;
    if (body_in) {
        float4 v[RM / 2];
#pragma unroll
        for (int i = 0; i < RM / 2; ++i) {
            const long s = s0 + 2L * (G0 + t + i * kDtBlock);
            // complex<float>: non-temporal, the body is read once (the halo
            // re-read is an L2 hit): 4 % at M = 2/4 x 63 taps; complex<int16_t>
            // measured 0-5 % slower with it (profiles/tuning/r02_tile_nt_ab.txt)
            if constexpr (CF) {
                v[i] = nt_load4((const float4 *)(in + s));
            } else {
                const uint2 w = *(const uint2 *)(in + s);
                v[i] = split(w.x, w.y);
            }
        }
#pragma unroll
        for (int i = 0; i < RM / 2; ++i) put(G0 + t + i * kDtBlock, v[i]);
    }
    for (int g = t; g < (body_in ? G0 : NG); g += kDtBlock) {
        const long s = s0 + 2L * g;
        float4 v;
        if constexpr (CF) {
            if (s >= 0 && s + 1 < n_in) {
                v = *(const float4 *)(in + s);
            } else {
                const float2 lo = fetch(in, hist, s, n_in, H), hi = fetch(in, hist, s + 1, n_in, H);
                v = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        } else {
            uint32_t w0, w1;
            if (s >= 0 && s + 1 < n_in) {
                const uint2 w = *(const uint2 *)(in + s);
                w0 = w.x;
                w1 = w.y;
            } else {
                w0 = fetch(in, hist, s, n_in, H);
                w1 = fetch(in, hist, s + 1, n_in, H);
            }
            v = split(w0, w1);
        }
        put(g, v);
    }
    __syncthreads();
    X2 W0[RM], W1[RM], W2[RM];
    auto load = [&](X2 (&w)[RM], int blk) {
#pragma unroll
        for (int i = 0; i < RM / 2; ++i) {
            const float4 v = dimg[blk * BS + i];
            if constexpr (CF) {
                w[2 * i] = make_float2(v.x, v.y);
                w[2 * i + 1] = make_float2(v.z, v.w);
            } else {
                w[2 * i] = make_int2(__float_as_int(v.x), __float_as_int(v.y));
                w[2 * i + 1] = make_int2(__float_as_int(v.z), __float_as_int(v.w));
            }
        }
    };
    typedef typename std::conditional<CF, float, uint32_t>::type Acc;
    Acc yr[R], yi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) yr[r] = yi[r] = Acc{};
    const int me = NCH + t;  // the lane's own block
    typedef typename std::conditional<CF, float, int32_t>::type Tap;
    ConstPtr<Tap> tp = const_view<Tap>(a.coef);
    auto chunk = [&](int c, const X2 (&cur)[RM], const X2 (&nxt)[RM], X2 (&nn)[RM]) {
        asm volatile("" : "+s"(tp));
        if (c + 1 < NCH) load(nn, me - c - 2);
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const int k = c * RM + i;
            if (k >= N) break;
            const Tap cf = tp[k];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int l = r * M - i;
                const X2 x = l >= 0 ? cur[l] : nxt[l + RM];
                if constexpr (CF) {
                    yr[r] = mac<P == 1>(cf, x.x, yr[r]);
                    yi[r] = mac<P == 1>(cf, x.y, yi[r]);
                } else if constexpr (P == 0) {  // |c| < 2^23: the low 32 bits of the exact product
                    yr[r] += (uint32_t)__mul24(cf, x.x);
                    yi[r] += (uint32_t)__mul24(cf, x.y);
                } else if constexpr (P == 1) {
                    yr[r] += (uint32_t)cf * (uint32_t)x.x;
                    yi[r] += (uint32_t)cf * (uint32_t)x.y;
                } else {  // std::operator*(short, complex<short>): int16 wrap
                    yr[r] += (uint32_t)sext16((uint32_t)__mul24(cf, x.x));
                    yi[r] += (uint32_t)sext16((uint32_t)__mul24(cf, x.y));
                }
            }
        }
    };
    load(W0, me);
    load(W1, me - 1);
    int c = 0;
    for (; c + 3 <= NCH; c += 3) {
        chunk(c, W0, W1, W2);
        chunk(c + 1, W1, W2, W0);
        chunk(c + 2, W2, W0, W1);
    }
    if (c < NCH) chunk(c, W0, W1, W2);
    if (c + 1 < NCH) chunk(c + 1, W1, W2, W0);
    const long o0 = tile * TO + (long)t * R;
    if constexpr (CF) {
        float2 *out = (float2 *)a.out + ch * a.out_stride;
        if (R % 2 == 0 && o0 + R <= a.n_out) {
#pragma unroll
            for (int r = 0; r + 1 < R; r += 2)
                store16<true>((float4 *)(out + o0 + r), make_float4(q16f(yr[r], a.shift), q16f(yi[r], a.shift),
                                                                    q16f(yr[r + 1], a.shift), q16f(yi[r + 1], a.shift)));
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (o0 + r < a.n_out) out[o0 + r] = make_float2(q16f(yr[r], a.shift), q16f(yi[r], a.shift));
        }
    } else {
        uint32_t *out = (uint32_t *)a.out + ch * a.out_stride;
        uint32_t w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = pack16(limit16((int32_t)yr[r], a.shift), limit16((int32_t)yi[r], a.shift));
        if (R % 2 == 0 && o0 + R <= a.n_out) {
#pragma unroll
            for (int r = 0; r + 1 < R; r += 2) *(uint2 *)(out + o0 + r) = make_uint2(w[r], w[r + 1]);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (o0 + r < a.n_out) out[o0 + r] = w[r];
        }
    }
}

}  // namespace srcdsp
