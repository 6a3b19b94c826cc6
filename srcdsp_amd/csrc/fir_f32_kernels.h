// fir_f32_kernels.h -- the single-rate float FIR (FilterFir on float input):
// fir_tile_f32 and the persistent fir_stream_f32.  See decim.hip for the
// semantics.
#pragma once
#include "fir_device.h"

namespace srcdsp {

// ------------------------------------------------------ single-rate float FIR
// FilterFir (filters.h:133-169) for float input -> complex<float> output
// with a zero imaginary part (KV_F32_REAL), any tap count up to kFirMaxTaps
// (runtime).  complex<float> FilterFir / M = 1 decimators run on the headline
// kernel (decim_stream_cf32<0, R, ..., 1>, any N <= kCfMaxTaps), which takes
// every complex<float> shape this kernel could.
// Each lane owns R = 8 consecutive outputs; taps are walked in chunks of 4
// with a 12-sample register window held as three 4-sample blocks A|B|C (tap
// chunk q of output r reads sample r - 4q - p, p < 4).  After a chunk C drops,
// B -> C, A -> B and A is refilled from LDS, so three chunks are unrolled with
// rotating block roles and the window slides without register moves.  Each
// output is ONE sequential fma (or mul+add) chain in ascending tap order, as
// the reference's loop over n (filters.h:150-161).
// LDS: the tile span (tile outputs + P0 halo samples, P0 = 8*ceil((N-1)/8))
// as 16-B granules with one pad granule after every lane chunk (8 samples),
// so lanes' ds_read_b128 land on distinct bank slots (odd granule stride).
constexpr int kFirMaxTaps = 1024;
constexpr int kFirR = 8, kFirBlock = 256;

template <int KV>
struct FirTraits;
template <>
struct FirTraits<KV_F32_REAL> {
    typedef float S;
    static constexpr int SPG = 4;  // samples per 16-B granule
};

__device__ __forceinline__ float fir_mac(bool fma, float c, float x, float y) {
    return fma ? __builtin_fmaf(c, x, y) : y + c * x;
}

// The FIR arithmetic of one lane: R outputs from the staged LDS image `fl`
// (lane base granule gb), N taps (runtime) through the constant view tp.
template <int KV, bool FMA>
__device__ __forceinline__ void fir_lane(const float4 *fl, int gb, int N, ConstPtr<float> tp, unsigned sh,
                                         float2 (&o)[kFirR]) {
    typedef typename FirTraits<KV>::S S;
    constexpr int SPG = FirTraits<KV>::SPG;
    constexpr int R = kFirR, GPL = R / SPG;
    const int NQ = (N + 3) / 4;
    auto slot = [&](int g) { return g + g / GPL; };
    float yr[R];
    f2_t y2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        yr[r] = 0.f;
        y2[r] = (f2_t){0.f, 0.f};
    }
    S A[4], B[4], C[4];
    // window reads through a volatile LDS view: every one a whole
    // ds_read_b128 (conflict-free at the odd granule stride).  Plain reads
    // were narrowed to the words used -- ds_read_b64 / b96 / read2_b32, whose
    // lane groups the padded layout does not spread (54.7 M conflict cycles
    // per launch at 31 taps, float in).
    typedef float f4v_t __attribute__((ext_vector_type(4)));
    auto rd = [&](int g) {
        const f4v_t w = *(const volatile __attribute__((address_space(3))) f4v_t *)(&fl[slot(g)]);
        return make_float4(w[0], w[1], w[2], w[3]);
    };
    auto fill = [&](S (&dst)[4], int m) {
        if constexpr (SPG == 4) {
            const float4 v = rd(gb + m / 4);
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        } else {
            const float4 v0 = rd(gb + m / 2), v1 = rd(gb + m / 2 + 1);
            dst[0] = make_float2(v0.x, v0.y); dst[1] = make_float2(v0.z, v0.w);
            dst[2] = make_float2(v1.x, v1.y); dst[3] = make_float2(v1.z, v1.w);
        }
    };
    // chunk q: window blocks (lo = samples -4q-4.., mid = -4q.., hi = -4q+4..)
    auto chunk = [&](int q, const S (&lo)[4], const S (&mid)[4], const S (&hi)[4], bool guard) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int k = 4 * q + p;
            if (guard && k >= N) break;
            const float c = tp[k];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int rel = r - p + 4;  // 0..11 over lo|mid|hi
                const S x = rel < 4 ? lo[rel] : (rel < 8 ? mid[rel - 4] : hi[rel - 8]);
                if constexpr (SPG == 4) {
                    yr[r] = fir_mac(FMA, c, x, yr[r]);
                } else {  // (re, im) as one packed pair: v_pk_fma_f32 / v_pk_mul + v_pk_add
                    const f2_t xv = {x.x, x.y}, cv = {c, c};
                    if constexpr (FMA) y2[r] = __builtin_elementwise_fma(cv, xv, y2[r]);
                    else y2[r] = y2[r] + cv * xv;
                }
            }
        }
    };
    fill(C, 4);
    fill(B, 0);
    int q = 0;
    for (; q + 3 <= NQ; q += 3) {
        asm volatile("" : "+s"(tp));
        fill(A, -4 * q - 4);
        chunk(q, A, B, C, false);          // A|B|C
        fill(C, -4 * q - 8);
        chunk(q + 1, C, A, B, false);      // C|A|B
        fill(B, -4 * q - 12);
        chunk(q + 2, B, C, A, q + 3 == NQ);  // B|C|A (guard the last chunk)
    }
    if (q < NQ) {
        fill(A, -4 * q - 4);
        chunk(q, A, B, C, true);
        if (q + 1 < NQ) {
            fill(C, -4 * q - 8);
            chunk(q + 1, C, A, B, true);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        o[r] = SPG == 4 ? make_float2(q16f(yr[r], sh), 0.f) : make_float2(q16f(y2[r].x, sh), q16f(y2[r].y, sh));
}

__host__ __device__ constexpr int fir_halo(int ntaps) { return 8 * (((ntaps + 3) / 4 + 1) / 2); }

// one tile per workgroup, any tap count up to kFirMaxTaps (dynamic LDS)
template <int KV, bool FMA>
__global__ __launch_bounds__(kFirBlock) void fir_tile_f32(DecimLaunch a) {
    typedef typename FirTraits<KV>::S S;
    constexpr int SPG = FirTraits<KV>::SPG;
    constexpr int R = kFirR, BLOCK = kFirBlock, TO = R * BLOCK;
    constexpr int GPL = R / SPG;  // granules per lane chunk
    extern __shared__ float4 fl[];
    const int N = a.ntaps, H = N - 1;
    const int P0 = fir_halo(N);  // >= 4*NQ: the last chunk's window block
    const int ch = blockIdx.y;
    const S *in = (const S *)a.in + ch * a.in_stride;
    const S *hist = (const S *)a.hist_in[ch];
    float2 *out = (float2 *)a.out + ch * a.out_stride;
    const long n_in = a.n_in;
    const int t = threadIdx.x;
    if (blockIdx.x == 0) write_history(in, n_in, hist, (S *)a.hist_out[ch], H);
    const long o0 = (long)blockIdx.x * TO;  // first output (= input sample) of the tile
    const int span = TO + P0;                // staged samples, origin o0 - P0
    auto slot = [&](int g) { return g + g / GPL; };
    // stage through the cache: the tile's own TO samples with every load of a
    // lane in flight before the LDS writes (every tile but the launch's last
    // lies inside the input), then the halo (from history on tile 0) and any
    // partial tile granule-wise
    const int GH = P0 / SPG;
    constexpr int GPB = TO / SPG / BLOCK;  // body granules per lane
    const bool body_in = o0 + TO <= n_in;
    if (body_in) {
        float4 v[GPB];
#pragma unroll
        for (int i = 0; i < GPB; ++i) v[i] = *(const float4 *)(in + o0 + (long)(t + i * BLOCK) * SPG);
#pragma unroll
        for (int i = 0; i < GPB; ++i) fl[slot(GH + t + i * BLOCK)] = v[i];
    }
    for (int g = t; g < (body_in ? GH : span / SPG); g += BLOCK) {
        const long s0 = o0 - P0 + (long)g * SPG;
        float4 v;
        if (s0 >= 0 && s0 + SPG <= n_in) {
            v = *(const float4 *)(in + s0);
        } else {
            S w[SPG];
#pragma unroll
            for (int j = 0; j < SPG; ++j) w[j] = fetch(in, hist, s0 + j, n_in, H);
            v = *(const float4 *)w;
        }
        fl[slot(g)] = v;
    }
    __syncthreads();
    float2 o[R];
    fir_lane<KV, FMA>(fl, (P0 + R * t) / SPG, N, const_view<float>(a.coef), a.shift, o);
    const long n0 = o0 + (long)t * R;
    if (n0 + R <= a.n_out) {
#pragma unroll
        for (int r = 0; r < R; r += 2) *(float4 *)(out + n0 + r) = make_float4(o[r].x, o[r].y, o[r + 1].x, o[r + 1].y);
    } else {
        for (int r = 0; r < R; ++r)
            if (n0 + r < a.n_out) out[n0 + r] = o[r];
    }
}

// Persistent variant for <= kFirStreamTaps taps (the headline decimator's
// memory schedule): grid-stride tile order, the next tile's buffer loads
// (non-temporal, range-checked zero fill past the end) issued into VGPRs
// right after this tile lands in LDS, outputs transposed across the wave's
// lanes into whole-line non-temporal stores (OST below).
constexpr int kFirStreamTaps = 128;

// OST: 1 = outputs staged through LDS (two more barriers per tile); 2 = the
// wave's outputs transposed across lanes (store_wave_lines) into whole-line
// stores, no LDS round trip.
// NTC > 0: the tap count as a compile-time constant (the tap loop unrolls
// completely); 0: a.ntaps at run time.
template <int KV, bool FMA, int OST = 2, int NTC = 0>
__global__ __launch_bounds__(kFirBlock, 4) void fir_stream_f32(DecimLaunch a) {
    typedef typename FirTraits<KV>::S S;
    constexpr int SPG = FirTraits<KV>::SPG;
    constexpr int R = kFirR, BLOCK = kFirBlock, TO = R * BLOCK;
    constexpr int GPL = R / SPG;
    constexpr int P0MAX = fir_halo(kFirStreamTaps);
    constexpr int TGMAX = (TO + P0MAX) / SPG;  // staged granules, worst case
    constexpr int PER = ceildiv(TGMAX, BLOCK);
    constexpr int LSTAGE = TGMAX + TGMAX / GPL + 1;
    constexpr int LOUT = TO * 8 / 16;          // output tile as float4
    __shared__ float4 fl[LSTAGE > LOUT ? LSTAGE : LOUT];
    const int N = NTC > 0 ? NTC : a.ntaps, H = N - 1;
    const int P0 = fir_halo(N);
    const int TG = (TO + P0) / SPG;
    const int ch = blockIdx.y;
    const S *in = (const S *)a.in + ch * a.in_stride;
    const S *hist = (const S *)a.hist_in[ch];
    float2 *out = (float2 *)a.out + ch * a.out_stride;
    const long n_in = a.n_in;
    const int t = threadIdx.x;
    const long nb = gridDim.x;
    const long b = xcd_tile(blockIdx.x, nb);
    if (b == 0) write_history(in, n_in, hist, (S *)a.hist_out[ch], H);
    auto slot = [&](int g) { return g + g / GPL; };
    float4 v[PER];
    auto stage_load = [&](long tile) {  // tile >= 1 (its halo is input, not history)
        const long s0 = tile * TO - P0;
        const long remb = (n_in - s0) * (long)sizeof(S);
        const unsigned nrec = (unsigned)(remb > 0xfffffff0L ? 0xfffffff0L : (remb < 0 ? 0 : remb));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(in + s0), 0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if (g < TG) {
                // lane offset in the VGPR, per-load step in soffset; aux 2 = nt
                auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * t, 16 * i * BLOCK, 2);
                v[i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]),
                                   __uint_as_float(w[3]));
            }
        }
    };
    if (b < a.ntiles) {
        if (b == 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = t + i * BLOCK;
                if (g < TG) {
                    const long s0 = -P0 + (long)g * SPG;
                    S w[SPG];
#pragma unroll
                    for (int j = 0; j < SPG; ++j) w[j] = fetch(in, hist, s0 + j, n_in, H);
                    v[i] = *(const float4 *)w;
                }
            }
        } else {
            stage_load(b);
        }
    }
    ConstPtr<float> tp = const_view<float>(a.coef);
    // the staged tile lands in LDS once every wave is done with the previous
    // tile's image and output staging
    auto stage_to_lds = [&]() {
        SRCDSP_LDS_BARRIER();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if (g < TG) fl[slot(g)] = v[i];
        }
        SRCDSP_LDS_BARRIER();
    };
    // as decim_stream_cf32: the next tile's loads are issued before this
    // tile's taps and land after its stores, in one iteration, so the wait
    // for them leaves the stores in flight
    auto do_tile = [&](long tile, auto whole_tag) {
        constexpr bool WHOLE = decltype(whole_tag)::value;
        float2 o[R];
        fir_lane<KV, FMA>(fl, (P0 + R * t) / SPG, N, tp, a.shift, o);
        const long o0 = tile * TO;
        if constexpr (OST == 2) {
            if constexpr (WHOLE) {
                store_wave_lines<R, true>(out + o0 + (t & ~63) * R, o, t & 63);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (o0 + t * R + r < a.n_out) out[o0 + t * R + r] = o[r];
            }
            return;
        }
        SRCDSP_LDS_BARRIER();  // every wave is done reading the staged input
        float2 *ob = (float2 *)fl;
#pragma unroll
        for (int r = 0; r < R; ++r) ob[t * R + r] = o[r];
        SRCDSP_LDS_BARRIER();
        if constexpr (WHOLE) {
#pragma unroll
            for (int i = 0; i < LOUT / BLOCK; ++i) {
                const int k = t + i * BLOCK;
                store16<true>((float4 *)(out + o0) + k, fl[k]);
            }
        } else {
            for (int k = t; k < TO; k += BLOCK)
                if (o0 + k < a.n_out) out[o0 + k] = ob[k];
        }
    };
    // prefetching loop, the workgroup's last tile peeled (as decim_stream_cf32)
    if (b < a.ntiles) {
        stage_to_lds();
        long tile = b;
        for (; tile + nb < a.ntiles; tile += nb) {
            stage_load(tile + nb);
            do_tile(tile, std::true_type{});
            stage_to_lds();
        }
        if ((tile + 1) * TO <= a.n_out)
            do_tile(tile, std::true_type{});
        else
            do_tile(tile, std::false_type{});
    }
}

}  // namespace srcdsp
