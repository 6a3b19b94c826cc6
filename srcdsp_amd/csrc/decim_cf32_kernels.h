// decim_cf32_kernels.h -- the complex<float> headline kernel
// (decim_stream_cf32) and its tap helpers, instantiated by decim_cf32_ct.hip
// and decim_cf32_rt.hip through cf32_launch.h.  See decim.hip for the
// semantics.
#pragma once
#include "fir_device.h"

namespace srcdsp {

// One packed fma step of a complex<float> accumulator by a real tap that sits
// in one half of an SGPR pair: acc = fma(c, x, acc) per component.  Inline asm
// so the tap loop issues in the order written (every accumulator's chain
// advances one tap before any advances the next): the scheduler otherwise
// groups up to ten dependent v_pk_fma_f32 of one chain back to back, each
// waiting for the previous one's result.  HI: the tap is the pair's odd
// element.  ZERO: acc starts from +0 (fma(c, x, +0), as the first step of
// the reference's accumulation from 0).
template <bool HI, bool ZERO>
__device__ __forceinline__ void pk_fma_tap(f2_t &acc, unsigned long long cp, f2_t x) {
    if constexpr (ZERO && HI)
        asm volatile("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(acc) : "s"(cp), "v"(x));
    else if constexpr (ZERO)
        asm volatile("v_pk_fma_f32 %0, %1, %2, 0 op_sel_hi:[0,1,0]" : "=v"(acc) : "s"(cp), "v"(x));
    else if constexpr (HI)
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "s"(cp), "v"(x));
    else
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(cp), "v"(x));
}

// The strict contract's step acc = acc + c*x (separately rounded product,
// then sum, as the reference's -O2 x86-64 build computes it), split so a
// tap's R products can issue before its R sums: pk_mul_tap writes the
// product, pk_add_acc adds it.
template <bool HI>
__device__ __forceinline__ void pk_mul_tap(f2_t &p, unsigned long long cp, f2_t x) {
    if constexpr (HI)
        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(p) : "s"(cp), "v"(x));
    else
        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(p) : "s"(cp), "v"(x));
}
__device__ __forceinline__ void pk_add_acc(f2_t &acc, f2_t p) {
    asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(p));
}

// One tap over R accumulators, skipped (by a branch inside the asm, so the
// compiler sees straight-line code) unless k < n as unsigned, i.e. 0 <= k < n.
// Used by the runtime-tap kernel's last chunk only.  The asm names its
// operands a0.., x0.., t0.., so every (R, HI, FMA) is a specialization of its
// own, generated below: SRCDSP_REP_R(F, S) is F(0, S) .. F(R-1, S) (asm lines),
// SRCDSP_LIST_R(F) the same comma-separated (operands).
template <int R, bool HI, bool FMA>
struct TapGuarded;

#define SRCDSP_REP_1(F, S) F(0, S)
#define SRCDSP_REP_2(F, S) SRCDSP_REP_1(F, S) F(1, S)
#define SRCDSP_REP_4(F, S) SRCDSP_REP_2(F, S) F(2, S) F(3, S)
#define SRCDSP_REP_8(F, S) SRCDSP_REP_4(F, S) F(4, S) F(5, S) F(6, S) F(7, S)
#define SRCDSP_LIST_1(F) F(0)
#define SRCDSP_LIST_2(F) SRCDSP_LIST_1(F), F(1)
#define SRCDSP_LIST_4(F) SRCDSP_LIST_2(F), F(2), F(3)
#define SRCDSP_LIST_8(F) SRCDSP_LIST_4(F), F(4), F(5), F(6), F(7)
#define SRCDSP_TG_FMA(i, S) "v_pk_fma_f32 %[a" #i "], %[c], %[x" #i "], %[a" #i "] " S "\n\t"
#define SRCDSP_TG_MUL(i, S) "v_pk_mul_f32 %[t" #i "], %[c], %[x" #i "] " S "\n\t"
#define SRCDSP_TG_ADD(i, S) "v_pk_add_f32 %[a" #i "], %[a" #i "], %[t" #i "]\n\t"
#define SRCDSP_TG_ACC(i) [a##i] "+v"(a[i])
#define SRCDSP_TG_TMP(i) [t##i] "=&v"(t[i])
#define SRCDSP_TG_X(i) [x##i] "v"(x[i])
#define SRCDSP_TG_IN(R) [k] "s"(k), [n] "s"(n), [c] "s"(c), SRCDSP_LIST_##R(SRCDSP_TG_X)
#define SRCDSP_TG_SKIP "s_cmp_lt_u32 %[k], %[n]\n\ts_cbranch_scc0 1f\n\t"
// the FMA and the mul+add specialization of one (R, HI); SEL3 / SEL2: the
// operand selects that pick the tap's half of the pair (three / two operands)
#define SRCDSP_TAP_GUARDED(R, HI, SEL3, SEL2)                                                                       \
    template <>                                                                                                     \
    struct TapGuarded<R, HI, true> {                                                                                \
        static __device__ __forceinline__ void run(f2_t (&a)[R], unsigned long long c, const f2_t (&x)[R], int k,   \
                                                   int n) {                                                         \
            asm volatile(SRCDSP_TG_SKIP SRCDSP_REP_##R(SRCDSP_TG_FMA, SEL3) "1:"                                    \
                         : SRCDSP_LIST_##R(SRCDSP_TG_ACC)                                                           \
                         : SRCDSP_TG_IN(R)                                                                          \
                         : "scc");                                                                                  \
        }                                                                                                           \
    };                                                                                                              \
    template <>                                                                                                     \
    struct TapGuarded<R, HI, false> {                                                                               \
        static __device__ __forceinline__ void run(f2_t (&a)[R], unsigned long long c, const f2_t (&x)[R], int k,   \
                                                   int n) {                                                         \
            f2_t t[R];                                                                                              \
            asm volatile(SRCDSP_TG_SKIP SRCDSP_REP_##R(SRCDSP_TG_MUL, SEL2) SRCDSP_REP_##R(SRCDSP_TG_ADD, "") "1:"  \
                         : SRCDSP_LIST_##R(SRCDSP_TG_ACC), SRCDSP_LIST_##R(SRCDSP_TG_TMP)                           \
                         : SRCDSP_TG_IN(R)                                                                          \
                         : "scc");                                                                                  \
        }                                                                                                           \
    };
#define SRCDSP_TAP_GUARDED_R(R)                                         \
    SRCDSP_TAP_GUARDED(R, false, "op_sel_hi:[0,1,1]", "op_sel_hi:[0,1]") \
    SRCDSP_TAP_GUARDED(R, true, "op_sel:[1,0,0] op_sel_hi:[1,1,1]", "op_sel:[1,0] op_sel_hi:[1,1]")
SRCDSP_TAP_GUARDED_R(1)
SRCDSP_TAP_GUARDED_R(2)
SRCDSP_TAP_GUARDED_R(4)
SRCDSP_TAP_GUARDED_R(8)

// Persistent complex<float> decimator: the headline (a1, M = 4, R = 4) and the
// same schedule at M = 16 / 8 / 3 / 2 / 1 with R = 1 / 2 / 4 / 4 / 8 outputs
// per lane (lane chunks of M R = 16 / 16 / 12 / 8 / 8 input samples; M = 1 is
// the complex<float> FilterFir).
//
// Tiles.  A tile is BLOCK*R outputs; its input span (M*BLOCK*R samples + a
// 4*NQ sample halo, NQ = ceil(N/4)) is staged HBM -> VGPR -> LDS as 16-B
// granules (2 samples).  LDS granule of tile granule g:
//   L(g) = g + (g - 2NQ + KPAD*PR) / PR,  PR = M*R/2 granules per lane chunk,
// i.e. one pad granule in front of every lane chunk, so lane t's chunk starts
// at B_t = 2NQ + KPAD + (PR+1) t and the 16 lanes of a ds_read_b128 group hit
// 16 distinct 16-B bank slots.
// Memory schedule.  Persistent grid, tiles in grid-stride order (the chip
// sweeps one contiguous window of the input at a time); the NEXT tile's
// loads (buffer_load_dwordx4, non-temporal, one descriptor per tile: the
// range check zero-fills past the end) are issued into VGPRs before this
// tile's taps and land in LDS after its stores, in one loop iteration, so
// the wait for them leaves the stores in flight.
// Taps.  Each lane owns R consecutive outputs and walks the taps as 4
// polyphase register windows sliding one sample per 4 taps; taps are
// wave-uniform SGPR pairs issued tap-major through inline asm (pk_fma_tap:
// every accumulator chain advances one tap before any advances the next).
// FMA: one v_pk_fma_f32 per tap and output (bit-exact to the -mfma build);
// strict: R v_pk_mul_f32, then R v_pk_add_f32 (bit-exact to the -O2 build).
// Tap count.  NT > 0: compiled in (the tap loop unrolls completely).  NT = 0:
// a.ntaps at run time (<= kCfMaxTaps), the tap loop in chunks of S 4-tap
// steps whose window groups rotate through S register slots (2S a multiple
// of PR, so a chunk's LDS reads are one base plus immediates), the chunk's
// taps loaded one chunk ahead, taps past N skipped (never multiplied by 0:
// 0 * inf would differ); the LDS image is dynamic, sized by the host.
// Outputs.  Quantised (Q0: the shift-0 quantiser) and paired across lanes
// by v_permlane32_swap / v_permlane16_swap (store_wave_lines) so every store
// instruction writes 1 KiB of whole lines, non-temporal.
// runtime-tap kernel geometry: the window's register slots (the EH + 3 live
// groups, EH = M(R-1)/4) and the 4-tap steps per chunk (the smallest multiple
// of the slots that makes 2 U a multiple of the PR granules of a lane chunk,
// so a chunk's LDS reads are one base plus immediates), and the front slack of
// its LDS image (granules below the halo that the tail chunk's unconditional
// window reads may touch)
__host__ __device__ constexpr int cf32_rt_slots(int M, int R) { return (M * (R - 1)) / 4 + 3; }
__host__ __device__ constexpr int cf32_rt_steps(int M, int R) {
    int u = cf32_rt_slots(M, R);
    while ((2 * u) % (M * R / 2) != 0) u += cf32_rt_slots(M, R);
    return u;
}
__host__ __device__ constexpr int cf32_rt_front(int M, int R) {
    return 2 * cf32_rt_steps(M, R) + ceildiv(2 * cf32_rt_steps(M, R), M * R / 2) + 2;
}
// dynamic LDS granules of the runtime-tap kernel (decim_stream_cf32<0, ...>)
__host__ __device__ constexpr int cf32_lds_granules(int M, int R, int BLOCK, int ntaps) {
    return cf32_rt_front(M, R) + (M * BLOCK * R / 2 + 2 * ((ntaps + 3) / 4)) +
           ((M * BLOCK * R / 2 + 2 * ((ntaps + 3) / 4)) + ceildiv(2 * ((ntaps + 3) / 4), M * R / 2) * (M * R / 2)) /
               (M * R / 2) +
           1;
}

template <int NT, int R, int BLOCK, bool FMA, int MINW, bool Q0, int M>
__global__ __launch_bounds__(BLOCK, MINW) void decim_stream_cf32(DecimLaunch a) {
    static_assert((M * R) % 4 == 0 && M * R <= 16, "a lane chunk is 4, 8, 12 or 16 input samples");
    static_assert(R == 1 || R == 2 || R == 4 || R == 8, "whole-line stores assume 1, 2, 4 or 8 outputs per lane");
    constexpr bool RT = NT == 0;
    // the compiled-in tap loop unrolls completely over a window of 4 (NQ + M R / 4)
    // samples; at M = 4 beyond 128 taps and at M = 1 beyond 64 it no longer stays
    // in registers (1-2 KiB of scratch per lane), so those lengths take NT = 0
    static_assert(RT || (M == 1 ? NT <= 64 : (M > 4 || NT <= 128)),
                  "compile the tap count in only where the unrolled window stays in registers");
    constexpr int NQC = RT ? (kCfMaxTaps + 3) / 4 : (NT + 3) / 4;  // the register prefetch is sized for this halo
    constexpr int TO = BLOCK * R;
    constexpr int PR = M * R / 2;  // granules per lane chunk (M R samples)
    constexpr int PER = ceildiv(M * TO / 2 + 2 * NQC, BLOCK);
    const int N = RT ? a.ntaps : NT;
    const int NQ = RT ? (N + 3) / 4 : NQC;
    const int TG = M * TO / 2 + 2 * NQ;  // staged granules: M TO input samples + the halo
    const int KPAD = ceildiv(2 * NQ, PR);
    float4 *lds;
    if constexpr (RT) {
        extern __shared__ float4 lds_dyn[];
        lds = lds_dyn + cf32_rt_front(M, R);
    } else {
        constexpr int TGC = M * TO / 2 + 2 * NQC, KPC = ceildiv(2 * NQC, PR);
        __shared__ float4 lds_st[TGC + (TGC + KPC * PR) / PR + 1];
        lds = lds_st;
    }

    const int ch = blockIdx.y;
    const float2 *in = (const float2 *)a.in + ch * a.in_stride;
    const float2 *hist = (const float2 *)a.hist_in[ch];
    float2 *out = (float2 *)a.out + ch * a.out_stride;
    const long n_in = a.n_in;
    const int H = N - 1;
    const int t = threadIdx.x;
    const long nb = gridDim.x;
    const long b = xcd_tile(blockIdx.x, nb);
    // grid-stride tile order: tiles b, b + nb, b + 2 nb, ...
    if (b == 0 && a.ntiles > 0) write_history(in, n_in, hist, (float2 *)a.hist_out[ch], H);

    float4 v[PER];
    // tiles >= 1: one descriptor per tile, 32-bit lane offsets, range-checked
    auto stage_load = [&](float4 (&v)[PER], long tile) {
        const long b0 = M * tile * TO - 4 * NQ;  // >= 0 for tile >= 1
        const long remb = (n_in - b0) * 8;
        const unsigned nrec = (unsigned)(remb > 0xfffffff0L ? 0xfffffff0L : (remb < 0 ? 0 : remb));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(in + b0), 0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if ((i + 1) * BLOCK <= M * TO / 2 || g < TG) {  // the tile body always exists; the halo tail may not
                // lane offset in the VGPR, the per-load step in soffset (an
                // SGPR constant): one offset VGPR for all PER loads; aux 2 = nt
                auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * t, 16 * i * BLOCK, 2);
                v[i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]),
                                   __uint_as_float(w[3]));
            }
        }
    };
    if (b < a.ntiles) {
        if (b == 0) {  // tile 0: the halo comes from the history
            const long b0 = -4 * NQ;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = t + i * BLOCK;
                const long s = b0 + 2 * (long)g;
                if (g < TG) {
                    float2 lo = fetch(in, hist, s, n_in, H), hi = fetch(in, hist, s + 1, n_in, H);
                    v[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
                }
            }
        } else {
            stage_load(v, b);
        }
    }
    const int Bt = 2 * NQ + KPAD + (PR + 1) * t;
    // the staged tile lands in LDS once every wave is done with the previous
    // tile's image
    // LDS granule of staged granule g = t + i BLOCK: g + (g - 2NQ + KPAD PR) / PR,
    // the quotient's lane part computed once (BLOCK a multiple of PR)
    const int lq = (t - 2 * NQ + KPAD * PR) / PR;  // >= 0
    auto stage_to_lds = [&]() {
        SRCDSP_LDS_BARRIER();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if ((i + 1) * BLOCK <= M * TO / 2 || g < TG) {
                if constexpr (BLOCK % PR == 0)
                    lds[g + lq + i * (BLOCK / PR)] = v[i];
                else
                    lds[g + (g - 2 * NQ + KPAD * PR) / PR] = v[i];
            }
        }
        SRCDSP_LDS_BARRIER();
    };
    // one tap step (4 taps k = 4q..4q+3) over the R accumulators; xs(r, p) is
    // sample M r - 4q - p of the lane frame; cp2(j) the tap pair j of the step
    auto tap_step = [&](f2_t (&acc)[R], int k0, auto first_tag, auto guard_tag, auto &&xs, auto &&cp2, int kn) {
        constexpr bool FIRST = decltype(first_tag)::value;  // k0 == 0: accumulators start from +0
        constexpr bool GUARD = decltype(guard_tag)::value;  // taps k0 + p >= kn skipped
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (GUARD && k0 + p >= kn) break;
            const unsigned long long cp = cp2(p >> 1);
            if constexpr (FMA) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float2 x = xs(r, p);
                    const f2_t xv = {x.x, x.y};
                    if (FIRST && p == 0) pk_fma_tap<false, true>(acc[r], cp, xv);
                    else if (p & 1) pk_fma_tap<true, false>(acc[r], cp, xv);
                    else pk_fma_tap<false, false>(acc[r], cp, xv);
                }
            } else {
                f2_t pr[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float2 x = xs(r, p);
                    const f2_t xv = {x.x, x.y};
                    if (p & 1) pk_mul_tap<true>(pr[r], cp, xv);
                    else pk_mul_tap<false>(pr[r], cp, xv);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) pk_add_acc(acc[r], pr[r]);
            }
        }
    };
    // one tile: taps over the LDS image, outputs stored
    // WHOLE: the tile's TO outputs all exist (every tile but a partial last one)
    auto do_tile = [&](long tile, auto whole_tag) {
        constexpr bool WHOLE = decltype(whole_tag)::value;
        ConstPtr<unsigned long long> tp2 = const_view<unsigned long long>(a.coef);
        asm volatile("" : "+s"(tp2));
        f2_t acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = f2_t{0.f, 0.f};
        auto rd = [&](int idx) { return lds[idx]; };
        if constexpr (!RT) {
            constexpr int GPC = M * R / 4;  // 4-sample groups per lane chunk
            float2 X[4 * (NQC + GPC)];
            auto load_group = [&](int e) {
                const float4 g0 = rd(Bt + 2 * e + floordiv(2 * e, PR));
                const float4 g1 = rd(Bt + 2 * e + 1 + floordiv(2 * e + 1, PR));
                X[4 * e + 4 * NQC + 0] = make_float2(g0.x, g0.y);
                X[4 * e + 4 * NQC + 1] = make_float2(g0.z, g0.w);
                X[4 * e + 4 * NQC + 2] = make_float2(g1.x, g1.y);
                X[4 * e + 4 * NQC + 3] = make_float2(g1.z, g1.w);
            };
#pragma unroll
            for (int e = -1; e < GPC; ++e) load_group(e);
#pragma unroll
            for (int q = 0; q < NQC; ++q) {
                if (q + 1 < NQC) load_group(-q - 2);
                if ((q & 3) == 0) asm volatile("" : "+s"(tp2));
                auto xs = [&](int r, int p) { return X[M * r - 4 * q - p + 4 * NQC]; };
                auto cp2 = [&](int j) { return tp2[2 * q + j]; };
                if (q == 0)
                    tap_step(acc, 4 * q, std::true_type{}, std::integral_constant<bool, (4 * NQC > NT)>{}, xs, cp2, NT);
                else if (q == NQC - 1)
                    tap_step(acc, 4 * q, std::false_type{}, std::integral_constant<bool, (4 * NQC > NT)>{}, xs, cp2, NT);
                else
                    tap_step(acc, 4 * q, std::false_type{}, std::false_type{}, xs, cp2, NT);
            }
        } else {
            // window groups e (samples 4e..4e+3 of the lane frame) in S rotating
            // register slots; a step q reads groups -q-1 .. EH-q and prefetches
            // -q-2; chunks of U steps (q0 a multiple of U)
            constexpr int EH = (M * (R - 1)) / 4;
            constexpr int S = cf32_rt_slots(M, R), U = cf32_rt_steps(M, R);
            static_assert(S == EH + 3 && U % S == 0 && (2 * U) % PR == 0, "window slots / chunk steps");
            float2 X[S][4];
            auto slot = [](int e) { return ((e % S) + S) % S; };
            // chunk base: LDS granule of group c - q0 is cb + 2c + floordiv(2c, PR)
            auto load_group = [&](int cb, int c) {
                const float4 g0 = rd(cb + 2 * c + floordiv(2 * c, PR));
                const float4 g1 = rd(cb + 2 * c + 1 + floordiv(2 * c + 1, PR));
                float2(&d)[4] = X[slot(c)];
                d[0] = make_float2(g0.x, g0.y);
                d[1] = make_float2(g0.z, g0.w);
                d[2] = make_float2(g1.x, g1.y);
                d[3] = make_float2(g1.z, g1.w);
            };
#pragma unroll
            for (int e = -1; e <= EH; ++e) load_group(Bt, e);
            // the chunk body: U steps from q0 (a multiple of U).  TAIL: the
            // last chunk, every tap through TapGuarded (k < N, a branch inside
            // the asm: the compiler sees the same straight line as a full
            // chunk); its window reads are unconditional (the image has front
            // slack for the reads past the halo)
            auto chunk = [&](int q0, auto tail_tag, auto jb_tag, auto je_tag) {
                constexpr bool TAIL = decltype(tail_tag)::value;
                constexpr int JB = decltype(jb_tag)::value, JE = decltype(je_tag)::value;  // steps [JB, JE)
                const int cb = Bt - 2 * q0 - 2 * q0 / PR;
                ConstPtr<unsigned long long> tc = tp2 + 2 * q0;
                asm volatile("" : "+s"(tc));
                const int kb = 4 * q0;
#pragma unroll
                for (int j = JB; j < JE; ++j) {
                    if (j > JB && (j & 3) == 0) asm volatile("" : "+s"(tc));  // taps in batches of 16 (one s_load_dwordx16)
                    load_group(cb, -j - 2);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const unsigned long long cp = tc[2 * j + (p >> 1)];
                        f2_t xv[R];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const int s = M * r - 4 * j - p;  // sample of the frame, relative to -4 q0
                            const int e = floordiv(s, 4);
                            const float2 x = X[slot(e)][s - 4 * e];
                            xv[r] = f2_t{x.x, x.y};
                        }
                        if constexpr (TAIL) {
                            if (p & 1) TapGuarded<R, true, FMA>::run(acc, cp, xv, kb + 4 * j + p, N);
                            else TapGuarded<R, false, FMA>::run(acc, cp, xv, kb + 4 * j + p, N);
                        } else if constexpr (FMA) {
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                if (p & 1) pk_fma_tap<true, false>(acc[r], cp, xv[r]);
                                else pk_fma_tap<false, false>(acc[r], cp, xv[r]);
                            }
                        } else {
                            f2_t pr[R];
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                if (p & 1) pk_mul_tap<true>(pr[r], cp, xv[r]);
                                else pk_mul_tap<false>(pr[r], cp, xv[r]);
                            }
#pragma unroll
                            for (int r = 0; r < R; ++r) pk_add_acc(acc[r], pr[r]);
                        }
                    }
                    // one step at a time: the next step's group is already in
                    // flight; hoisting more reads only lengthens the live window
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            // full chunks while all their taps exist, then the last chunk,
            // guarded, in two halves: the second only when steps remain there
            // (the guarded steps' reads and branches are the runtime kernel's
            // overhead over a compiled tap count)
            using I0 = std::integral_constant<int, 0>;
            using IH = std::integral_constant<int, U / 2>;
            using IU = std::integral_constant<int, U>;
            int q0 = 0;
            for (; 4 * (q0 + U) <= N; q0 += U) chunk(q0, std::false_type{}, I0{}, IU{});
            if (q0 < NQ) {
                chunk(q0, std::true_type{}, I0{}, IH{});
                if (q0 + U / 2 < NQ) chunk(q0, std::true_type{}, IH{}, IU{});
            }
        }
        const long n0 = tile * TO + (long)t * R;
        const unsigned sh = a.shift;
        auto q = [&](float y) { return Q0 ? q16f_shift0(y) : q16f(y, sh); };
        if constexpr (WHOLE && R == 2) {  // 16 B per lane: whole lines as they stand
            store16<true>((float4 *)(out + n0), make_float4(q(acc[0].x), q(acc[0].y), q(acc[1].x), q(acc[1].y)));
        } else if constexpr (WHOLE && R == 1) {  // 8 B per lane, lane-contiguous
            out[n0] = make_float2(q(acc[0].x), q(acc[0].y));
        } else if constexpr (WHOLE) {
            float2 o[R];
#pragma unroll
            for (int r = 0; r < R; ++r) o[r] = make_float2(q(acc[r].x), q(acc[r].y));
            store_wave_lines<R, true>(out + tile * TO + (t & ~63) * R, o, t & 63);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (n0 + r < a.n_out) out[n0 + r] = make_float2(q(acc[r].x), q(acc[r].y));
        }
    };
    // Every iteration of the loop prefetches (the workgroup's last tile is
    // peeled off after it), and only the launch's last tile can be partial, so
    // the loop body is one straight path with a fixed number of stores: the
    // compiler waits for the prefetch with a counted vmcnt and the stores stay
    // in flight across iterations.
    if (b < a.ntiles) {
        stage_to_lds();
        long tile = b;
        for (; tile + nb < a.ntiles; tile += nb) {
            stage_load(v, tile + nb);
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
