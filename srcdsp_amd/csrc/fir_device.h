// fir_device.h -- device helpers shared by the FIR-core kernel families
// (decim_cf32_kernels.h, decim_ci16_kernels.h, decim_tile_kernels.h,
// fir_f32_kernels.h), the DDC bank (ddc_bank_kernels.h), the correlator and
// the tuning harness under scripts/tune: tap arithmetic and quantisers,
// history, whole-line stores, and the v_dot2 helpers and geometry of the
// complex<int16_t> plane kernels.
#pragma once
#include "ops.h"

namespace srcdsp {
typedef short short2_t_ __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------ arithmetic
template <bool FMA>
__device__ __forceinline__ float mac(float c, float x, float y) {
    if constexpr (FMA) return __builtin_fmaf(c, x, y);
    else return y + x * c;  // -ffp-contract=off: rounded product, then rounded sum
}

__device__ __forceinline__ float q16f(float y, unsigned shift) {
    return (float)limit16(cvt_f2i_x86(y), shift);
}

// read one input sample of channel data / history; idx may be negative (history)
template <typename T>
__device__ __forceinline__ T fetch(const T *in, const T *hist, long idx, long n_in, int H) {
    if (idx >= 0) return idx < n_in ? in[idx] : T{};
    long h = idx + H;
    return h >= 0 ? hist[h] : T{};
}

// ---------------------------------------------------------------- history
// hist_out[k] = (hist_in ++ in)[H + n_in - H + k], k < H
template <typename T>
__device__ void write_history(const T *in, long n_in, const T *hist_in, T *hist_out, int H) {
    for (int k = threadIdx.x; k < H; k += blockDim.x) {
        long idx = n_in - H + k;
        hist_out[k] = idx >= 0 ? in[idx] : hist_in[H + idx];
    }
}

// limitScale16 of a float accumulator when (coeffScaling - leftShift) & 31 == 0:
// trunc, clamp to +-32767, and 0 for |y| >= 2^31 or NaN (x86 cvttss2si gives
// INT_MIN there, which limitScale16 passes through and int16 truncates to 0).
// 4 VALU ops instead of the integer path's ~8; identical results.
__device__ __forceinline__ float q16f_shift0(float y) {
    // "+ 0.0f" turns the -0.0 that trunc gives for y in (-1, 0) into +0.0, as the
    // integer round trip of the reference does
    const float t = __builtin_fminf(__builtin_fmaxf(__builtin_truncf(y), -32767.0f), 32767.0f) + 0.0f;
    return __builtin_fabsf(y) < 2147483648.0f ? t : 0.0f;
}

// NCO mixer of mixers.h:169-188 on one packed sample
__device__ __forceinline__ uint32_t mix_sample(uint32_t w, const int16_t *tab, unsigned N, unsigned phi) {
    unsigned ic = phi + N / 4;  // (phi + N/4) % N with phi < N
    ic = ic >= N ? ic - N : ic;
    int32_t lr = tab[ic], li = tab[phi];
    int32_t ar = sext16(w), ai = sext16_hi(w);
    int32_t r = ar * lr - ai * li;   // |.| < 2^31: |T| <= 16383
    int32_t i = ai * lr + li * ar;
    return pack16(limit16(r, 14), limit16(i, 14));
}

// LDS hand-off between the waves of one workgroup without a memory fence:
// waits for this wave's LDS traffic only, so outstanding global loads (the
// next tile's prefetch) and output stores stay in flight across the barrier.
#define SRCDSP_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Phase clock of decim_dot2_ci16 (tuning builds only, -DSRCDSP_PHASE_CLOCK,
// scripts/tune/phase_clock.py): every wave sums the shader cycles (s_memtime)
// it spends in each phase of its tile loop, and lane 0 adds the sums to
// phase_clock[] (vector atomics) at exit:
//   0 prologue (table build, history, first staging load), 1 wait at the
//   barrier before staging, 2 staging (mix + LDS writes), 3 wait at the
//   barrier after staging (+ next tile's load issue), 4 tap loop + quantise,
//   5 stores, 6 waves, 7 tiles.
// The stamps wait for outstanding LDS reads (lgkmcnt), so they perturb the
// schedule a little; they are a diagnosis, not a timing.
#ifdef SRCDSP_PHASE_CLOCK
static __device__ unsigned long long phase_clock[8];
#define SRCDSP_PH(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define SRCDSP_PH_ADD(k, d) ph_acc[k] += (d)
#else
#define SRCDSP_PH(v)
#define SRCDSP_PH_ADD(k, d)
#endif

template <bool NTS>
__device__ __forceinline__ void store16(float4 *p, float4 v) {
    if constexpr (NTS) {
        typedef float f4_t __attribute__((ext_vector_type(4)));
        f4_t w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, (f4_t *)p);
    } else {
        *p = v;
    }
}
// Whole-line stores of one wave's outputs without an LDS round trip.  Lane l
// holds R = 4 or 8 consecutive float2 outputs (wave output l*R + r), i.e.
// R/2 16-B units; storing them as they stand would make every store
// instruction half- or quarter-cover its 128-B lines.  A transpose of units
// across 32-lane halves (v_permlane32_swap) and, for R = 8, 16-lane rows
// (v_permlane16_swap) leaves in register j the units of lanes
// [64j/(R/2), 64(j+1)/(R/2)): each store instruction then writes 1 KiB of
// whole lines.  wo = the wave's first output; ln = lane in wave.
template <int R, bool NTS>
__device__ __forceinline__ void store_wave_lines(float2 *wo, const float2 (&o)[R], int ln) {
    static_assert(R == 4 || R == 8, "4 or 8 outputs per lane");
    constexpr int U = R / 2;  // 16-B units per lane
    unsigned u[U][4];
#pragma unroll
    for (int k = 0; k < U; ++k) {
        u[k][0] = __float_as_uint(o[2 * k].x);
        u[k][1] = __float_as_uint(o[2 * k].y);
        u[k][2] = __float_as_uint(o[2 * k + 1].x);
        u[k][3] = __float_as_uint(o[2 * k + 1].y);
    }
    // vdst rows of the upper half <-> vsrc rows of the lower half
#pragma unroll
    for (int k = 0; k < U / 2; ++k)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            auto sw = __builtin_amdgcn_permlane32_swap(u[k][d], u[k + U / 2][d], false, false);
            u[k][d] = sw[0];
            u[k + U / 2][d] = sw[1];
        }
    if constexpr (U == 4) {  // odd 16-lane rows of vdst <-> even rows of vsrc
#pragma unroll
        for (int k = 0; k < U; k += 2)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                auto sw = __builtin_amdgcn_permlane16_swap(u[k][d], u[k + 1][d], false, false);
                u[k][d] = sw[0];
                u[k + 1][d] = sw[1];
            }
    }
    // register j, lane ln: unit (ln / (64/U)) of lane (64/U) j + ln % (64/U)
    constexpr int LPJ = 64 / U;
    float2 *base = wo + (ln % LPJ) * R + 2 * (ln / LPJ);
#pragma unroll
    for (int j = 0; j < U; ++j)
        store16<NTS>((float4 *)(base + LPJ * R * j), make_float4(__uint_as_float(u[j][0]), __uint_as_float(u[j][1]),
                                                                __uint_as_float(u[j][2]), __uint_as_float(u[j][3])));
}
__device__ __forceinline__ float4 nt_load4(const float4 *p) {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const f4_t w = __builtin_nontemporal_load((const f4_t *)p);
    return make_float4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------- v_dot2 planes (complex<int16_t>)
// Shared by decim_dot2_ci16 (decim_ci16_kernels.h) and ddc_bank_ci16.
// LDS: the planes are stored column-major.  Plane granule G (8 samples of one
// component, 16 B) of plane pl sits in slot  pl*2NC + (G&1)*NC + (G>>1)
// (NC = 4 mod 8).  A lane's window reads (granule 2t + HG + c, c compile-time)
// are then one per-lane base t plus an immediate offset -- no per-read
// address arithmetic -- and the 16 lanes of a ds_read_b128 group hit 16
// consecutive slots; the staging writes (staged granule g -> 8-B half g&1 of
// plane granule g>>1) put 16 consecutive lanes on 16 distinct 8-B bank slots
// because 2NC = 8 (mod 16).  No padding.  (The XOR-swizzled layout this
// replaces needed ~6 VALU ops per read: ~200 per wave tile.)
template <int NC>
__device__ __forceinline__ int dot2_slot(int G, int pl) {
    static_assert(NC % 8 == 4, "2 NC = 8 (mod 16): conflict-free staging writes");
    return pl * 2 * NC + (G & 1) * NC + (G >> 1);
}
// outputs per lane of decim_dot2_ci16 at decimation M: a lane chunk is 16
// input samples (2 plane granules) at every M
__host__ __device__ constexpr int dot2_r(int M) { return 16 / M; }
// run-time tap count (decim_dot2_ci16<0, ...>): N <= kDot2MaxTaps; tap pairs
// padded with zero pairs to whole 4-pair steps (exact: integer products of a
// zero pair add 0), and the halo of that padded count plus one plane granule
// pair (the window granule read one step ahead of the last step)
constexpr int kDot2MaxTaps = 1024;
__host__ __device__ constexpr int dot2_rt_pairs(int ntaps) { return 4 * ceildiv(ntaps / 2 + 1, 4); }
__host__ __device__ constexpr int dot2_rt_halo(int ntaps) {
    return 16 * ceildiv(2 * (dot2_rt_pairs(ntaps) - 1), 16) + 16;
}
// device tap-pair array length: zero pairs of slack past the padded count for
// the chunk of up to 24 pairs requested one chunk ahead
constexpr int dot2_pair_slack = 32;  // >= the largest chunk (24 pairs at M = 1)
__host__ __device__ constexpr int dot2_pair_alloc(int ntaps) { return dot2_rt_pairs(ntaps) + dot2_pair_slack; }
// decim_dot2_ci16<NT, BLOCK, ..., MD>, for the kernel and its launcher: tap
// pairs and halo samples (a whole number of lane chunks) of a compiled tap
// count NT, or (NT = 0) of the run-time count ntaps; input samples per tile
__host__ __device__ constexpr int dot2_pairs(int NT, int ntaps) { return NT == 0 ? dot2_rt_pairs(ntaps) : NT / 2 + 1; }
__host__ __device__ constexpr int dot2_halo(int NT, int ntaps) {
    return NT == 0 ? dot2_rt_halo(ntaps) : 16 * ceildiv(2 * (dot2_pairs(NT, ntaps) - 1), 16);
}
__host__ __device__ constexpr int dot2_spt(int BLOCK, int MD) { return MD * BLOCK * dot2_r(MD); }
__device__ __forceinline__ int32_t clamp_s14(int32_t v) {
    const int32_t a = v >> 14;  // |v| < 2^30: never INT_MIN
    return a > 32767 ? 32767 : (a < -32767 ? -32767 : a);
}
__device__ __forceinline__ uint32_t lo16_pair(uint32_t a, uint32_t b) {  // (lo a, lo b)
    return __builtin_amdgcn_perm(b, a, 0x05040100u);
}
__device__ __forceinline__ uint32_t hi16_pair(uint32_t a, uint32_t b) {  // (hi a, hi b)
    return __builtin_amdgcn_perm(b, a, 0x07060302u);
}
__device__ __forceinline__ int32_t sdot2(uint32_t a, uint32_t b, int32_t c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_, a), __builtin_bit_cast(short2_t_, b), c, false);
}
// dot2 into a fresh accumulator: the VOP3 form with an inline 0 (the compiler
// otherwise materialises the 0 with a v_mov for the accumulating VOP2 form)
__device__ __forceinline__ int32_t sdot2_0(uint32_t a, uint32_t b) {
    int32_t r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// limitScale16 of a complex<int32_t> accumulator pair for a shift in 1..31
// (never INT_MIN after the shift): saturating pack, then -32768 -> -32767
__device__ __forceinline__ uint32_t limit16_pair_sh(int32_t re, int32_t im, unsigned shift) {
    const short2_t_ p = __builtin_amdgcn_cvt_pk_i16(re >> (shift & 31u), im >> (shift & 31u));
    const short2_t_ lo = {-32767, -32767};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(p, lo));
}
// two mixer outputs (int32, >> 14 pending) -> one packed int16 pair clamped to
// +-32767 (limitScale16; |v >> 14| < 2^17 so INT_MIN never occurs):
// saturating v_cvt_pk_i16_i32, then v_pk_max_i16 with -32767
__device__ __forceinline__ uint32_t clamp_pair_s14(int32_t a, int32_t b) {
    const short2_t_ p = __builtin_amdgcn_cvt_pk_i16(a >> 14, b >> 14);
    const short2_t_ lo = {-32767, -32767};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(p, lo));
}

// mixers.h:169-188 on one packed sample with the (lr, li) table word
__device__ __forceinline__ void mix_dot2(uint32_t w, uint32_t C, int32_t &re, int32_t &im) {
    const uint32_t A = __builtin_bit_cast(uint32_t, __builtin_bit_cast(short2_t_, C) * (short2_t_){1, -1});
    const uint32_t ws = __builtin_amdgcn_alignbit(w, w, 16);
    re = clamp_s14(sdot2(w, A, 0));
    im = clamp_s14(sdot2(ws, C, 0));
}

// The same on one staged granule (four packed samples w): the dot2 sums of
// its real (r) and imaginary (i) parts, >> 14 and clamp pending
// (clamp_granule_s14 below).  Two-word table form: sample j's words
// A = (lr, -li) and B = (li, lr), re = dot2(x, A), im = dot2(x, B).
__device__ __forceinline__ void mix_granule_ab(uint4 w, uint4 A, uint4 B, int32_t (&r)[4], int32_t (&i)[4]) {
    r[0] = sdot2_0(w.x, A.x), i[0] = sdot2_0(w.x, B.x);
    r[1] = sdot2_0(w.y, A.y), i[1] = sdot2_0(w.y, B.y);
    r[2] = sdot2_0(w.z, A.z), i[2] = sdot2_0(w.z, B.z);
    r[3] = sdot2_0(w.w, A.w), i[3] = sdot2_0(w.w, B.w);
}
// One-word form: sample j's word C = (lr, li); re = dot2(x, (lr, -li)), im =
// dot2(swap(x), (lr, li)): one negate of the high half and one half swap per sample.
__device__ __forceinline__ void mix_granule_c(uint4 w, uint4 C, int32_t (&r)[4], int32_t (&i)[4]) {
    auto neg_hi = [](uint32_t c) {
        return __builtin_bit_cast(uint32_t, __builtin_bit_cast(short2_t_, c) * (short2_t_){1, -1});
    };
    auto swp = [](uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 16); };
    r[0] = sdot2_0(w.x, neg_hi(C.x)), i[0] = sdot2_0(swp(w.x), C.x);
    r[1] = sdot2_0(w.y, neg_hi(C.y)), i[1] = sdot2_0(swp(w.y), C.y);
    r[2] = sdot2_0(w.z, neg_hi(C.z)), i[2] = sdot2_0(swp(w.z), C.z);
    r[3] = sdot2_0(w.w, neg_hi(C.w)), i[3] = sdot2_0(swp(w.w), C.w);
}
// the granule's half of one plane: the four sums as two clamped int16 pairs
__device__ __forceinline__ uint2 clamp_granule_s14(const int32_t (&v)[4]) {
    return make_uint2(clamp_pair_s14(v[0], v[1]), clamp_pair_s14(v[2], v[3]));
}

}  // namespace srcdsp
