// up_dot2_kernels.h -- the interpolator's handle layout and its v_dot2 tile
// (FilterUpsamplingFir, upsampling_filters.h:36-326), shared by upsamp.hip
// (srcdsp_up_step) and upmix.hip (the interpolator -> mixer chain, which runs
// the same tile with the mixer in its output epilogue); modulate.hip feeds it
// from bits, modulate_offset.hip adds the OQPSK stagger ahead of the mixer,
// modulate_sum.hip runs it once per chain without its store phase and
// resample.hip puts the decimator behind it in place of that phase.
//
// What the six have in common around the tile lives in one place each: which
// instantiations <LR, PPC> a family has and which one a call runs in
// up_dot2_dispatch.h; the tile's size, tile count and LDS here (kUpTile,
// up_tiles, up_dot2_smem); the mixer's kernel prologue and the interpolator +
// mixer half of a launch in upmix_kernels.h; the bits source's prologue and the
// mapper's half in modulate_kernels.h; the stagger's in
// modulate_offset_kernels.h.
#pragma once
#include <string>

#include "ops.h"

#include "up_dot2_dispatch.h"

namespace srcdsp {

enum { UV_CI16_I32 = 0, UV_CI16_I16 = 1, UV_I16_I32 = 2 };
typedef short short2_t_u __attribute__((ext_vector_type(2)));

struct srcdsp_up_state {
    int variant = 0;
    unsigned L = 1;
    int ntaps = 0, H = 0;
    unsigned length = 0;
    int left_shift_factor = 0;
    std::string h_raw;          // the taps as given (CoefType bytes), for copies
    int32_t *d_coef = nullptr;  // polyphase order: d_coef[o*H + i] = c[o + i*L]
    bool coef_i24 = false;      // every tap in (-2^23, 2^23): v_mad_i32_i24
    bool coef_i16 = false;      // every tap in int16 range: v_dot2 tap pairs (variant 0)
    uint32_t *d_pair = nullptr; // per phase o: pairs[o*(H/2+1) + p] = (lo c_o[2p], hi c_o[2p-1])
    void *d_hist[2] = {nullptr, nullptr};
    size_t hist_cap = 0;
    int cur = 0;
    Ordering order;
    HostStage stage;
    // the interpolated stream between the two launches of an unfused
    // interpolator -> decimator call (resample.hip)
    GrowBuf mid{GrowBuf::kDevice};
};

// sample j of the virtual stream (history ++ input ++ flush zeros), as a packed word
template <int UV>
__device__ __forceinline__ uint32_t up_fetch(const void *in, const void *hist, long j, long n_in, int Hm1) {
    if (j < 0) {
        long h = j + Hm1;
        if (h < 0) return 0;
        return UV == UV_I16_I32 ? (uint32_t)(uint16_t)((const int16_t *)hist)[h] : ((const uint32_t *)hist)[h];
    }
    if (j >= n_in) return 0;
    return UV == UV_I16_I32 ? (uint32_t)(uint16_t)((const int16_t *)in)[j] : ((const uint32_t *)in)[j];
}

constexpr int kUpMaxTaps = 4096;

// Tiled polyphase interpolator on v_dot2_i32_i16 (variant 0 with int16-range
// taps, LR in 2..8).  Each lane owns RD = 8 consecutive input samples.  Taps
// of phase o are paired Q_p = (lo c_o[2p+1], hi c_o[2p]) (c_o[H] = 0), p <
// ceil(H/2); the pair of input j multiplies the packed samples (x[j-2p-1],
// x[j-2p]), which for even j = 2m is dword m-p-1 of an odd-aligned plane
// O[e] = (x[2e+1], x[2e+2]) and for odd j = 2m+1 dword m-p of an even-aligned
// plane E[e] = (x[2e], x[2e+1]).  A lane's 8 inputs read O[4t'+r/2-1-p] (even
// r) / E[4t'+(r-1)/2-p] (odd r): one 4-dword register window per plane and
// component sliding one dword per pair, one ds_read_b128 per plane every 4
// pairs.  ceil(H/2) dot2 per phase and component (the (c[2p], c[2p-1])
// pairing needed H/2 + 1).  int16 x int16 -> int32 products, wrap-around
// accumulate: exactly the reference's complex<int32_t> arithmetic.
constexpr int kUpRD = 8, kUpBlockD = 256;
constexpr int kUpTile = kUpRD * kUpBlockD;  // inputs per tile (workgroup)

// tiles (grid.x) of a call of n_total inputs
inline long up_tiles(long n_total) { return (n_total + kUpTile - 1) / kUpTile; }

// dynamic LDS of one tile: the four input planes, reused for the staged output
inline size_t up_dot2_smem(int H, unsigned L) {
    const int PP = (H + 1) / 2, HG = (PP + 3) / 4, PGR = kUpTile / 8 + HG;
    const size_t out_lds = 16 * (size_t)kUpBlockD * (kUpRD * L / 4 + 1);  // staged output tile
    return 4 * 16 * (size_t)PGR > out_lds ? 4 * 16 * (size_t)PGR : out_lds;
}

// behind up_dot2_dispatch (up_dot2_dispatch.h) and the launch in its callback:
// a ratio the family has no kernel for is an error, as is a failed launch
inline int up_dot2_launched(bool served) {
    if (!served) {
        set_error("v_dot2 tile: no kernel of this family for the interpolator's L");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    SRCDSP_HIP_TRY(hipGetLastError());
    return SRCDSP_OK;
}

// Where a tile's input words come from (the staging policy SRC of
// up_dot2_tile): at(j) is input sample j, 0 <= j < n_in, as a packed word;
// load5 the five samples from s0 (a multiple of 4, all five inside the input).
// This one reads the words of a sample buffer, as upsamp.hip and upmix.hip do.
struct UpWordsIn {
    const uint32_t *in;
    __device__ __forceinline__ uint32_t at(long j) const { return in[j]; }
    __device__ __forceinline__ void load5(long s0, uint32_t (&w)[5]) const {
        const uint4 v = *(const uint4 *)(in + s0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = in[s0 + 4];
    }
};

// the interpolator alone: every packed output word is stored as it is
struct UpStoreEpilogue {
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ uint32_t operator()(uint32_t w) { return w; }
};

// no stagger between the clamp and the epilogue: the tile as upsamp.hip,
// upmix.hip and modulate.hip run it
struct UpNoStagger {
    static constexpr bool on = false;
};

// no deeper halo and no second stage behind the tile: every kernel but the
// resampler's (resample_kernels.h)
struct UpNoHalo {
    static constexpr bool on = false;
};

// the uniform delay d (1..K) as a compile-time constant: f(integral_constant<int, d>)
template <int K, class F>
__device__ __forceinline__ void up_stagger_dispatch(int d, F &f) {
    if (d == K) {
        f(std::integral_constant<int, K>{});
    } else if constexpr (K > 1) {
        up_stagger_dispatch<K - 1>(d, f);
    }
}

// The store phase of a tile: the staged output tile in LDS (lane chunk of
// 8 LR words at the padded stride, every wave's chunk written and a barrier
// passed) -> whole-line 16-B stores of the tile's contiguous output.  Shared by
// up_dot2_tile and by the kernels that stage words of their own
// (modulate_sum.hip).
template <int LR, bool NTS>
__device__ __forceinline__ void up_tile_flush(uint4 *ob, int t, uint32_t *out, long j0, long n_total) {
    constexpr int GPLo = kUpRD * LR / 4, STR = GPLo + 1;
    const long wbase = (long)LR * j0;             // first output word of the tile
    const long wend = (long)LR * n_total;         // output words of the call
    // one whole ds_read_b128 per granule (volatile: the compiler split these
    // reads into ds_read_b32 / ds_read2_b32 for the partial-tile branch, whose
    // 32-lane groups at a 16-B stride hit 8 banks: 25 M conflict cycles per
    // launch at L = 4, 2^26 inputs)
    typedef uint32_t o4v_t __attribute__((ext_vector_type(4)));
    typedef const volatile __attribute__((address_space(3))) o4v_t *lds_o4v;
    auto oread = [&](int G) { return *(lds_o4v)(&ob[(G / GPLo) * STR + (G % GPLo)]); };
    if (wbase + 4L * GPLo * kUpBlockD <= wend) {
        // whole tile: every granule read, then every store issued, at one
        // base address (no per-store range checks)
        o4v_t v[GPLo];
#pragma unroll
        for (int i = 0; i < GPLo; ++i) v[i] = oread(i * kUpBlockD + t);
        uint32_t *o = out + wbase + 4L * t;
#pragma unroll
        for (int i = 0; i < GPLo; ++i) {
            if constexpr (NTS) {  // streaming store: the output is written once, 4L x the input bytes
                __builtin_nontemporal_store(v[i], (o4v_t *)(o + 4 * i * kUpBlockD));
            } else {
                *(o4v_t *)(o + 4 * i * kUpBlockD) = v[i];
            }
        }
        return;
    }
    for (int i = 0; i < GPLo; ++i) {  // the call's last, partial tile
        const int G = i * kUpBlockD + t;          // output granule within the tile
        const o4v_t vv4 = oread(G);
        const long w0 = wbase + 4L * G;
        for (int u = 0; u < 4; ++u)
            if (w0 + u < wend) out[w0 + u] = vv4[u];
    }
}

// One tile (blockIdx.x) of the call.
// WS: window register sets (3: the next granule is read a chunk ahead, 150
// VGPRs at LR = 4; 2: it is read at the end of the chunk into the set that
// chunk is done with, <= 128 VGPRs -> 4 waves per SIMD)
// PPC: pairs per phase as a compile-time constant (0: runtime, from H): the
// chunk loop unrolls completely, the window sets rotate without register
// copies and each accumulator starts with a dot2 into an inline 0.
// SRC: where the input words come from (UpWordsIn: a sample buffer).
// EPI: what happens to a lane's 8 LR packed output words on their way to the
// output tile: epi.begin(k) with k the lane's first output word within the
// tile, then epi(word) once per word in output order.
// STG: a delay of stg.D <= LR output words on the imaginary rail between the
// clamp and the epilogue (UpNoStagger: none; the OQPSK stagger of
// modulate_offset.hip).  Output word idx of a lane takes its imaginary half
// from word idx - D: of the lane itself, or of the lane before through the
// padding granule of its output chunk (after the second barrier, so across
// waves too).  The tile's first lane takes them from stg.seed: the carry
// (tile 0) or the last phases of the sample before the tile, recomputed from
// the halo the planes hold (D lanes, ceil(H/2) dot2 each; no workgroup waits
// on another).  The same D lanes of the call's last tile write the new carry.
// STORE: false ends the tile behind the epilogue: nothing is staged or stored
// and `out` is not used; the epilogue keeps what it was given (the summing
// tile of modulate_sum.hip, which runs the tile once per chain).
// HALO: the planes are staged halo.HG granules deep instead of ceil(PP/4), and
// once they are staged halo.fill(t, j0, 8 HG, tile_w) runs, tile_w(jr, o) being
// the clamped output word of phase o of staged sample jr (counted from the
// planes' first sample; jr >= 2 PP) computed on the calling lane (UpNoHalo:
// neither; the resampler's decimator stage, resample_kernels.h, which needs
// the interpolated words before the tile).
template <int LR, bool NTS, int WS, int PPC, class EPI, class SRC, class STG = UpNoStagger, bool STORE = true,
          class HALO = UpNoHalo>
__device__ __forceinline__ void up_dot2_tile(const SRC &src, long n_in, long n_total, const uint32_t *hist_in,
                                             uint32_t *hist_out, const uint32_t *pairs, int H, unsigned shift,
                                             uint32_t *out, EPI &epi, const STG &stg = STG(),
                                             const HALO &halo = HALO()) {
    constexpr int R = kUpRD, TI = R * kUpBlockD;
    extern __shared__ uint4 ug[];  // 4 planes (E_re, E_im, O_re, O_im) of PGR granules each
    const int Hm1 = H - 1;
    const int PP = PPC ? PPC : (H + 1) / 2;  // pairs per phase
    // halo granules per plane (window reach: dword D0 - PP)
    const int HG = [&] {
        if constexpr (HALO::on) {
            return halo.HG;
        } else {
            return (PP + 3) / 4;
        }
    }();
    const int PGR = TI / 8 + HG;         // granules per plane (4 dwords = 8 samples)
    const int t = threadIdx.x;
    // sample j of the virtual stream (history ++ input ++ flush zeros)
    auto fetch = [&](long j) -> uint32_t {
        if (j < 0) return j + Hm1 < 0 ? 0u : hist_in[j + Hm1];
        return j >= n_in ? 0u : src.at(j);
    };
    if (blockIdx.x == 0) {
        for (int k = t; k < Hm1; k += kUpBlockD) {
            const long j = n_total - Hm1 + k;
            hist_out[k] = fetch(j);
        }
    }
    const long j0 = (long)blockIdx.x * TI;
    // staging: sample granule g (4 samples from j0 - 8*HG + 4g) -> plane dwords 2g, 2g+1
    uint32_t *pl = (uint32_t *)ug;
    const int PDW = 4 * PGR;  // dwords per plane
    const int ng = 2 * PGR;
    auto lo = [](uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); };
    auto hi = [](uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); };
    auto put = [&](int g, const uint32_t (&w)[5]) {
        *(uint2 *)&pl[0 * PDW + 2 * g] = make_uint2(lo(w[0], w[1]), lo(w[2], w[3]));
        *(uint2 *)&pl[1 * PDW + 2 * g] = make_uint2(hi(w[0], w[1]), hi(w[2], w[3]));
        *(uint2 *)&pl[2 * PDW + 2 * g] = make_uint2(lo(w[1], w[2]), lo(w[3], w[4]));
        *(uint2 *)&pl[3 * PDW + 2 * g] = make_uint2(hi(w[1], w[2]), hi(w[3], w[4]));
    };
    // a tile whose whole span (halo included) lies inside the input: the
    // lane's first three granules are loaded together, then written (one
    // exposed load latency per tile instead of one per granule)
    constexpr int NI = 3;
    const bool interior = j0 - 8L * HG >= 0 && j0 + TI + 1 <= n_in;
    int g1 = t;  // first granule of the generic loop
    if (interior) {
        uint32_t w[NI][5];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int g = t + i * kUpBlockD;
            if (i < 2 || g < ng) {  // ng >= 2 * kUpBlockD
                src.load5(j0 - 8L * HG + 4L * g, w[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i < 2 || t + i * kUpBlockD < ng) put(t + i * kUpBlockD, w[i]);
        g1 = t + NI * kUpBlockD;
    }
    for (int g = g1; g < ng; g += kUpBlockD) {
        const long s0 = j0 - 8L * HG + 4L * g;
        uint32_t w[5];
        if (s0 >= 0 && s0 + 5 <= n_in) {
            src.load5(s0, w);
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) w[k] = fetch(s0 + k);
        }
        put(g, w);
    }
    __syncthreads();
    if constexpr (STG::on) {
        // (ahead of the main loop, where no accumulator is live: behind it the
        // unrolled loop was scheduled for 180 instead of 77 VGPRs at (2, 32))
        // the clamped imaginary output of phase o of staged sample jr (counted
        // from the planes' first sample), on one lane: the pairs of the main
        // loop, p-th pair on dword m - p of plane E_im (jr = 2m + 1) or dword
        // m - 1 - p of plane O_im (jr = 2m)
        auto tile_q = [&](int jr, int o) -> uint32_t {
            const uint32_t *pq = pl + ((jr & 1) ? 1 * PDW + (jr >> 1) : 3 * PDW + (jr >> 1) - 1);
            int32_t acc = 0;
#pragma unroll 8  // 8 tap and 8 plane loads in flight
            for (int p = 0; p < PP; ++p)
                acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, pq[-p]),
                                             __builtin_bit_cast(short2_t_u, pairs[p * LR + o]), acc, false);
            return limit_t16_pair(0, acc, shift) >> 16;
        };
        stg.template seed<LR>(t, j0, n_total, 8 * HG, tile_q);
    }
    if constexpr (HALO::on) {
        // as tile_q, both components: pair p on dwords m - p of planes E_re /
        // E_im (jr = 2m + 1) or m - 1 - p of planes O_re / O_im (jr = 2m)
        auto tile_w = [&](int jr, int o) -> uint32_t {
            const uint32_t *pr = pl + ((jr & 1) ? (jr >> 1) : 2 * PDW + (jr >> 1) - 1), *pi = pr + PDW;
            int32_t ar = 0, ai = 0;
#pragma unroll 8  // 8 tap and 16 plane loads in flight
            for (int p = 0; p < PP; ++p) {
                const short2_t_u c = __builtin_bit_cast(short2_t_u, pairs[p * LR + o]);
                ar = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, pr[-p]), c, ar, false);
                ai = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, pi[-p]), c, ai, false);
            }
            return limit_t16_pair(ar, ai, shift);
        };
        halo.fill(t, j0, 8 * HG, tile_w);
    }
    // lane base: input j0 + 8t = plane dword D0 = 4t + 4*HG (granule gb).  Input
    // r, pair p reads dword D0 + k - p, k = r/2 - 1 in plane O for even r,
    // k = (r-1)/2 in plane E for odd r:
    // for the chunk of pairs 4q..4q+3 those are dwords of granules gb - q
    // (`cur`) and gb - q - 1 (`nxt`), two register sets that swap roles.
    const int gb = t + HG;
    int32_t yr[LR][R], yi[LR][R];
    if constexpr (PPC == 0) {
#pragma unroll
        for (int o = 0; o < LR; ++o)
#pragma unroll
            for (int r = 0; r < R; ++r) yr[o][r] = yi[o][r] = 0;
    }
    ConstPtr<uint32_t> tp = const_view<uint32_t>(pairs);
    // Three window register sets rotate over the chunks and the taps of a
    // chunk (4 pairs x LR phases, contiguous: dword (4q + pp) LR + o) arrive in
    // one s_load; both for chunk q+1 are requested after chunk q's first pair,
    // so the lgkmcnt wait at chunk q+1 lands three pairs of dot2 after them
    // (waiting on a tap s_load drains every LDS read in flight too).
    uint32_t W0[4][4], W1[4][4], W2[4][4];  // [plane][dword]
    constexpr int TPC = 4 * LR;            // tap dwords per chunk
    uint32_t Tc[TPC], Tn[TPC];
    auto load = [&](uint32_t (&w)[4][4], int gi) {
#pragma unroll
        for (int pl4 = 0; pl4 < 4; ++pl4) {
            typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
            // volatile keeps every window read a whole ds_read_b128
            // (conflict-free at the lanes' 16-B stride): at the window's far end
            // the compiler would read only the dwords used, as ds_read_b32 /
            // ds_read2_b32, whose 32-lane groups at a 16-B stride hit 8 banks
            typedef const volatile __attribute__((address_space(3))) u4v_t *lds_u4v;
            const u4v_t v = *(lds_u4v)(&ug[pl4 * PGR + gi]);
            w[pl4][0] = v[0]; w[pl4][1] = v[1]; w[pl4][2] = v[2]; w[pl4][3] = v[3];
        }
    };
    auto load_taps = [&](uint32_t (&T)[TPC], int q) {
        asm volatile("" : "+s"(tp));
#pragma unroll
        for (int i = 0; i < TPC; ++i) T[i] = tp[q * TPC + i];
    };
    const int NQ = (PP + 3) / 4;
    auto chunk = [&](int q, const uint32_t (&cur)[4][4], const uint32_t (&nxt)[4][4], uint32_t (&nn)[4][4]) {
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
            const int p = 4 * q + pp;
            if (p >= PP) break;  // the last chunk only
            if (WS == 3 && pp == 1 && q + 1 < NQ) {
                load(nn, gb - q - 2);
                load_taps(Tn, q + 1);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = (r & 1) ? (r >> 1) : (r >> 1) - 1, rel = k - pp;  // -4..3
                const int pr = (r & 1) ? 0 : 2, pi = pr + 1;  // planes E_re/E_im or O_re/O_im
                const uint32_t xr = rel >= 0 ? cur[pr][rel] : nxt[pr][rel + 4];
                const uint32_t xi = rel >= 0 ? cur[pi][rel] : nxt[pi][rel + 4];
#pragma unroll
                for (int o = 0; o < LR; ++o) {
                    const uint32_t P = Tc[pp * LR + o];
                    if (PPC && q == 0 && pp == 0) {  // first pair: into an inline 0
                        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(yr[o][r]) : "v"(xr), "s"(P));
                        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(yi[o][r]) : "v"(xi), "s"(P));
                    } else {
                        yr[o][r] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, xr),
                                                          __builtin_bit_cast(short2_t_u, P), yr[o][r], false);
                        yi[o][r] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, xi),
                                                          __builtin_bit_cast(short2_t_u, P), yi[o][r], false);
                    }
                }
            }
        }
        if constexpr (WS == 3) {
#pragma unroll
            for (int i = 0; i < TPC; ++i) Tc[i] = Tn[i];
        }
    };
    load(W0, gb);
    load(W1, gb - 1);
    load_taps(Tc, 0);
    int q = 0;
    if constexpr (WS == 3) {
#pragma unroll
        for (; q + 3 <= NQ; q += 3) {
            chunk(q, W0, W1, W2);
            chunk(q + 1, W1, W2, W0);
            chunk(q + 2, W2, W0, W1);
        }
        if (q < NQ) chunk(q, W0, W1, W2);
        if (q + 1 < NQ) chunk(q + 1, W1, W2, W0);
    } else {
        // chunk q reads granules gb-q (cur) and gb-q-1 (nxt); the next chunk's
        // new granule gb-q-2 goes into cur once this chunk is done with it
        (void)W2;
        auto chunk2 = [&](int qq, uint32_t (&cur)[4][4], const uint32_t (&nxt)[4][4]) {
            uint32_t none[4][4];
            chunk(qq, cur, nxt, none);  // no early read (nn unused when WS == 2)
            if (qq + 1 < NQ) {
                load(cur, gb - qq - 2);
                load_taps(Tc, qq + 1);
            }
        };
#pragma unroll
        for (; q + 2 <= NQ; q += 2) {
            chunk2(q, W0, W1);
            chunk2(q + 1, W1, W0);
        }
        if (q < NQ) chunk2(q, W0, W1);
    }
    // outputs -> LDS (lane chunk of 8*LR words at a 9-granule stride for LR = 4,
    // conflict-free) -> whole-line 16-B stores of the tile's contiguous output
    constexpr int GPLo = R * LR / 4;    // output granules per lane
    constexpr int STR = GPLo + 1;       // padded lane stride (odd)
    // (each lane storing its own 128-B output line directly, 8 x 16 B at a
    // 128-B lane stride, measured 30 % slower with plain stores and 5.5x
    // slower with nt stores than this LDS transpose into whole-line stores:
    // profiles/tuning/r03_up_stage_ab.txt)
    __syncthreads();                    // every wave is done reading the planes
    uint4 *ob = ug;
    auto word = [&](int idx) { return limit_t16_pair(yr[idx % LR][idx / LR], yi[idx % LR][idx / LR], shift); };
    uint32_t qp[4] = {0, 0, 0, 0};     // the 8 imaginary halves before the lane's first word, two per dword
    if constexpr (STG::on) {
        constexpr int T0 = R * LR - 8;
        ob[t * STR + GPLo] = make_uint4(hi(word(T0), word(T0 + 1)), hi(word(T0 + 2), word(T0 + 3)),
                                        hi(word(T0 + 4), word(T0 + 5)), hi(word(T0 + 6), word(T0 + 7)));
        __syncthreads();
        const uint4 v = t ? ob[(t - 1) * STR + GPLo] : stg.seeds();
        qp[0] = v.x; qp[1] = v.y; qp[2] = v.z; qp[3] = v.w;
    }
    auto emit = [&](auto dc) {
        constexpr int DC = decltype(dc)::value;  // 0: no stagger
        epi.begin(R * LR * t);
#pragma unroll
        for (int k = 0; k < GPLo; ++k) {
            uint32_t w4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = 4 * k + u;
                uint32_t w = word(idx);
                if constexpr (DC > 0) {
                    if (idx >= DC) {
                        w = __builtin_amdgcn_perm(word(idx - DC), w, 0x07060100u);
                    } else {
                        const int e = 8 + idx - DC;
                        w = __builtin_amdgcn_perm(qp[e >> 1], w, (e & 1) ? 0x07060100u : 0x05040100u);
                    }
                }
                w4[u] = epi(w);
            }
            if constexpr (STORE) ob[t * STR + k] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
    };
    if constexpr (STG::on) {
        up_stagger_dispatch<LR>(stg.D, emit);
    } else {
        emit(std::integral_constant<int, 0>{});
    }
    if constexpr (STORE) {
        __syncthreads();
        up_tile_flush<LR, NTS>(ob, t, out, j0, n_total);
    }
}

}  // namespace srcdsp

struct srcdsp_up { srcdsp::srcdsp_up_state u; };
