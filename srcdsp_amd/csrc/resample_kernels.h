// resample_kernels.h -- the interpolator -> decimator tile (resample.hip):
// FilterUpsamplingFir::step (upsampling_filters.h:149-233) then
// FilterDnsamplingFir::step (dnsampling_filters.h:129-172) on one workgroup's
// LDS, the L x interpolated stream never reaching memory.
//
// The tile is up_dot2_tile (up_dot2_kernels.h) with its store phase off.  Its
// epilogue puts the lane's clamped words into the "mid" plane behind the input
// planes, de-interleaved: entry e = (re pair, im pair) of local words 2e and
// 2e + 1 (resample_index.h), one ds_write_b128 per four words.  ONE plane
// serves both parities of i M - k, because the parity moves into the taps:
// output y = sum_k c[k] x[a - k] pairs, for an even local word a, (x[a - 2j],
// x[a - 2j + 1]) = entry a/2 - j with P_j = (c[2j], c[2j-1]); for an odd a,
// (x[a - 2j - 1], x[a - 2j]) = entry (a-1)/2 - j with P'_j = (c[2j+1], c[2j]).
// So no second, odd-aligned pair of planes (half the LDS: 64 KiB instead of
// 128 at L = 8) and no realignment of the data; a lane picks its tap table.
//
// Decimator stage.  Lane t takes outputs i_lo + t + 256 k of the tile's range
// (resample_index.h), four at a time (256 M words apart: one parity); per pair
// and output one ds_read_b64 (both components) and two v_dot2_i32_i16.  Both
// tap tables are staged in LDS behind the mid plane and read four pairs at a
// time at one address for all lanes (a broadcast ds_read_b128), so the loop
// waits on LDS alone, whose reads return in order (a scalar tap load drains
// every LDS read in flight).  With M even every output is even-aligned and
// only P is read.  int32 wrap-around accumulation, limitScale16 (common.h:
// limit16), a coalesced dword store per output: a wave writes 256 contiguous
// bytes.
//
// Halo.  The HP = rs_halo_words(N_d) words before the tile come from the
// decimator's history in tile 0 and are recomputed in every other tile from
// input planes staged rs_halo_granules deep (one lane per entry, 2 x 2 x
// ceil(H/2) dot2): no workgroup waits on another.  The last tile writes the
// decimator's new history from the plane (in tile 0 the old history is its
// halo, which is the sliding rule when L n < N_d - 1); tile 0 writes the
// interpolator's, as in every kernel built on the tile.
//
// N_d cap: kRsMaxDecimTaps = 1024, the decimator's own v_dot2 limit
// (kDot2MaxTaps).  LDS at the cap: HP = 1032 halo words are 4128 B of the mid
// plane and ceil(HP / L / 8) more granules of each input plane; with L = 8 and
// kUpMaxTaps interpolator taps that is rs_smem(512, 8, 1024) = 21 568 B of
// planes + 69 680 B of mid plane + 4128 B of tap pairs = 95 376 B, inside the
// 160 KiB of a CU.
#pragma once
#include "ops.h"

#include "resample_index.h"
#include "up_dot2_kernels.h"

namespace srcdsp {

constexpr int kRsMaxDecimTaps = 1024;
static_assert(kRsTile == kUpTile, "the interpolator's tile");
static_assert(rs_smem(kUpMaxTaps / 8, 8, kRsMaxDecimTaps) <= 160 * 1024, "LDS of a CU");

struct ResampleLaunch {
    const uint32_t *in;
    uint32_t *out;
    const uint32_t *pairs;  // the interpolators' tap pairs (srcdsp_up_state::d_pair), shared
    const uint32_t *cpair;  // the decimators' (FirCore::d_cpair), shared
    long n_in, n_total, n_out;
    long in_stride, out_stride;  // samples, between channels (grid.y)
    int H, Nd, M;
    unsigned shift_up, shift_dn;
    int HP, HG;          // rs_halo_words, rs_halo_granules
    unsigned mid_off;    // byte offset of the mid plane in dynamic LDS
    const uint32_t *uhist_in[kMaxBatch];
    uint32_t *uhist_out[kMaxBatch];
    const uint32_t *dhist_in[kMaxBatch];
    uint32_t *dhist_out[kMaxBatch];
};

__device__ __forceinline__ uint32_t rs_lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t rs_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// the tile's epilogue: the lane's words into its entries of the mid plane
struct RsMidEpilogue {
    uint2 *tile;  // the entry of the tile's first word
    uint2 *p;
    uint32_t w0, w1, w2;
    int i;
    __device__ __forceinline__ void begin(int k) {
        p = tile + (k >> 1);
        i = 0;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t x) {
        switch (i & 3) {  // i is a constant in the tile's unrolled emit loop
        case 0: w0 = x; break;
        case 1: w1 = x; break;
        case 2: w2 = x; break;
        default:
            *(uint4 *)p = make_uint4(rs_lo(w0, w1), rs_hi(w0, w1), rs_lo(w2, x), rs_hi(w2, x));
            p += 2;
        }
        ++i;
        return 0;
    }
};

// the tile's halo policy (up_dot2_tile's HALO)
struct RsHalo {
    static constexpr bool on = true;
    int HG;
    int HP, L, Nd;
    long tile;
    const uint32_t *dhist;  // the decimator's history: the N_d - 1 mid words before the call
    uint2 *mid;
    template <class F>
    __device__ __forceinline__ void fill(int t, long, int, F &tile_w) const {
        for (int e = t; e < HP / 2; e += kUpBlockD) {
            uint32_t w0, w1;
            if (tile == 0) {
                const int k = 2 * e - HP + Nd - 1;  // word k of the history; before it: zeros never tapped
                w0 = k >= 0 ? dhist[k] : 0u;
                w1 = k + 1 >= 0 ? dhist[k + 1] : 0u;
            } else {
                int jr = rs_halo_sample(2 * e, tile, L, HP, HG), o = rs_halo_phase(2 * e, tile, L, HP);
                w0 = tile_w(jr, o);
                if (++o == L) {
                    o = 0;
                    ++jr;
                }
                w1 = tile_w(jr, o);
            }
            mid[e] = make_uint2(rs_lo(w0, w1), rs_hi(w0, w1));
        }
    }
};

template <int LR, int PPC>
__global__ __launch_bounds__(kUpBlockD) void resample_tile_dot2(const ResampleLaunch P) {
    extern __shared__ uint4 ug[];
    const int c = blockIdx.y, t = threadIdx.x;
    const long tile = blockIdx.x;
    uint2 *mid = (uint2 *)((char *)ug + P.mid_off);
    const int HP = P.HP;
    // the decimator's tap pairs behind the mid plane, zero pairs up to a whole
    // four: P_j = (lo c[2j], hi c[2j-1]) for an even-aligned output, then P'_j =
    // (lo c[2j+1], hi c[2j]) = (hi of P_j+1, lo of P_j) for an odd-aligned one;
    // visible to the decimator stage through the tile's barriers
    const int J4 = rs_decim_pairs4(P.Nd);
    uint32_t *taps = (uint32_t *)((char *)mid + rs_mid_bytes(LR, HP));
    for (int i = t; i < J4; i += kUpBlockD) {
        const int J = rs_decim_pairs(P.Nd);
        const uint32_t p0 = i < J ? P.cpair[i] : 0u, p1 = i + 1 < J ? P.cpair[i + 1] : 0u;
        taps[i] = p0;
        taps[J4 + i] = (p1 >> 16) | (p0 << 16);
    }
    RsMidEpilogue epi;
    epi.tile = mid + HP / 2;
    const RsHalo halo{P.HG, HP, LR, P.Nd, tile, P.dhist_in[c], mid};
    up_dot2_tile<LR, true, 3, PPC, RsMidEpilogue, UpWordsIn, UpNoStagger, false, RsHalo>(
        UpWordsIn{P.in + c * P.in_stride}, P.n_in, P.n_total, P.uhist_in[c], P.uhist_out[c], P.pairs, P.H, P.shift_up,
        nullptr, epi, UpNoStagger(), halo);
    __syncthreads();  // halo and tile words are in the plane
    const int M = P.M;
    const long m0 = (long)LR * kRsTile * tile;  // the tile's first mid word
    const long i_lo = rs_out_lo(tile, LR, M), i_hi = rs_out_hi(tile, LR, M, P.n_out);
    uint32_t *out = P.out + c * P.out_stride;
    typedef uint32_t u2v_t __attribute__((ext_vector_type(2)));
    typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
    // whole ds_read_b64 / ds_read_b128, as the tile's window reads
    typedef const volatile __attribute__((address_space(3))) u2v_t *lds_u2v;
    typedef const volatile __attribute__((address_space(3))) u4v_t *lds_u4v;
    constexpr int NO = 4;  // outputs of a lane in flight
    // ODD: some local words a are odd (M odd); with M even every a is even (L *
    // kRsTile and HP are).  A lane's NO outputs lie 256 M words apart: one parity.
    auto stage = [&](auto odd) {
        constexpr bool ODD = decltype(odd)::value;
        for (long ib = i_lo + t; ib < i_hi; ib += NO * kUpBlockD) {
            int pe[NO];  // the entry of pair 0
            int32_t ar[NO], ai[NO];
            bool lane_odd = false;
#pragma unroll
            for (int u = 0; u < NO; ++u) {
                long i = ib + (long)u * kUpBlockD;
                i = i < i_hi ? i : i_hi - 1;  // past the range: computed again, not stored
                const int a = (int)(i * M - m0) + HP;
                pe[u] = a >> 1;
                ar[u] = ai[u] = 0;
                if (ODD && u == 0) lane_odd = a & 1;
            }
            for (int j4 = 0; j4 < J4; j4 += 4) {
                // one address for every lane: a broadcast
                u4v_t tp = *(lds_u4v)&taps[j4];
                if constexpr (ODD) {
                    const u4v_t to = *(lds_u4v)&taps[J4 + j4];
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp) tp[pp] = lane_odd ? to[pp] : tp[pp];
                }
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {
                    const short2_t_u tap = __builtin_bit_cast(short2_t_u, (uint32_t)tp[pp]);
#pragma unroll
                    for (int u = 0; u < NO; ++u) {
                        const u2v_t cur = *(lds_u2v)&mid[pe[u] - j4 - pp];
                        ar[u] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, (uint32_t)cur[0]), tap, ar[u], false);
                        ai[u] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t_u, (uint32_t)cur[1]), tap, ai[u], false);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < NO; ++u) {
                const long i = ib + (long)u * kUpBlockD;
                // limitScale16 of the accumulator pair (dnsampling_filters.h:167-168)
                if (i < i_hi) out[i] = pack16(limit16(ar[u], P.shift_dn), limit16(ai[u], P.shift_dn));
            }
        }
    };
    if (M & 1)
        stage(std::true_type{});
    else
        stage(std::false_type{});
    if (tile == (long)gridDim.x - 1) {
        // the decimator's new history: the last N_d - 1 mid words of history ++ call
        const long first = (long)LR * P.n_total - (P.Nd - 1) - m0 + HP;  // local word of history word 0
        for (int k = t; k < P.Nd - 1; k += kUpBlockD) {
            const int a = (int)first + k;
            const uint2 v = mid[a >> 1];
            P.dhist_out[c][k] = (a & 1) ? (v.x >> 16) | (v.y & 0xffff0000u) : (v.x & 0xffffu) | (v.y << 16);
        }
    }
}

}  // namespace srcdsp
