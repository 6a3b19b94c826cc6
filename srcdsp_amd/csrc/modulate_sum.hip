// modulate_sum.hip -- C transmit chains from bits summed onto ONE wire in one
// call (srcdsp_modulate_sum_step): what srcdsp_modulate_offset_step_batched
// (modulators.h:103-117 / :169-184, upsampling_filters.h:149-233, the Q-rail
// stagger, mixers.h:169-188; without staggers srcdsp_modulate_step_batched)
// into C private rows and srcdsp_combine_step over them (limitScale,
// dsp_complex.h:83-108) leave, output and every handle's state bit for bit,
// without the [C, n_out] rows in between.
//
// The fused kernel.  One workgroup per output tile (blockIdx.x, no grid.y)
// loops over the chains of the launch.  Per chain it runs modulate_offset.hip's
// tile (up_dot2_kernels.h with STORE off: staging from row c's bits, the
// stagger's seed, the v_dot2 loop, the interpolator's clamp, the stagger, the
// mixer epilogue with chain c's phase) and, where that tile stages the mixed
// words, adds them into int32 sums, 2 * 8 L per lane, kept in registers.  The
// same tile that writes hist_out[c], carry_out[c] and the QPSK st_out[c] in the
// bank writes them here.  After the last chain the sums go through
// combine_word (combine_kernels.h, the one source of that arithmetic) into the
// tile's LDS transpose and out in whole-line non-temporal 16-byte stores.  The
// mixer table is staged once per workgroup; no workgroup waits on another and
// there are no atomics.
//
// Dispatch.  The fused kernel takes what the bank's one-launch path takes
// (modulate_offset.hip: variant 0 with int16-range taps, N <= 4096, D <= L,
// d_bits 16-byte aligned, bits_stride a multiple of 16) with L = 2, 4 or 8
// (L = 8 with a stagger: D = 4, the half symbol, which the kernel compiles in), at
// most kMaxBatch chains and d_out 16-byte aligned.  Of these it serves the
// calls modsum_route(L) names: its only parallelism is across tiles and it runs
// one wave per SIMD, so it wins only on long rows at L = 2 (DESIGN 5.8c has the
// figures).  Every other legal call runs the bank into grow-only rows on the
// lead mapper, then the combiner, inside the call.
#include <algorithm>
#include <atomic>

#include "combine_kernels.h"
#include "modulate_offset_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_fused_calls, g_bank_calls;

// the kernel's L (a workgroup takes kUpTile symbols); the others go to the bank
bool modsum_serves(unsigned L) { return UpDot2SummingTile::has((int)L, 0); }

// The calls the fused kernel serves of those it takes: at least min_tiles tiles
// (0: none) and at most max_channels chains.  Measured (DESIGN 5.8c,
// profiles/modulate_sum_time.json): at L = 2 it is faster than the bank and the
// combiner by more than their twice-timed spread from 2048 tiles on with 2 and
// with 8 chains, and not with 64 up to the 1024 tiles measured; at L = 4 and
// L = 8 it is not faster at any length measured (one wave per SIMD against the
// bank's four), so no call is routed to it there.
struct SumRoute {
    long min_tiles;
    int max_channels;
};
constexpr SumRoute kSumRouteL2{2048, 8}, kSumRouteNone{0, 0};
std::atomic<long> g_min_tiles{0};  // > 0: set by srcdsp_modulate_sum_set_min_tiles, for every L the kernel has

SumRoute modsum_route(unsigned L) {
    if (!modsum_serves(L)) return kSumRouteNone;
    const long forced = g_min_tiles.load(std::memory_order_relaxed);
    if (forced > 0) return SumRoute{forced, kMaxBatch};
    return L == 2 ? kSumRouteL2 : kSumRouteNone;
}

// Where the sums of a lane live: registers (2 NW VGPRs), or the lane's own
// column of an int32 tile [2 NW][256] in LDS behind the seed slot (no barrier:
// no other lane touches it).  The A/B is profiles/tuning/modulate_sum_sums.json
#ifdef SRCDSP_MODSUM_FORCE_LDS_SUMS  // a tuning build: 0 or 1 for every L (scripts/modulate_sum_ab.py)
constexpr bool modsum_lds_sums(int LR) { return SRCDSP_MODSUM_FORCE_LDS_SUMS != 0 && LR <= 4; }  // L = 8: 128 KiB
#else
constexpr bool modsum_lds_sums(int) { return false; }
#endif

// the tile's epilogue: the mixer, then onto the sums of the lane's word
template <int NW>
struct UpMixSumRegs {
    UpMixEpilogue mix;
    int32_t re[NW], im[NW];
    int i;
    __device__ __forceinline__ void zero(void *) {
#pragma unroll
        for (int k = 0; k < NW; ++k) re[k] = im[k] = 0;
    }
    __device__ __forceinline__ void begin(int k) {
        mix.begin(k);
        i = 0;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t w) {
        combine_add(re[i], im[i], mix(w));
        ++i;
        return 0;
    }
    __device__ __forceinline__ uint32_t word(int k, unsigned shift) const { return combine_word(re[k], im[k], shift); }
};

template <int NW>
struct UpMixSumLds {
    UpMixEpilogue mix;
    int32_t *col;  // the lane's column: re of word k at col[2 k * 256], im at col[(2 k + 1) * 256]
    int i;
    __device__ __forceinline__ void zero(void *tile) {
        col = (int32_t *)tile + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 2 * NW; ++k) col[k * kUpBlockD] = 0;
    }
    __device__ __forceinline__ void begin(int k) {
        mix.begin(k);
        i = 0;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t w) {
        int32_t re = col[2 * i * kUpBlockD], im = col[(2 * i + 1) * kUpBlockD];
        combine_add(re, im, mix(w));
        col[2 * i * kUpBlockD] = re;
        col[(2 * i + 1) * kUpBlockD] = im;
        ++i;
        return 0;
    }
    __device__ __forceinline__ uint32_t word(int k, unsigned shift) const {
        return combine_word(col[2 * k * kUpBlockD], col[(2 * k + 1) * kUpBlockD], shift);
    }
};

inline size_t modsum_lds_bytes(unsigned L) { return 2 * (size_t)kUpRD * L * kUpBlockD * 4; }

// STG: the chains have a stagger; LDSS: the sums live in LDS
template <int LR, int PPC, bool STG, bool LDSS>
__global__ __launch_bounds__(kUpBlockD) void modsum_tile_dot2(const ModOffLaunch A, const int nc, const unsigned cshift,
                                                              uint32_t *const wire) {
    extern __shared__ uint4 ug[];
    constexpr int NW = kUpRD * LR, GPLo = NW / 4, STR = GPLo + 1;
    constexpr int WS = 3;
    const ModLaunch &Q = A.mod;
    const UpmixLaunch &P = Q.up;
    const int t = threadIdx.x;
    typedef typename std::conditional<LDSS, UpMixSumLds<NW>, UpMixSumRegs<NW>>::type Sum;
    Sum epi;
    upmix_stage_table(epi.mix, P, ug);  // once per workgroup
    epi.zero((char *)ug + A.slot_off + 16);
    const unsigned long w0 = upmix_tile_word<LR>();
    for (int c = 0; c < nc; ++c) {
        // the chain before is done with the planes' padding granules and the seed slot
        if (c) __syncthreads();
        upmix_aim<LR>(epi.mix, P, c, w0);
        const UpBitsIn src = mod_bits_row(Q, c);
        if constexpr (STG && LR == 8) {
            // the delay of half a symbol, compiled in: eight emit loops for a
            // run-time delay, each over 128 sums, do not fit the register file
            typedef UpQStaggerOf<std::integral_constant<int, LR / 2>> Half;
            const Half stg{{}, A.carry_in[c], A.carry_out[c], (uint16_t *)((char *)ug + A.slot_off)};
            up_dot2_tile<LR, true, WS, PPC, Sum, UpBitsIn, Half, false>(
                src, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c], P.pairs, P.H, P.shift, nullptr, epi, stg);
        } else if constexpr (STG) {
            const UpQStagger stg{A.D, A.carry_in[c], A.carry_out[c], (uint16_t *)((char *)ug + A.slot_off)};
            up_dot2_tile<LR, true, WS, PPC, Sum, UpBitsIn, UpQStagger, false>(
                src, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c], P.pairs, P.H, P.shift, nullptr, epi, stg);
        } else {
            up_dot2_tile<LR, true, WS, PPC, Sum, UpBitsIn, UpNoStagger, false>(
                src, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c], P.pairs, P.H, P.shift, nullptr, epi);
        }
    }
    __syncthreads();  // every wave is done with the last chain's planes
#pragma unroll
    for (int k = 0; k < GPLo; ++k)
        ug[t * STR + k] = make_uint4(epi.word(4 * k, cshift), epi.word(4 * k + 1, cshift), epi.word(4 * k + 2, cshift),
                                     epi.word(4 * k + 3, cshift));
    __syncthreads();
    up_tile_flush<LR, true>(ug, t, wire, (long)kUpTile * blockIdx.x, P.n_total);
}

// what the fused kernel takes of a checked call, the tile count aside
bool fused_takes(const srcdsp_up_state &u, const MixerState &m, const srcdsp_stagger_t *stags, int channels,
                 const void *d_bits, size_t bits_stride, const void *d_out) {
    const unsigned D = stags ? stags[0]->g.D : 0;
    // L = 8: the delay is compiled in (half a symbol), see the kernel
    return upmix_fused_takes(u, m, d_bits, d_out) && D <= u.L && (!stags || u.L != 8 || D == 4) &&
           bits_stride % 16 == 0 && channels <= kMaxBatch && modsum_serves(u.L);
}

template <int LR, int PPC, bool STG>
int launch_one(const ModOffLaunch &A, int nc, unsigned shift, void *d_out, unsigned tiles, size_t smem, hipStream_t s) {
    constexpr bool LDSS = modsum_lds_sums(LR);
    auto kern = modsum_tile_dot2<LR, PPC, STG, LDSS>;
    if (LDSS) {
        smem += modsum_lds_bytes(LR);
        // beyond the default limit of dynamic LDS: the kernel's largest launch, so once per kernel
        int rc = raise_lds_limit((const void *)kern, up_dot2_smem(kUpMaxTaps / LR, LR) + 2 * kUpmixMaxN + 32 +
                                                         modsum_lds_bytes(LR));
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(kUpBlockD), smem, s, A, nc, shift, (uint32_t *)d_out);
    return SRCDSP_OK;
}

// the checked call on the fused kernel: a shape fused_takes accepts
int sum_fused(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_stagger_t *stags,
              const srcdsp_mixer_t *mixers, int nc, const void *d_bits, size_t bits_stride, void *d_out, size_t n_bits,
              size_t n_sym, long n_total, unsigned shift, hipStream_t s) {
    const srcdsp_up_state &u0 = ups[0]->u;
    ModOffLaunch A{};
    size_t smem = 0;
    int rc = modoff_launch_begin(A, maps, ups, stags, mixers, nc, d_bits, bits_stride, nullptr, 0, n_bits, n_sym,
                                 n_total, false, s, &smem);
    if (rc) return rc;
    const unsigned tiles = (unsigned)up_tiles(n_total);
    const bool served = up_dot2_dispatch<UpDot2SummingTile>(u0.L, (u0.H + 1) / 2, [&](auto lr, auto ppc) {
        constexpr int LR = decltype(lr)::value, PPC = decltype(ppc)::value;
        rc = stags ? launch_one<LR, PPC, true>(A, nc, shift, d_out, tiles, smem, s)
                   : launch_one<LR, PPC, false>(A, nc, shift, d_out, tiles, smem, s);
    });
    if (!rc) rc = up_dot2_launched(served);
    if (rc) return rc;
    return modoff_launch_commit(maps, ups, stags, mixers, nc, n_bits, n_total, s);
}

// the checked call through the bank: C rows on the lead mapper, whose event
// orders their reuse, then the combiner
int sum_bank(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_stagger_t *stags,
             const srcdsp_mixer_t *mixers, int channels, const void *d_bits, size_t bits_stride, void *d_out,
             size_t n_out, size_t n_bits, bool flush, unsigned shift, void *stream) {
    MapperState &lead = maps[0]->m;
    const size_t stride = (n_out + 3) & ~(size_t)3;  // rows 16 bytes apart: the bank's launch, the combiner's 16-byte loads
    int rc = lead.touch();
    if (!rc) rc = lead.order.before((hipStream_t)stream);
    if (!rc) rc = lead.rows.reserve(4 * stride * (size_t)channels);
    if (!rc)
        rc = stags ? srcdsp_modulate_offset_step_batched(maps, ups, stags, mixers, channels, d_bits, bits_stride,
                                                         lead.rows.d, stride, n_bits, flush, stream)
                   : srcdsp_modulate_step_batched(maps, ups, mixers, channels, d_bits, bits_stride, lead.rows.d, stride,
                                                  n_bits, flush, stream);
    if (!rc) rc = srcdsp_combine_step(lead.rows.d, stride, (size_t)channels, d_out, n_out, shift, stream);
    if (!rc) rc = lead.order.after((hipStream_t)stream);
    return rc;
}

}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_modulate_sum_step(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                        const srcdsp_stagger_t *staggers, const srcdsp_mixer_t *mixers, int channels,
                                        const void *d_bits, size_t bits_stride, void *d_out, size_t n_out,
                                        size_t n_bits, int flush, unsigned shift, void *stream) {
    const char *who = "modulate_sum_step";
    SRCDSP_ARG_CHECK(mappers != nullptr && ups != nullptr && mixers != nullptr && channels >= 1,
                     "modulate_sum_step: no handles");
    SRCDSP_ARG_CHECK(shift <= kCombineMaxShift, "modulate_sum_step: shift is 0..15");
    size_t n_sym = 0, want = 0;
    int rc = modulate_bank_check(mappers, ups, staggers, mixers, channels, n_bits, bits_stride, flush != 0, &n_sym,
                                 &want, who);
    if (rc) return rc;
    if (n_out != want) {
        set_error("modulate_sum_step: the output row holds exactly L*symbols samples (L*(symbols + length/L) when "
                  "flushing)");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_bits || n_bits == 0), "modulate_sum_step: null buffer");
    const srcdsp_up_state &u0 = ups[0]->u;
    const long n_total = (long)(n_out / u0.L);
    const SumRoute route = modsum_route(u0.L);
    if (fused_takes(u0, mixers[0]->m, staggers, channels, d_bits, bits_stride, d_out) && route.min_tiles > 0 &&
        up_tiles(n_total) >= route.min_tiles && channels <= route.max_channels) {
        rc = sum_fused(mappers, ups, staggers, mixers, channels, d_bits, bits_stride, d_out, n_bits, n_sym, n_total,
                       shift, (hipStream_t)stream);
        if (rc == SRCDSP_OK) g_fused_calls.hit();
        return rc;
    }
    rc = sum_bank(mappers, ups, staggers, mixers, channels, d_bits, bits_stride, d_out, n_out, n_bits, flush != 0, shift,
                  stream);
    if (rc == SRCDSP_OK) g_bank_calls.hit();
    return rc;
}

SRCDSP_API int srcdsp_modulate_sum_stats(unsigned long *fused_calls, unsigned long *bank_calls) {
    g_fused_calls.read(fused_calls);
    g_bank_calls.read(bank_calls);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_modulate_sum_geometry(unsigned L, int *tile_symbols, long *min_tiles, int *max_channels) {
    const SumRoute route = modsum_route(L);
    if (tile_symbols) *tile_symbols = kUpTile;
    if (min_tiles) *min_tiles = route.min_tiles;
    if (max_channels) *max_channels = route.max_channels;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_modulate_sum_set_min_tiles(long min_tiles) {
    SRCDSP_ARG_CHECK(min_tiles >= 0, "modulate_sum_set_min_tiles: min_tiles is >= 1, or 0 for the measured routing");
    g_min_tiles.store(min_tiles, std::memory_order_relaxed);
    return SRCDSP_OK;
}

}  // extern "C"
