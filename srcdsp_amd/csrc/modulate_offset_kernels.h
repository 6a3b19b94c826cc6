// modulate_offset_kernels.h -- what the offset modulator bank
// (modulate_offset.hip) and the summing modulator bank (modulate_sum.hip)
// share: the tile's stagger policy, the launch description, the size and
// sharing rules of a bank call, and the stagger layer of the two halves of a
// bank launch on either side of the kernel (every handle's begin, every
// handle's commit; the layers below are in modulate_kernels.h and
// upmix_kernels.h).
#pragma once
#include <string>

#include "modulate_kernels.h"
#include "stagger_state.h"

namespace srcdsp {

// the tile's stagger policy (STG of up_dot2_tile).  DT: int, or an
// std::integral_constant<int, d> where the delay is known at compile time (the
// tile then holds the one emit loop of that delay)
template <class DT>
struct UpQStaggerOf {
    static constexpr bool on = true;
    DT D;                     // 1..LR
    const int16_t *carry_in;  // D values: the imaginary halves of the call's first D outputs
    int16_t *carry_out;
    uint16_t *slot;           // 8 values in LDS: the halves ahead of the tile's first word, the last D used

    // lanes t < D, while the planes still hold the tile's input: value t of the
    // D ahead of the tile, and of the D that end the call (its last tile only).
    // tile_q(jr, o): clamped imaginary output of phase o of staged sample jr;
    // halo: the staged index of the tile's first sample
    template <int LR, class F>
    __device__ __forceinline__ void seed(int t, long j0, long n_total, int halo, F &tile_q) const {
        if (t >= D) return;
        const int o = LR - D + t;
        slot[8 - D + t] = j0 == 0 ? (uint16_t)carry_in[t] : (uint16_t)tile_q(halo - 1, o);
        const long jl = n_total - 1 - j0;
        if (jl < kUpTile) carry_out[t] = (int16_t)(uint16_t)tile_q(halo + (int)jl, o);
    }
    __device__ __forceinline__ uint4 seeds() const { return *(const uint4 *)slot; }
};
typedef UpQStaggerOf<int> UpQStagger;

struct ModOffLaunch {
    ModLaunch mod;
    int D;
    unsigned slot_off;  // byte offset of the seed slot in dynamic LDS
    const int16_t *carry_in[kMaxBatch];
    int16_t *carry_out[kMaxBatch];
};

// Every rule of a bank call of `channels` chains that shares a kind, a
// variant, L, taps, D and N, before anything changes: the handle lists, the
// chain's own sizes (modulate_check: *n_sym symbols and a row of *n_out
// samples) and bits_stride.  staggers == nullptr: chains without a stagger.
inline int modulate_bank_check(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups, const srcdsp_stagger_t *staggers,
                               const srcdsp_mixer_t *mixers, int channels, size_t n_bits, size_t bits_stride,
                               bool flush, size_t *n_sym, size_t *n_out, const char *who) {
    const std::string w(who);
    int rc = check_handles(mappers, channels, who);
    if (!rc) rc = check_handles(ups, channels, who);
    if (!rc && staggers) rc = check_handles(staggers, channels, who);
    if (!rc) rc = check_handles(mixers, channels, who);
    if (rc) return rc;
    const srcdsp_up_state &u0 = ups[0]->u;
    rc = modulate_check(mappers[0]->m, u0, n_bits, n_sym, n_out, flush, who);
    if (rc) return rc;
    for (int c = 1; c < channels; ++c) {
        const srcdsp_up_state &uc = ups[c]->u;
        SRCDSP_ARG_CHECK(mappers[c]->m.kind == mappers[0]->m.kind, w + ": mappers must share a kind");
        SRCDSP_ARG_CHECK(uc.variant == u0.variant && uc.L == u0.L && uc.h_raw == u0.h_raw,
                         w + ": interpolators must share variant, L and taps");
        SRCDSP_ARG_CHECK(!staggers || staggers[c]->g.D == staggers[0]->g.D, w + ": staggers must share D");
        SRCDSP_ARG_CHECK(mixers[c]->m.N == mixers[0]->m.N, w + ": mixers must share N");
    }
    SRCDSP_ARG_CHECK(bits_stride == 0 || bits_stride >= n_bits, w + ": bits_stride must be 0 (shared) or >= n_bits");
    return SRCDSP_OK;
}

// The stagger layer of a bank launch's two halves, on mod_launch_begin /
// mod_launch_commit (modulate_kernels.h), for nc <= kMaxBatch chains of a shape
// the tile takes.  Ahead of the kernel: the layers below with every stagger's
// begin, and the seed slot behind the mixer's table.  *smem: the dynamic LDS of
// the launch.  stags == nullptr: no stagger (A.D = 0, no carry).
inline int modoff_launch_begin(ModOffLaunch &A, const srcdsp_mapper_t *maps, const srcdsp_up_t *ups,
                               const srcdsp_stagger_t *stags, const srcdsp_mixer_t *mixers, int nc, const void *d_bits,
                               size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits, size_t n_sym,
                               long n_total, bool iter, hipStream_t s, size_t *smem) {
    A.D = stags ? (int)stags[0]->g.D : 0;
    int rc = mod_launch_begin(A.mod, maps, ups, mixers, nc, d_bits, bits_stride, d_out, out_stride, n_bits, n_sym,
                              n_total, iter, s, smem, [&](int c) {
                                  return stags ? stagger_begin(stags[c]->g, s, A.carry_in[c], A.carry_out[c]) : SRCDSP_OK;
                              });
    A.slot_off = (unsigned)*smem;
    *smem = A.slot_off + 16;
    return rc;
}

// Behind the kernel: the layers below with every stagger's commit
inline int modoff_launch_commit(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_stagger_t *stags,
                                const srcdsp_mixer_t *mixers, int nc, size_t n_bits, long n_total, hipStream_t s) {
    return mod_launch_commit(maps, ups, mixers, nc, n_bits, n_total, s,
                             [&](int c) { return stags ? stagger_commit(stags[c]->g, s) : SRCDSP_OK; });
}

}  // namespace srcdsp
