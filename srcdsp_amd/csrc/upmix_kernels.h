// upmix_kernels.h -- what the interpolator -> mixer kernel (upmix.hip) and the
// mapper -> interpolator -> mixer kernel (modulate.hip) share: the launch
// description, the mixer epilogue of the tile with its kernel prologue, the
// shapes the tile takes and the interpolator + mixer layer of a launch's begin
// and commit.
#pragma once
#include "ops.h"

#include "nco_device.h"
#include "up_dot2_kernels.h"

namespace srcdsp {

constexpr unsigned kUpmixMaxN = 4096;  // table entries staged in LDS (8 KiB)

struct UpmixLaunch {
    const uint32_t *in;
    uint32_t *out;
    const uint32_t *pairs;   // shared by all channels
    const int16_t *table;    // one table for all: built from N alone (mixers.h:155-158)
    long n_in, n_total;
    long in_stride, out_stride;  // samples, between channels (grid.y)
    int H;
    unsigned shift, N;
    unsigned tab_off;        // byte offset of the table in dynamic LDS
    const uint32_t *hist_in[kMaxBatch];
    uint32_t *hist_out[kMaxBatch];
    uint32_t mix[kMaxBatch];  // lo: phase, hi: frequency word
};

// the mixer on a lane's consecutive output words
struct UpMixEpilogue {
    const int16_t *tab;
    unsigned N, freq, phi_tile;  // phi_tile: phase of the tile's first output
    unsigned ph;
    __device__ __forceinline__ void begin(int k) { ph = (phi_tile + ((unsigned)k % N) * freq) % N; }
    __device__ __forceinline__ uint32_t operator()(uint32_t w) {
        const uint32_t y = nco_mix(w, tab, N, ph);
        ph += freq;
        ph = ph >= N ? ph - N : ph;
        return y;
    }
};

// The mixer's kernel prologue, once per workgroup: the table into dynamic LDS
// (`lds`: its start) behind the tile, visible to the epilogue through the
// tile's own barriers, and the epilogue's table and N
__device__ __forceinline__ void upmix_stage_table(UpMixEpilogue &epi, const UpmixLaunch &P, void *lds) {
    int16_t *tab = (int16_t *)((char *)lds + P.tab_off);
    const unsigned nv = P.N / 8;
    for (unsigned i = threadIdx.x; i < nv; i += kUpBlockD) ((uint4 *)tab)[i] = ((const uint4 *)P.table)[i];
    for (unsigned i = 8 * nv + threadIdx.x; i < P.N; i += kUpBlockD) tab[i] = P.table[i];
    epi.tab = tab;
    epi.N = P.N;
}

// the first output word of tile blockIdx.x
template <int LR>
__device__ __forceinline__ unsigned long upmix_tile_word() {
    return (unsigned long)LR * kUpTile * blockIdx.x;
}

// ... and per chain: the epilogue aimed at chain c's mixer in tile blockIdx.x.
// (A kernel that aims it in a loop over chains passes w0 = upmix_tile_word from
// outside the loop: taken inside it, the summing tile compiled to other code.)
template <int LR>
__device__ __forceinline__ void upmix_aim(UpMixEpilogue &epi, const UpmixLaunch &P, int c,
                                          unsigned long w0 = upmix_tile_word<LR>()) {
    const uint32_t mw = P.mix[c];
    epi.freq = mw >> 16;
    epi.phi_tile = phase_at(w0, mw & 0xffffu, epi.freq, P.N);
}

// the shapes the fused tile takes (d_in: the tile's input buffer)
inline bool upmix_fused_takes(const srcdsp_up_state &u, const MixerState &m, const void *d_in, const void *d_out) {
    return u.variant == UV_CI16_I32 && u.coef_i16 && u.L >= 2 && u.L <= 8 && u.ntaps <= kUpMaxTaps &&
           m.N <= kUpmixMaxN && aligned16(d_in) && aligned16(d_out);
}

// The two halves of a launch of nc <= kMaxBatch interpolator -> mixer chains
// on either side of the kernel, as layers: this one has the interpolators and
// the mixers, modulate_kernels.h puts the mappers on top and
// modulate_offset_kernels.h the staggers on top of those.  A layer passes
// `more(c)`, its own part of chain c, to the layer below, which runs it behind
// its own part of that chain: the begins and the commits record events, so a
// chain's calls keep one order, interpolator, mixer, stagger, mapper.
inline int upmix_no_more(int) { return SRCDSP_OK; }

// Ahead of the kernel: the launch description (in / in_stride aside: the
// caller's, where the input is a sample buffer) and every handle's begin.
// *smem: the tile and the mixer's table, the dynamic LDS of the launch.
template <class More>
int upmix_launch_begin(UpmixLaunch &P, const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc, void *d_out,
                       size_t out_stride, size_t n_in, long n_total, bool iter, hipStream_t s, size_t *smem,
                       More more) {
    srcdsp_up_state &u0 = ups[0]->u;
    P.out = (uint32_t *)d_out;
    P.pairs = u0.d_pair;
    P.table = mixers[0]->m.d_table;
    P.n_in = (long)n_in;
    P.n_total = n_total;
    P.out_stride = (long)out_stride;
    P.H = u0.H;
    P.shift = iter ? 0u : (unsigned)(15 - u0.left_shift_factor);
    P.N = mixers[0]->m.N;
    const size_t tile_lds = up_dot2_smem(u0.H, u0.L);
    P.tab_off = (unsigned)tile_lds;
    *smem = tile_lds + ((2 * (size_t)P.N + 15) & ~(size_t)15);
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        int rc = chan_begin(ups[c]->u, s, P.hist_in[c], P.hist_out[c]);
        if (!rc) rc = m.order.before(s);
        if (!rc) rc = more(c);
        if (rc) return rc;
        P.mix[c] = m.word();
    }
    return SRCDSP_OK;
}

// Behind the kernel: every mixer advanced by the row's samples and every
// handle's commit
template <class More>
int upmix_launch_commit(const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc, long n_total, hipStream_t s,
                        More more) {
    const unsigned long n_out = (unsigned long)ups[0]->u.L * (unsigned long)n_total;
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        m.advance(n_out);
        int rc = chan_commit(ups[c]->u, s);
        if (!rc) rc = m.order.after(s);
        if (!rc) rc = more(c);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

}  // namespace srcdsp
