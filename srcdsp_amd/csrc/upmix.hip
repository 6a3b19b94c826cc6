// upmix.hip -- FilterUpsamplingFir -> Mixer in one pass (the transmit chain:
// interpolate at baseband, shift to the carrier; upsampling_filters.h:149-233
// then mixers.h:169-188), single (srcdsp_upmix_step) and as a bank of C chains
// in one launch (srcdsp_upmix_step_batched).
//
// Every output is limitScale16(limitScale<complex<int16_t>>(y, shift) * lo, 14):
// the interpolator's asymmetric int16 clamp first (dsp_complex.h:83-108), the
// intermediate rounded to int16, then the mixer's product and symmetric clamp
// (dsp_complex.cpp:31-37, 63-73).  The kernel is the interpolator's v_dot2 tile
// (up_dot2_kernels.h) with the mixer in its epilogue: where the tile packs an
// output word, the word is mixed before it goes to the staged output tile.  A
// lane holds the 8 L consecutive outputs of its 8 inputs: its first phase is
// the closed form (phi + w freq) mod N of its first output w, the later ones
// add freq and subtract N conditionally.  The N-entry int16 table (any N <=
// 4096) is staged per workgroup behind the planes / output tile.
//
// Dispatch.  The fused kernel takes what up_tile_dot2 takes (variant 0 with
// int16-range taps, L = 2..8, taps <= 4096, 16-byte aligned input and output)
// with a mixer of N <= 4096; the bank also needs 16-byte aligned row strides.
// Every other legal shape runs the two operators inside the call: the
// interpolator into d_out, the mixer in place on d_out (it is element-wise);
// the bank then loops over its channels.  Either way outputs and both handles'
// state are those of the two calls, bit for bit.
#include <algorithm>

#include "ops.h"

#include "upmix_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_fused_calls, g_pair_calls, g_bank_calls, g_loop_calls;

template <int LR, int PPC>
__global__ __launch_bounds__(kUpBlockD) void upmix_tile_dot2(const UpmixLaunch P) {
    extern __shared__ uint4 ug[];
    const int c = blockIdx.y;
    int16_t *tab = (int16_t *)((char *)ug + P.tab_off);
    // visible to the epilogue through the tile's own barriers
    const unsigned nv = P.N / 8;
    for (unsigned i = threadIdx.x; i < nv; i += kUpBlockD) ((uint4 *)tab)[i] = ((const uint4 *)P.table)[i];
    for (unsigned i = 8 * nv + threadIdx.x; i < P.N; i += kUpBlockD) tab[i] = P.table[i];
    const uint32_t mw = P.mix[c];
    UpMixEpilogue epi;
    epi.tab = tab;
    epi.N = P.N;
    epi.freq = mw >> 16;
    epi.phi_tile = phase_at((unsigned long)LR * kUpRD * kUpBlockD * blockIdx.x, mw & 0xffffu, epi.freq, P.N);
    up_dot2_tile<LR, true, 3, PPC>(UpWordsIn{P.in + c * P.in_stride}, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c],
                                   P.pairs, P.H, P.shift, P.out + c * P.out_stride, epi);
}

// nc <= kMaxBatch chains in one launch; the shape is one upmix_fused_takes accepts
int fused_launch(const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc, const void *d_in, size_t in_stride,
                 void *d_out, size_t out_stride, size_t n_in, long n_total, bool iter, hipStream_t s) {
    srcdsp_up_state &u0 = ups[0]->u;
    UpmixLaunch P{};
    P.in = (const uint32_t *)d_in;
    P.out = (uint32_t *)d_out;
    P.pairs = u0.d_pair;
    P.table = mixers[0]->m.d_table;
    P.n_in = (long)n_in;
    P.n_total = n_total;
    P.in_stride = (long)in_stride;
    P.out_stride = (long)out_stride;
    P.H = u0.H;
    P.shift = iter ? 0u : (unsigned)(15 - u0.left_shift_factor);
    P.N = mixers[0]->m.N;
    const size_t tile_lds = up_dot2_smem(u0.H, u0.L);
    P.tab_off = (unsigned)tile_lds;
    const size_t smem = tile_lds + ((2 * (size_t)P.N + 15) & ~(size_t)15);
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        int rc = chan_begin(ups[c]->u, s, P.hist_in[c], P.hist_out[c]);
        if (!rc) rc = m.order.before(s);
        if (rc) return rc;
        P.mix[c] = m.word();
    }
    constexpr int TI = kUpRD * kUpBlockD;
    const int PP = (u0.H + 1) / 2;
    const dim3 grid((unsigned)((n_total + TI - 1) / TI), (unsigned)nc);
#define SRCDSP_UPMIX(LR, PPV) hipLaunchKernelGGL((upmix_tile_dot2<LR, PPV>), grid, dim3(kUpBlockD), smem, s, P)
    // the compile-time shapes of up_tile_dot2: 16, 32 or 64 taps per phase
#define SRCDSP_UPMIX_PP(LR, PPV)      \
    if (u0.L == LR && PP == PPV) {    \
        SRCDSP_UPMIX(LR, PPV);        \
    } else
    SRCDSP_UPMIX_PP(2, 8)
    SRCDSP_UPMIX_PP(2, 16)
    SRCDSP_UPMIX_PP(2, 32)
    SRCDSP_UPMIX_PP(4, 8)
    SRCDSP_UPMIX_PP(4, 16)
    SRCDSP_UPMIX_PP(4, 32)
    SRCDSP_UPMIX_PP(8, 8)
    SRCDSP_UPMIX_PP(8, 16)
#undef SRCDSP_UPMIX_PP
    switch (u0.L) {
    case 2: SRCDSP_UPMIX(2, 0); break;
    case 3: SRCDSP_UPMIX(3, 0); break;
    case 4: SRCDSP_UPMIX(4, 0); break;
    case 5: SRCDSP_UPMIX(5, 0); break;
    case 6: SRCDSP_UPMIX(6, 0); break;
    case 7: SRCDSP_UPMIX(7, 0); break;
    default: SRCDSP_UPMIX(8, 0); break;
    }
#undef SRCDSP_UPMIX
    SRCDSP_HIP_TRY(hipGetLastError());
    const unsigned long n_out = (unsigned long)u0.L * (unsigned long)n_total;
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        m.advance(n_out);
        int rc = chan_commit(ups[c]->u, s);
        if (!rc) rc = m.order.after(s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

// one chain; *fused tells which path served it (untouched when nothing ran)
int upmix_one(srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_in, size_t n_in, void *d_out, size_t n_out,
              bool flush, bool iter, void *stream, bool *fused) {
    srcdsp_up_state &u = up->u;
    if (u.variant == UV_I16_I32) {
        set_error("upmix_step: a real int16_t interpolator cannot feed the mixer (complex<int16_t> input)");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    const size_t extra = flush ? u.length / u.L : 0;
    // exactly the interpolator's output, also when flushing: the mixer steps
    // over every sample of the buffer (mixers.h:169-188)
    if (n_out != (size_t)u.L * (n_in + extra)) {
        set_error("upmix_step: output must hold exactly L*n_in samples (L*(n_in + length/L) when flushing)");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_in || n_in == 0), "upmix_step: null buffer");
    if (upmix_fused_takes(u, mixer->m, d_in, d_out)) {
        *fused = true;
        return fused_launch(&up, &mixer, 1, d_in, 0, d_out, 0, n_in, (long)(n_in + extra), iter, (hipStream_t)stream);
    }
    *fused = false;
    int rc = srcdsp_up_step(up, d_in, n_in, d_out, n_out, flush, iter, stream);
    if (rc == SRCDSP_OK) rc = srcdsp_mixer_step(mixer, d_out, n_out, d_out, stream);
    return rc;
}
}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_upmix_step(srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_in, size_t n_in, void *d_out,
                                 size_t n_out, int flush, int iterator, void *stream) {
    SRCDSP_ARG_CHECK(up != nullptr && mixer != nullptr, "upmix_step: null handle");
    const bool ran = n_out != 0;
    bool fused = false;
    int rc = upmix_one(up, mixer, d_in, n_in, d_out, n_out, flush != 0, iterator != 0, stream, &fused);
    if (rc == SRCDSP_OK && ran) (fused ? g_fused_calls : g_pair_calls).hit();
    return rc;
}

SRCDSP_API int srcdsp_upmix_step_batched(const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int channels,
                                         const void *d_in, size_t in_stride, void *d_out, size_t out_stride,
                                         size_t n_in, int flush, void *stream) {
    SRCDSP_ARG_CHECK(ups != nullptr && mixers != nullptr && channels >= 1, "upmix_step_batched: no handles");
    int rc = check_handles(ups, channels, "upmix_step_batched");
    if (!rc) rc = check_handles(mixers, channels, "upmix_step_batched");
    if (rc) return rc;
    const srcdsp_up_state &u0 = ups[0]->u;
    const MixerState &m0 = mixers[0]->m;
    if (u0.variant == UV_I16_I32) {
        set_error("upmix_step_batched: a real int16_t interpolator cannot feed the mixer (complex<int16_t> input)");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    for (int c = 1; c < channels; ++c) {
        const srcdsp_up_state &uc = ups[c]->u;
        SRCDSP_ARG_CHECK(uc.variant == u0.variant && uc.L == u0.L && uc.h_raw == u0.h_raw,
                         "upmix_step_batched: interpolators must share variant, L and taps");
        SRCDSP_ARG_CHECK(mixers[c]->m.N == m0.N, "upmix_step_batched: mixers must share N");
    }
    const size_t extra = flush ? u0.length / u0.L : 0;
    const size_t n_out = (size_t)u0.L * (n_in + extra);
    SRCDSP_ARG_CHECK(in_stride == 0 || in_stride >= n_in, "upmix_step_batched: in_stride must be 0 (shared) or >= n_in");
    if (out_stride < n_out) {
        set_error("upmix_step_batched: out_stride must hold a row of L*(n_in + length/L when flushing) samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_in || n_in == 0), "upmix_step_batched: null buffer");
    if (!(upmix_fused_takes(u0, m0, d_in, d_out) && (in_stride * 4) % 16 == 0 && (out_stride * 4) % 16 == 0)) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c) {
            bool fused;
            rc = upmix_one(ups[c], mixers[c], chan_row(d_in, c, in_stride), n_in, chan_row(d_out, c, out_stride), n_out,
                           flush != 0, false, stream, &fused);
        }
        return rc;
    }
    g_bank_calls.hit();
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = fused_launch(ups + c0, mixers + c0, std::min(kMaxBatch, channels - c0), chan_row(d_in, c0, in_stride),
                          in_stride, chan_row(d_out, c0, out_stride), out_stride, n_in, (long)(n_in + extra), false,
                          (hipStream_t)stream);
    return rc;
}

SRCDSP_API int srcdsp_upmix_stats(unsigned long *fused_calls, unsigned long *pair_calls, unsigned long *bank_calls,
                                  unsigned long *loop_calls) {
    g_fused_calls.read(fused_calls);
    g_pair_calls.read(pair_calls);
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
