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
    UpMixEpilogue epi;
    upmix_stage_table(epi, P, ug);
    upmix_aim<LR>(epi, P, c);
    up_dot2_tile<LR, true, 3, PPC>(UpWordsIn{P.in + c * P.in_stride}, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c],
                                   P.pairs, P.H, P.shift, P.out + c * P.out_stride, epi);
}

// nc <= kMaxBatch chains in one launch; the shape is one upmix_fused_takes accepts
int fused_launch(const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc, const void *d_in, size_t in_stride,
                 void *d_out, size_t out_stride, size_t n_in, long n_total, bool iter, hipStream_t s) {
    const srcdsp_up_state &u0 = ups[0]->u;
    UpmixLaunch P{};
    P.in = (const uint32_t *)d_in;
    P.in_stride = (long)in_stride;
    size_t smem = 0;
    int rc = upmix_launch_begin(P, ups, mixers, nc, d_out, out_stride, n_in, n_total, iter, s, &smem, upmix_no_more);
    if (rc) return rc;
    const dim3 grid((unsigned)up_tiles(n_total), (unsigned)nc);
    const bool served = up_dot2_dispatch<UpDot2Standard>(u0.L, (u0.H + 1) / 2, [&](auto lr, auto ppc) {
        hipLaunchKernelGGL((upmix_tile_dot2<decltype(lr)::value, decltype(ppc)::value>), grid, dim3(kUpBlockD), smem, s,
                           P);
    });
    rc = up_dot2_launched(served);
    if (rc) return rc;
    return upmix_launch_commit(ups, mixers, nc, n_total, s, upmix_no_more);
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
