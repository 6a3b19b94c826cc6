// modulate.hip -- SymbolMapper{Sdpsk,Qpsk} -> FilterUpsamplingFir -> Mixer in
// one call (the transmit chain from bits: modulators.h:103-117 / :169-184,
// upsampling_filters.h:149-233, mixers.h:169-188), single
// (srcdsp_modulate_step) and as a bank of C chains (srcdsp_modulate_step_batched).
//
// The kernel is the interpolator's v_dot2 tile (up_dot2_kernels.h) with the
// mixer in its epilogue (UpMixEpilogue, upmix_kernels.h) and its input staging
// fed from bits instead of a symbol buffer (the tile's SRC policy):
//   QPSK   a symbol is a pure function of two bytes: the staging reads the
//          bits themselves, 10 bytes for its 5 samples;
//   SDPSK  a symbol needs the state, a scan over the whole stream.  The
//          mapper's own launches (tile parities, their scan, the streaming
//          kernel; mapper.hip) run first on the same stream and leave the
//          states packed 2 bits each, n/4 bytes, which the staging reads back
//          as a pure lookup.  No workgroup waits on another.
// Samples before the call come from the interpolator's history, which holds
// symbols either way.
//
// Dispatch.  The fused kernel takes what upmix_tile_dot2 takes, with d_bits
// 16-byte aligned (and, in the bank, row strides that are multiples of 16
// bytes).  Every other legal shape runs srcdsp_mapper_step into scratch and
// srcdsp_upmix_step from it inside the call; the bank then loops over its
// channels.  Either way outputs and all three handles' state are those of the
// three calls, bit for bit.
#include <algorithm>

#include "modulate_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_fused_calls, g_chain_calls, g_bank_calls, g_loop_calls;

template <int LR, int PPC>
__global__ __launch_bounds__(kUpBlockD) void modulate_tile_dot2(const ModLaunch Q) {
    extern __shared__ uint4 ug[];
    const UpmixLaunch &P = Q.up;
    const int c = blockIdx.y;
    UpMixEpilogue epi;
    upmix_stage_table(epi, P, ug);
    upmix_aim<LR>(epi, P, c);
    const UpBitsIn src = mod_bits_row(Q, c);
    up_dot2_tile<LR, true, 3, PPC>(src, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c], P.pairs, P.H, P.shift,
                                   P.out + c * P.out_stride, epi);
}

bool fused_takes(const srcdsp_up_state &u, const MixerState &m, const void *d_bits, const void *d_out) {
    return upmix_fused_takes(u, m, d_bits, d_out);
}

// nc <= kMaxBatch chains in one launch of the tile (SDPSK: after the mapper's
// launches); the shape is one fused_takes accepts
int fused_launch(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc,
                 const void *d_bits, size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits, size_t n_sym,
                 long n_total, bool iter, hipStream_t s) {
    const srcdsp_up_state &u0 = ups[0]->u;
    ModLaunch Q{};
    size_t smem = 0;
    int rc = mod_launch_begin(Q, maps, ups, mixers, nc, d_bits, bits_stride, d_out, out_stride, n_bits, n_sym, n_total,
                              iter, s, &smem, upmix_no_more);
    if (rc) return rc;
    const dim3 grid((unsigned)up_tiles(n_total), (unsigned)nc);
    const bool served = up_dot2_dispatch<UpDot2Standard>(u0.L, (u0.H + 1) / 2, [&](auto lr, auto ppc) {
        hipLaunchKernelGGL((modulate_tile_dot2<decltype(lr)::value, decltype(ppc)::value>), grid, dim3(kUpBlockD), smem,
                           s, Q);
    });
    rc = up_dot2_launched(served);
    if (rc) return rc;
    return mod_launch_commit(maps, ups, mixers, nc, n_bits, n_total, s, upmix_no_more);
}

// one checked chain of n_out > 0; *fused tells which path served it
int modulate_one(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_bits, size_t n_bits,
                 size_t n_sym, void *d_out, size_t n_out, bool flush, bool iter, void *stream, bool *fused) {
    srcdsp_up_state &u = up->u;
    if (fused_takes(u, mixer->m, d_bits, d_out)) {
        *fused = true;
        return fused_launch(&mapper, &up, &mixer, 1, d_bits, 0, d_out, 0, n_bits, n_sym,
                            (long)(n_out / u.L), iter, (hipStream_t)stream);
    }
    *fused = false;
    MapperState &mp = mapper->m;
    int rc = mp.touch();  // the symbols are the mapper's scratch: its event orders their reuse
    if (!rc) rc = mp.sym.reserve(4 * std::max<size_t>(n_sym, 1));
    if (!rc && n_bits) rc = srcdsp_mapper_step(mapper, d_bits, n_bits, mp.sym.d, n_sym, stream);
    if (!rc) rc = srcdsp_upmix_step(up, mixer, mp.sym.d, n_sym, d_out, n_out, flush, iter, stream);
    if (!rc) rc = mp.order.after((hipStream_t)stream);
    return rc;
}

}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_modulate_step(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_bits,
                                    size_t n_bits, void *d_out, size_t n_out, int flush, int iterator, void *stream) {
    SRCDSP_ARG_CHECK(mapper != nullptr && up != nullptr && mixer != nullptr, "modulate_step: null handle");
    size_t n_sym = 0, want = 0;
    int rc = modulate_check(mapper->m, up->u, n_bits, &n_sym, &want, flush != 0, "modulate_step");
    if (rc) return rc;
    if (n_out != want) {
        set_error("modulate_step: output must hold exactly L*symbols samples (L*(symbols + length/L) when flushing)");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_bits || n_bits == 0), "modulate_step: null buffer");
    bool fused = false;
    rc = modulate_one(mapper, up, mixer, d_bits, n_bits, n_sym, d_out, n_out, flush != 0, iterator != 0, stream, &fused);
    if (rc == SRCDSP_OK) (fused ? g_fused_calls : g_chain_calls).hit();
    return rc;
}

SRCDSP_API int srcdsp_modulate_step_batched(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                            const srcdsp_mixer_t *mixers, int channels, const void *d_bits,
                                            size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits,
                                            int flush, void *stream) {
    SRCDSP_ARG_CHECK(mappers != nullptr && ups != nullptr && mixers != nullptr && channels >= 1,
                     "modulate_step_batched: no handles");
    int rc = check_handles(mappers, channels, "modulate_step_batched");
    if (!rc) rc = check_handles(ups, channels, "modulate_step_batched");
    if (!rc) rc = check_handles(mixers, channels, "modulate_step_batched");
    if (rc) return rc;
    const srcdsp_up_state &u0 = ups[0]->u;
    const MixerState &m0 = mixers[0]->m;
    size_t n_sym = 0, n_out = 0;
    rc = modulate_check(mappers[0]->m, u0, n_bits, &n_sym, &n_out, flush != 0, "modulate_step_batched");
    if (rc) return rc;
    for (int c = 1; c < channels; ++c) {
        const srcdsp_up_state &uc = ups[c]->u;
        SRCDSP_ARG_CHECK(mappers[c]->m.kind == mappers[0]->m.kind, "modulate_step_batched: mappers must share a kind");
        SRCDSP_ARG_CHECK(uc.variant == u0.variant && uc.L == u0.L && uc.h_raw == u0.h_raw,
                         "modulate_step_batched: interpolators must share variant, L and taps");
        SRCDSP_ARG_CHECK(mixers[c]->m.N == m0.N, "modulate_step_batched: mixers must share N");
    }
    SRCDSP_ARG_CHECK(bits_stride == 0 || bits_stride >= n_bits,
                     "modulate_step_batched: bits_stride must be 0 (shared) or >= n_bits");
    if (out_stride < n_out) {
        set_error("modulate_step_batched: out_stride must hold a row of L*(symbols + length/L when flushing) samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_bits || n_bits == 0), "modulate_step_batched: null buffer");
    if (!(fused_takes(u0, m0, d_bits, d_out) && bits_stride % 16 == 0 && (out_stride * 4) % 16 == 0)) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c) {
            bool fused;
            rc = modulate_one(mappers[c], ups[c], mixers[c], chan_row(d_bits, c, bits_stride, 1), n_bits, n_sym,
                              chan_row(d_out, c, out_stride), n_out, flush != 0, false, stream, &fused);
        }
        return rc;
    }
    g_bank_calls.hit();
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = fused_launch(mappers + c0, ups + c0, mixers + c0, std::min(kMaxBatch, channels - c0),
                          chan_row(d_bits, c0, bits_stride, 1), bits_stride, chan_row(d_out, c0, out_stride), out_stride,
                          n_bits, n_sym, (long)(n_out / u0.L), false, (hipStream_t)stream);
    return rc;
}

SRCDSP_API int srcdsp_modulate_stats(unsigned long *fused_calls, unsigned long *chain_calls, unsigned long *bank_calls,
                                     unsigned long *loop_calls) {
    g_fused_calls.read(fused_calls);
    g_chain_calls.read(chain_calls);
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
