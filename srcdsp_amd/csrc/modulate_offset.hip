// modulate_offset.hip -- SymbolMapper{Sdpsk,Qpsk} -> FilterUpsamplingFir ->
// Q-rail stagger -> Mixer in one call: the offset-QPSK transmit chain from
// bits (modulators.h:103-117 / :169-184, upsampling_filters.h:149-233, a delay
// of D samples on the imaginary rail, mixers.h:169-188), single
// (srcdsp_modulate_offset_step) and as a bank (srcdsp_modulate_offset_step_batched).
//
// The kernel is modulate.hip's tile with the tile's stagger policy switched on
// (up_dot2_kernels.h, STG): the delay acts on the clamped interpolator output,
// ahead of the mixer epilogue.  Of the two ways to give a later tile's first
// lane the D values before the tile, this one recomputes them from the halo
// the tile has staged anyway (D lanes, ceil(H/2) dot2 each), so the call stays
// one launch and no workgroup waits on another; a launch of its own that
// writes them per tile would read every tile's halo from memory a second
// time.  The Q rail has no tap table of its own.
//
// Dispatch.  The fused kernel takes what modulate_tile_dot2 takes with
// 1 <= D <= L.  Every other legal shape runs the four operators inside the
// call through grow-only scratch: srcdsp_mapper_step, srcdsp_up_step,
// srcdsp_stagger_step into d_out, srcdsp_mixer_step in place; the bank then
// loops over its channels.  Either way outputs and all four handles' state
// are those of the four calls, bit for bit.
#include <algorithm>

#include "modulate_offset_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_fused_calls, g_chain_calls, g_bank_calls, g_loop_calls;

template <int LR, int PPC>
__global__ __launch_bounds__(kUpBlockD) void modoffset_tile_dot2(const ModOffLaunch A) {
    extern __shared__ uint4 ug[];
    const ModLaunch &Q = A.mod;
    const UpmixLaunch &P = Q.up;
    const int c = blockIdx.y;
    UpMixEpilogue epi;
    upmix_stage_table(epi, P, ug);
    upmix_aim<LR>(epi, P, c);
    const UpBitsIn src = mod_bits_row(Q, c);
    const UpQStagger stg{A.D, A.carry_in[c], A.carry_out[c], (uint16_t *)((char *)ug + A.slot_off)};
    up_dot2_tile<LR, true, 3, PPC>(src, P.n_in, P.n_total, P.hist_in[c], P.hist_out[c], P.pairs, P.H, P.shift,
                                   P.out + c * P.out_stride, epi, stg);
}

bool fused_takes(const srcdsp_up_state &u, const MixerState &m, const StaggerState &g, const void *d_bits,
                 const void *d_out) {
    return upmix_fused_takes(u, m, d_bits, d_out) && g.D <= u.L;
}

// nc <= kMaxBatch chains in one launch of the tile (SDPSK: after the mapper's
// launches); the shape is one fused_takes accepts
int fused_launch(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_stagger_t *stags,
                 const srcdsp_mixer_t *mixers, int nc, const void *d_bits, size_t bits_stride, void *d_out,
                 size_t out_stride, size_t n_bits, size_t n_sym, long n_total, bool iter, hipStream_t s) {
    const srcdsp_up_state &u0 = ups[0]->u;
    ModOffLaunch A{};
    size_t smem = 0;
    int rc = modoff_launch_begin(A, maps, ups, stags, mixers, nc, d_bits, bits_stride, d_out, out_stride, n_bits, n_sym,
                                 n_total, iter, s, &smem);
    if (rc) return rc;
    const dim3 grid((unsigned)up_tiles(n_total), (unsigned)nc);
    const bool served = up_dot2_dispatch<UpDot2Standard>(u0.L, (u0.H + 1) / 2, [&](auto lr, auto ppc) {
        hipLaunchKernelGGL((modoffset_tile_dot2<decltype(lr)::value, decltype(ppc)::value>), grid, dim3(kUpBlockD), smem,
                           s, A);
    });
    rc = up_dot2_launched(served);
    if (rc) return rc;
    return modoff_launch_commit(maps, ups, stags, mixers, nc, n_bits, n_total, s);
}

// one checked chain of n_out > 0; *fused tells which path served it
int modoff_one(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_stagger_t stag, srcdsp_mixer_t mixer,
               const void *d_bits, size_t n_bits, size_t n_sym, void *d_out, size_t n_out, bool flush, bool iter,
               void *stream, bool *fused) {
    srcdsp_up_state &u = up->u;
    if (fused_takes(u, mixer->m, stag->g, d_bits, d_out)) {
        *fused = true;
        return fused_launch(&mapper, &up, &stag, &mixer, 1, d_bits, 0, d_out, 0, n_bits, n_sym, (long)(n_out / u.L),
                            iter, (hipStream_t)stream);
    }
    *fused = false;
    MapperState &mp = mapper->m;
    StaggerState &g = stag->g;
    // the symbols are the mapper's scratch, the interpolator's output the
    // stagger's: their events order the reuse
    int rc = mp.touch();
    if (!rc) rc = g.touch();
    if (!rc) rc = mp.order.before((hipStream_t)stream);
    if (!rc) rc = g.order.before((hipStream_t)stream);
    if (!rc) rc = mp.sym.reserve(4 * std::max<size_t>(n_sym, 1));
    if (!rc) rc = g.scratch.reserve(4 * n_out);
    if (!rc && n_bits) rc = srcdsp_mapper_step(mapper, d_bits, n_bits, mp.sym.d, n_sym, stream);
    if (!rc) rc = srcdsp_up_step(up, mp.sym.d, n_sym, g.scratch.d, n_out, flush, iter, stream);
    if (!rc) rc = srcdsp_stagger_step(stag, g.scratch.d, n_out, d_out, stream);
    if (!rc) rc = srcdsp_mixer_step(mixer, d_out, n_out, d_out, stream);
    if (!rc) rc = mp.order.after((hipStream_t)stream);
    if (!rc) rc = g.order.after((hipStream_t)stream);
    return rc;
}

}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_modulate_offset_step(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_stagger_t stagger,
                                           srcdsp_mixer_t mixer, const void *d_bits, size_t n_bits, void *d_out,
                                           size_t n_out, int flush, int iterator, void *stream) {
    SRCDSP_ARG_CHECK(mapper != nullptr && up != nullptr && stagger != nullptr && mixer != nullptr,
                     "modulate_offset_step: null handle");
    size_t n_sym = 0, want = 0;
    int rc = modulate_check(mapper->m, up->u, n_bits, &n_sym, &want, flush != 0, "modulate_offset_step");
    if (rc) return rc;
    if (n_out != want) {
        set_error("modulate_offset_step: output must hold exactly L*symbols samples (L*(symbols + length/L) when "
                  "flushing)");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_bits || n_bits == 0), "modulate_offset_step: null buffer");
    bool fused = false;
    rc = modoff_one(mapper, up, stagger, mixer, d_bits, n_bits, n_sym, d_out, n_out, flush != 0, iterator != 0, stream,
                    &fused);
    if (rc == SRCDSP_OK) (fused ? g_fused_calls : g_chain_calls).hit();
    return rc;
}

SRCDSP_API int srcdsp_modulate_offset_step_batched(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                                   const srcdsp_stagger_t *staggers, const srcdsp_mixer_t *mixers,
                                                   int channels, const void *d_bits, size_t bits_stride, void *d_out,
                                                   size_t out_stride, size_t n_bits, int flush, void *stream) {
    const char *who = "modulate_offset_step_batched";
    SRCDSP_ARG_CHECK(mappers != nullptr && ups != nullptr && staggers != nullptr && mixers != nullptr && channels >= 1,
                     "modulate_offset_step_batched: no handles");
    size_t n_sym = 0, n_out = 0;
    int rc = modulate_bank_check(mappers, ups, staggers, mixers, channels, n_bits, bits_stride, flush != 0, &n_sym,
                                 &n_out, who);
    if (rc) return rc;
    const srcdsp_up_state &u0 = ups[0]->u;
    const MixerState &m0 = mixers[0]->m;
    if (out_stride < n_out) {
        set_error("modulate_offset_step_batched: out_stride must hold a row of L*(symbols + length/L when flushing) "
                  "samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n_out == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_bits || n_bits == 0), "modulate_offset_step_batched: null buffer");
    if (!(fused_takes(u0, m0, staggers[0]->g, d_bits, d_out) && bits_stride % 16 == 0 && (out_stride * 4) % 16 == 0)) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c) {
            bool fused;
            rc = modoff_one(mappers[c], ups[c], staggers[c], mixers[c], chan_row(d_bits, c, bits_stride, 1), n_bits,
                            n_sym, chan_row(d_out, c, out_stride), n_out, flush != 0, false, stream, &fused);
        }
        return rc;
    }
    g_bank_calls.hit();
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = fused_launch(mappers + c0, ups + c0, staggers + c0, mixers + c0, std::min(kMaxBatch, channels - c0),
                          chan_row(d_bits, c0, bits_stride, 1), bits_stride, chan_row(d_out, c0, out_stride),
                          out_stride, n_bits, n_sym, (long)(n_out / u0.L), false, (hipStream_t)stream);
    return rc;
}

SRCDSP_API int srcdsp_modulate_offset_stats(unsigned long *fused_calls, unsigned long *chain_calls,
                                            unsigned long *bank_calls, unsigned long *loop_calls) {
    g_fused_calls.read(fused_calls);
    g_chain_calls.read(chain_calls);
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
