// ddc_bank.hip -- srcdsp_mixdecim_step_batched: C mixer -> decimator chains in
// one call (a digital down-converter bank: one wideband input or one input per
// channel, C local oscillators, one shared channel filter).
//
// Dispatch.  The bank kernel (ddc_bank_kernels.h) takes: variant 1
// (complex<int16_t>, int32 taps all in int16 range), M = 4, 1..1024 taps, a
// mixer table of N = 2^k <= 4096 entries, a 16-byte aligned input and input
// row stride (output rows need only their samples' 4-byte alignment: a row of
// n_in / 4 outputs is a multiple of 16 bytes only for some n_in), and
// n_in x taps <= 2^31 per channel (kBankMaxWork below: past it the loop's
// per-frequency register table wins).  Every other shape -- other M, taps
// beyond int16, variant 2, other N, misaligned input views, longer calls -- is
// the loop of srcdsp_mixdecim_step over the channels.
// Either way the outputs and every handle's state (mixer phase, decimator
// history) are those of that loop, bit for bit.
#include <algorithm>

#include "ops.h"

#include "ddc_bank_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_bank_calls, g_loop_calls;

// persistent grid: the resident capacity (256 CUs x 4 workgroups) twice over
constexpr long kBankGridCap = 2048;

// The bank kernel's one general mixer table costs ~12 VALU operations per
// sample and channel where the single-channel kernel's per-frequency register
// table costs ~3, so once a call is long enough to hide the loop's launches
// behind its kernels and the tap loop is VALU-bound, the loop is faster.
// Measured on MI355X (8 channels, bank / loop time per step): n_in x taps =
// 2.1e9: 0.91 (31 taps, 2^26 samples), 0.96 (127 taps, 2^24); 4.3e9: 1.07
// (63 taps, 2^26), 1.005 (255 taps, 2^24), 1.05 (1024 taps, 2^22); 8.5e9: 1.25
// (127 taps, 2^26).  Below the bound the bank is 0.33-0.84 of the loop.
constexpr unsigned long kBankMaxWork = 1ul << 31;  // n_in x taps per channel

bool bank_takes(const FirCore &f, const MixerState &m, const void *d_in, size_t in_stride, size_t n_in) {
    return f.kv == KV_CI16_I32 && f.M == 4 && f.coef_fits_i16 && f.ntaps >= 1 && f.ntaps <= kDot2MaxTaps &&
           m.N >= 4 && m.N <= (unsigned)kBankMaxN && (m.N & (m.N - 1)) == 0 && aligned16(d_in) &&
           (in_stride * 4) % 16 == 0 && n_in <= kBankMaxWork / (unsigned long)f.ntaps;
}

int bank_launch(const srcdsp_mixer_t *mixers, const srcdsp_decim_t *decims, int nc, const void *d_in, size_t in_stride,
                void *d_out, size_t out_stride, size_t n_in, hipStream_t s) {
    FirCore &f0 = decims[0]->core;
    BankLaunch L{};
    L.in = d_in;
    L.out = d_out;
    L.cpair = f0.d_cpair;
    L.table = mixers[0]->m.d_table;  // one table for all: built from N alone (mixers.h:155-158)
    L.n_in = (long)n_in;
    L.n_out = (long)(n_in / 4);
    L.in_stride = (long)in_stride;
    L.out_stride = (long)out_stride;
    L.ntiles = (L.n_out + kBankTO - 1) / kBankTO;
    L.ntaps = f0.ntaps;
    L.shift = f0.shift();
    L.N = mixers[0]->m.N;
    L.channels = nc;
    // a shared input: a workgroup serves a group of channels from one fetch of
    // the tile; the group shrinks while the grid would not fill the device
    const long grid_cap = stream_grid_cap(kBankGridCap);
    int group = 1;
    if (in_stride == 0) {
        group = std::min(kBankGroup, nc);
        while (group > 1 && L.ntiles * ((nc + group - 1) / group) < grid_cap / 2) group = (group + 1) / 2;
    }
    L.group = group;
    const int ngroups = (nc + group - 1) / group;
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        int rc = m.order.before(s);
        if (!rc) rc = chan_begin(decims[c]->core, s, L.hist_in[c], L.hist_out[c]);
        if (rc) return rc;
        L.mix[c] = m.word();
    }
    dim3 grid(persistent_grid(L.ntiles, std::max<long>(1, grid_cap / ngroups)), (unsigned)ngroups);
    hipLaunchKernelGGL(ddc_bank_ci16, grid, dim3(kBankBlock), 0, s, L);
    SRCDSP_HIP_TRY(hipGetLastError());
    for (int c = 0; c < nc; ++c) {
        MixerState &m = mixers[c]->m;
        m.advance(n_in);
        int rc = m.order.after(s);
        if (!rc) rc = chan_commit(decims[c]->core, s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}
}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_mixdecim_step_batched(const srcdsp_mixer_t *mixers, const srcdsp_decim_t *decims, int channels,
                                            const void *d_in, size_t in_stride, void *d_out, size_t out_stride,
                                            size_t n_in, void *stream) {
    SRCDSP_ARG_CHECK(mixers != nullptr && decims != nullptr && channels >= 1, "mixdecim_step_batched: no handles");
    int rc = check_handles(mixers, channels, "mixdecim_step_batched");
    if (!rc) rc = check_handles(decims, channels, "mixdecim_step_batched");
    if (rc) return rc;
    const FirCore &f0 = decims[0]->core;
    const MixerState &m0 = mixers[0]->m;
    if (f0.kv != KV_CI16_I32 && f0.kv != KV_CI16_I16) {
        set_error("mixdecim_step_batched: the decimators must take complex<int16_t> input (the mixer's output)");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    for (int c = 1; c < channels; ++c) {
        const FirCore &fc = decims[c]->core;
        SRCDSP_ARG_CHECK(fc.kv == f0.kv && fc.M == f0.M && fc.ntaps == f0.ntaps && fc.flags == f0.flags &&
                             fc.shift() == f0.shift() && fc.h_coef == f0.h_coef,
                         "mixdecim_step_batched: decimators must share variant, M, taps, flags and shift");
        SRCDSP_ARG_CHECK(mixers[c]->m.N == m0.N, "mixdecim_step_batched: mixers must share N");
    }
    SRCDSP_ARG_CHECK(n_in % f0.M == 0, "mixdecim_step_batched: n_in must be a multiple of M");
    if (n_in == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in && d_out, "mixdecim_step_batched: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (!bank_takes(f0, m0, d_in, in_stride, n_in)) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c)
            rc = srcdsp_mixdecim_step(mixers[c], decims[c], chan_row(d_in, c, in_stride), n_in,
                                      chan_row(d_out, c, out_stride), n_in / f0.M, stream);
        return rc;
    }
    g_bank_calls.hit();
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = bank_launch(mixers + c0, decims + c0, std::min(kMaxBatch, channels - c0), chan_row(d_in, c0, in_stride),
                         in_stride, chan_row(d_out, c0, out_stride), out_stride, n_in, s);
    return rc;
}

SRCDSP_API int srcdsp_mixdecim_batched_stats(unsigned long *bank_calls, unsigned long *loop_calls) {
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
