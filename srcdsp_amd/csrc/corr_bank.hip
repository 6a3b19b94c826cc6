// corr_bank.hip -- srcdsp_corr_step_batched: C FixedPatternCorrelators (shared
// N and S, own patterns) each scanned up to its own first detection in one
// call, on one input per channel or on one shared input.
//
// Dispatch.  The bank serves the shapes of the fused single-channel scan
// (corr_run's `fused`): S == 1, an int16-range pattern in every channel and
// NP <= kCorrDot2MaxTaps.  It is two launches for up to kMaxBatch channels,
//   corr_bank_s1     : corr_scan_s1's tile (corr_scan_kernels.h), grid row = channel;
//   corr_bank_finish : corr_tail (corr_tail.h), one workgroup per channel --
//                      the registers at the last processed sample, the new
//                      history, bitSamples and a final result row: the tail
//                      of srcdsp_corr_step itself,
// then one D2H copy of the result rows and, when some channel hit, one more of
// those channels' bitSamples rows: two host synchronisations at most, however
// many channels; corr_commit (corr_tail.h) puts each row into its handle.
// Every other shape (S > 1, N > 8192, wider patterns) is the
// loop of srcdsp_corr_step over the channels.  Either way every handle is left
// bit for bit as srcdsp_corr_step leaves it.
#include <algorithm>

#include "ops.h"
#include "corr_state.h"
#include "corr_scan_kernels.h"
#include "corr_tail.h"

namespace srcdsp {

// one launch's channels (passed by value: 3.8 KB of the 4 KB kernel arguments)
struct CorrBankArgs {
    CorrChanArgs ch;
    unsigned *best;  // [channels]
    uint32_t *res;   // [channels][kCorrRow]
    uint32_t *bits;  // [channels][N]
};
static_assert(sizeof(CorrBankArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kCBlock, SRCDSP_CORR_MINW) void corr_bank_s1(const CorrBankArgs A) {
    const int c = blockIdx.y;
    corr_scan_tile(A.ch.in + (long)c * A.ch.in_stride, A.ch.n, A.ch.hist[c], A.ch.ptaps[c], A.ch.N, A.ch.NP,
                   A.ch.cs[c], A.ch.prev[c][0], A.ch.prev[c][1], A.ch.prev[c][3], A.best + c, (long)blockIdx.x);
}

// the per-channel tail of a step, one workgroup per channel (N <= kCorrDot2MaxTaps here)
__global__ __launch_bounds__(kCorrTailBlock) void corr_bank_finish(const CorrBankArgs A) {
    const int c = blockIdx.x;
    corr_tail(A.ch.in + (long)c * A.ch.in_stride, A.ch.n, A.ch.hist[c], A.ch.hist_out[c], A.ch.coef[c],
              (unsigned)A.ch.N, 1u, A.ch.cs[c], A.ch.prev[c], A.best[c], A.res + (long)kCorrRow * c,
              A.bits + (long)c * A.ch.N, 0u, 1u);
}

namespace {
PathCounter g_bank_calls, g_loop_calls;

int bank_run(const srcdsp_corr_t *hs, int channels, const uint32_t *d_in, size_t in_stride, long n, int *found,
             int *corr_index, hipStream_t s) {
    srcdsp_corr_state &lead = hs[0]->c;
    const size_t C = (size_t)channels, N = lead.N;
    // hs[0]'s scratch: device best[C] | res[C][kCorrRow] | bits[C][N], pinned host res | bits
    int rc = lead.bank.reserve(4 * C * (1 + kCorrRow + N));
    if (rc) return rc;
    unsigned *d_best = lead.bank.dev<unsigned>();
    uint32_t *d_res = d_best + C, *d_bits = d_res + kCorrRow * C;
    uint32_t *h_res = lead.bank.host<uint32_t>(), *h_bits = h_res + kCorrRow * C;
    for (int c = 0; c < channels; ++c) {
        rc = hs[c]->c.order.before(s);
        if (rc) return rc;
    }
    SRCDSP_HIP_TRY(hipMemsetAsync(d_best, 0xff, 4 * C, s));
    constexpr long TO = (long)kCBlock * kCR;
    const unsigned tiles = (unsigned)((n + TO - 1) / TO);
    const size_t smem = 4 * (size_t)corr_scan_lds_words((int)lead.NP);
    for (int c0 = 0; c0 < channels; c0 += kMaxBatch) {
        const int nc = std::min(kMaxBatch, channels - c0);
        CorrBankArgs A{};
        corr_chan_args(A.ch, hs + c0, nc, d_in + (size_t)c0 * in_stride, in_stride, n);
        A.best = d_best + c0;
        A.res = d_res + (size_t)kCorrRow * c0;
        A.bits = d_bits + N * c0;
        hipLaunchKernelGGL(corr_bank_s1, dim3(tiles, (unsigned)nc), dim3(kCBlock), smem, s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(corr_bank_finish, dim3((unsigned)nc), dim3(kCorrTailBlock), 0, s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_res, d_res, 4 * kCorrRow * C, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    int hit_lo = channels, hit_hi = -1;
    for (int c = 0; c < channels; ++c)
        if (h_res[(size_t)kCorrRow * c] != kCorrNone) {
            hit_lo = std::min(hit_lo, c);
            hit_hi = c;
        }
    if (hit_hi >= 0) {  // the bitSamples rows of the channels that hit, in one copy
        SRCDSP_HIP_TRY(hipMemcpyAsync(h_bits + N * hit_lo, d_bits + N * hit_lo, 4 * N * (size_t)(hit_hi - hit_lo + 1),
                                      hipMemcpyDeviceToHost, s));
        SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    }
    for (int ch = 0; ch < channels; ++ch) {
        rc = corr_commit(hs[ch]->c, h_res + (size_t)kCorrRow * ch, h_bits + N * ch, found + ch, corr_index + ch, s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}
}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_corr_step_batched(const srcdsp_corr_t *hs, int channels, const void *d_in, size_t in_stride,
                                        size_t n, int *found, int *corr_index, void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && found != nullptr && corr_index != nullptr && channels >= 1,
                     "corr_step_batched: no handles or result arrays");
    int rc = check_handles(hs, channels, "corr_step_batched");
    if (rc) return rc;
    const srcdsp_corr_state &c0 = hs[0]->c;
    bool bank = corr_fused_shape(c0);
    for (int c = 1; c < channels; ++c) {
        SRCDSP_ARG_CHECK(hs[c]->c.N == c0.N && hs[c]->c.S == c0.S, "corr_step_batched: correlators must share N and S");
        bank = bank && corr_fused_shape(hs[c]->c);
    }
    for (int c = 0; c < channels; ++c) found[c] = 0;
    if (n == 0) return SRCDSP_OK;
    if (n > 0x7fffffffUL) {
        set_error("corr_step_batched: input longer than INT_MAX samples (correlators.h:212 uses int)");
        return SRCDSP_ERR_SIZE;
    }
    SRCDSP_ARG_CHECK(d_in != nullptr, "corr_step_batched: null input");
    if (!bank) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c)
            rc = srcdsp_corr_step(hs[c], chan_row(d_in, c, in_stride), n, found + c, corr_index + c, stream);
        return rc;
    }
    g_bank_calls.hit();
    return bank_run(hs, channels, (const uint32_t *)d_in, in_stride, (long)n, found, corr_index, (hipStream_t)stream);
}

SRCDSP_API int srcdsp_corr_batched_stats(unsigned long *bank_calls, unsigned long *loop_calls) {
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
