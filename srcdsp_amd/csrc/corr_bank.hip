// corr_bank.hip -- srcdsp_corr_step_batched: C FixedPatternCorrelators (shared
// N and S, own patterns) each scanned up to its own first detection in one
// call, on one input per channel or on one shared input.
//
// Dispatch.  The bank serves the shapes of the fused single-channel scan
// (corr_run's `fused`): S == 1, an int16-range pattern in every channel and
// NP <= kCorrDot2MaxTaps.  It is two launches for up to kMaxBatch channels,
//   corr_bank_s1     : corr_scan_s1's tile (corr_scan_kernels.h), grid row = channel;
//   corr_bank_finish : one workgroup per channel -- the registers at the last
//                      processed sample, the new history, bitSamples and a
//                      packed result row,
// then one D2H copy of the result rows and, when some channel hit, one more of
// those channels' bitSamples rows: two host synchronisations at most, however
// many channels.  Every other shape (S > 1, N > 8192, wider patterns) is the
// loop of srcdsp_corr_step over the channels.  Either way every handle is left
// bit for bit as srcdsp_corr_step leaves it.
#include <algorithm>

#include "ops.h"
#include "corr_state.h"
#include "corr_scan_kernels.h"

namespace srcdsp {

constexpr unsigned kNone = 0xffffffffu;
constexpr int kRow = 8;  // result row: best, pad, corr(last - 0..2), energy(last - 0..2)

// one launch's channels (passed by value: 3.1 KB of the 4 KB kernel arguments)
struct CorrBankArgs {
    const uint32_t *in;  // channel c reads in + c * in_stride (0: one shared input)
    long in_stride, n;
    int N, NP;
    unsigned *best;  // [channels]
    uint32_t *res;   // [channels][kRow]
    uint32_t *bits;  // [channels][N]
    const uint32_t *hist[kMaxBatch];
    uint32_t *hist_out[kMaxBatch];
    const uint32_t *ptaps[kMaxBatch];
    const int32_t *coef[kMaxBatch];
    unsigned cs[kMaxBatch];
    uint32_t prev[kMaxBatch][3];  // corr[0], corr[1], energy[0] carried from the previous call
};
static_assert(sizeof(CorrBankArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kCBlock, SRCDSP_CORR_MINW) void corr_bank_s1(const CorrBankArgs A) {
    const int c = blockIdx.y;
    corr_scan_tile(A.in + (long)c * A.in_stride, A.n, A.hist[c], A.ptaps[c], A.N, A.NP, A.cs[c], A.prev[c][0],
                   A.prev[c][1], A.prev[c][2], A.best + c, (long)blockIdx.x);
}

// the per-channel tail of a step (corr_run after its scan), on the device
__global__ __launch_bounds__(256) void corr_bank_finish(const CorrBankArgs A) {
    const int c = blockIdx.x;
    const uint32_t *in = A.in + (long)c * A.in_stride, *hist = A.hist[c];
    const unsigned b = A.best[c];
    uint32_t *row = A.res + (long)kRow * c;
    corr_point_regs(in, A.n, hist, A.coef[c], (unsigned)A.N, 1u, A.cs[c], b, row + 2);
    if (threadIdx.x == 0) {
        row[0] = b;
        row[1] = 0;
    }
    const bool hit = b != kNone;
    const long NSm1 = A.N - 1;
    // history: the last N - 1 samples of the effective stream; the detected
    // sample is not kept (correlators.h:291 breaks without advancing `top`)
    const long last_eff = hit ? (long)b - 1 : A.n - 1;
    uint32_t *ho = A.hist_out[c];
    for (long k = threadIdx.x; k < NSm1; k += blockDim.x) ho[k] = corr_fetch(in, hist, last_eff - NSm1 + 1 + k, NSm1);
    // bitSamples (correlators.h:278-288) at S = 1: the ring read backwards from
    // the peak sample b - 1; its oldest slot already holds the detected sample
    if (hit) {
        uint32_t *bo = A.bits + (long)c * A.N;
        for (int m = threadIdx.x; m < A.N; m += blockDim.x)
            bo[m] = corr_fetch(in, hist, m == 0 ? (long)b : (long)b - 1 - (A.N - 1 - m), NSm1);
    }
}

namespace {
PathCounter g_bank_calls, g_loop_calls;

int bank_run(const srcdsp_corr_t *hs, int channels, const uint32_t *d_in, size_t in_stride, long n, int *found,
             int *corr_index, hipStream_t s) {
    srcdsp_corr_state &lead = hs[0]->c;
    const size_t C = (size_t)channels, N = lead.N;
    // hs[0]'s scratch: device best[C] | res[C][kRow] | bits[C][N], pinned host res | bits
    int rc = lead.bank.reserve(4 * C * (1 + kRow + N));
    if (rc) return rc;
    unsigned *d_best = lead.bank.dev<unsigned>();
    uint32_t *d_res = d_best + C, *d_bits = d_res + kRow * C;
    uint32_t *h_res = lead.bank.host<uint32_t>(), *h_bits = h_res + kRow * C;
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
        A.in = d_in + (size_t)c0 * in_stride;
        A.in_stride = (long)in_stride;
        A.n = n;
        A.N = (int)lead.N;
        A.NP = (int)lead.NP;
        A.best = d_best + c0;
        A.res = d_res + (size_t)kRow * c0;
        A.bits = d_bits + N * c0;
        for (int k = 0; k < nc; ++k) {
            srcdsp_corr_state &c = hs[c0 + k]->c;
            hist_pair(c, A.hist[k], A.hist_out[k]);
            A.ptaps[k] = c.d_ptaps;
            A.coef[k] = c.d_coef;
            A.cs[k] = (unsigned)c.coeff_scaling;
            A.prev[k][0] = c.corr[0];
            A.prev[k][1] = c.corr[1];
            A.prev[k][2] = c.energy[0];
        }
        hipLaunchKernelGGL(corr_bank_s1, dim3(tiles, (unsigned)nc), dim3(kCBlock), smem, s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(corr_bank_finish, dim3((unsigned)nc), dim3(256), 0, s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_res, d_res, 4 * kRow * C, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    int hit_lo = channels, hit_hi = -1;
    for (int c = 0; c < channels; ++c)
        if (h_res[(size_t)kRow * c] != kNone) {
            hit_lo = std::min(hit_lo, c);
            hit_hi = c;
        }
    if (hit_hi >= 0) {  // the bitSamples rows of the channels that hit, in one copy
        SRCDSP_HIP_TRY(hipMemcpyAsync(h_bits + N * hit_lo, d_bits + N * hit_lo, 4 * N * (size_t)(hit_hi - hit_lo + 1),
                                      hipMemcpyDeviceToHost, s));
        SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    }
    for (int ch = 0; ch < channels; ++ch) {
        srcdsp_corr_state &c = hs[ch]->c;
        const uint32_t *row = h_res + (size_t)kRow * ch;
        const unsigned best = row[0];
        const bool hit = best != kNone;
        const long last = hit ? (long)best : n - 1;  // last processed sample
        // registers after processing `last` (correlators.h:228-230, 248-250)
        uint32_t ncv[3], nev[3];
        for (int k = 0; k < 3; ++k) {
            const long idx = last - k;
            if (idx >= 0) {
                ncv[k] = row[2 + k];
                nev[k] = row[5 + k];
            } else {  // reach back into the previous registers
                ncv[k] = c.corr[-idx - 1];
                nev[k] = c.energy[-idx - 1];
            }
        }
        for (int k = 0; k < 3; ++k) {
            c.corr[k] = ncv[k];
            c.energy[k] = nev[k];
        }
        if (N > 1) c.cur ^= 1;
        found[ch] = hit ? 1 : 0;
        if (hit) {
            memcpy(c.bits.data(), h_bits + N * ch, 4 * N);
            corr_index[ch] = (int)best - 1;
        }
        rc = c.order.after(s);
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
