// corr_all.hip -- srcdsp_corr_step_all: every detection the loop of
// FixedPatternCorrelator::step on the remainders makes in a stream, for one
// correlator or C of them (shared N and S, own patterns), in one call.
//
// Dispatch.  The shapes of the fused scan (corr_fused_shape: S == 1, an
// int16-range pattern, NP <= kCorrDot2MaxTaps) take two launches for up to
// kMaxBatch channels,
//   corr_all_map     : corr_scan_s1's tile without its early exit, grid row =
//                      channel -- one bit per output, "the peak test fires on
//                      the undisturbed stream", into a per-channel bitmap;
//   corr_all_resolve : one workgroup per channel runs the walk of
//                      corr_all_walk.h over the bitmap -- accepts a candidate,
//                      recomputes the patch after it on the stream with the
//                      detected samples deleted, and finishes with a tail of
//                      its own (registers, new history, the bitSamples row of
//                      every detection, one result row: corr_tail's work, but
//                      stepping over the deleted samples),
// then one D2H copy of the result rows and detection lists and one of the
// bitSamples rows: two host synchronisations at most, whatever the channel
// count and the number of detections.  Every other shape runs the literal
// loop of srcdsp_corr_step inside the call.
#include <algorithm>

#include "ops.h"
#include "corr_state.h"
#include "corr_scan_kernels.h"
#include "corr_tail.h"  // the per-channel argument block, the register commit
#include "corr_all_walk.h"

namespace srcdsp {

constexpr int kAllRow = 8;        // result row: hits, consumed, corr[3], energy[3]
constexpr int kAllBlock = 1024;   // lanes of a resolve workgroup = outputs per patch batch

struct CorrAllArgs {
    CorrChanArgs ch;
    int max_hits;
    uint16_t *map;    // [channels][map_stride]: one bit per output, written whole by corr_all_map
    long map_stride;  // 16-bit words per channel (tiles * kCBlock)
    int *det;         // [channels][max_hits]: the detected samples, ascending
    uint32_t *res;    // [channels][kAllRow]
    uint32_t *bits;   // [channels][max_hits][N]
};
static_assert(sizeof(CorrAllArgs) <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kCBlock, SRCDSP_CORR_MINW) void corr_all_map(const CorrAllArgs A) {
    const int c = blockIdx.y;
    const CorrChanArgs &H = A.ch;
    corr_scan_tile<true>(H.in + (long)c * H.in_stride, H.n, H.hist[c], H.ptaps[c], H.N, H.NP, H.cs[c], H.prev[c][0],
                         H.prev[c][1], H.prev[c][3], nullptr, (long)blockIdx.x, A.map + (long)c * A.map_stride);
}

// the walk's cooperative parts for one workgroup of kAllBlock lanes
struct CorrAllDev {
    const uint32_t *in, *hist;
    const int32_t *coef;
    const unsigned long long *map64;
    long nwords;  // 64-bit words of the channel's bitmap
    int *det;
    int N;
    unsigned cs;
    uint32_t pc[3], pe[3];
    const uint32_t *ptaps;  // the scan's packed taps, front-padded with `pad` zero taps
    int pad;
    uint32_t *win;      // LDS, N - 1 + kAllBlock words (dynamic)
    uint32_t *cb, *eb;  // LDS, kAllBlock words each
    unsigned *found;    // LDS

    __device__ long next(long pos) {
        const long w0 = pos >> 6;
        for (long base = w0; base < nwords; base += kAllBlock) {
            if (threadIdx.x == 0) *found = 0xffffffffu;
            __syncthreads();
            const long w = base + threadIdx.x;
            if (w < nwords) {
                unsigned long long v = map64[w];
                if (w == w0) v &= ~0ull << (pos & 63);
                if (v) atomicMin(found, (unsigned)(w * 64 + __builtin_ctzll(v)));
            }
            __syncthreads();
            const unsigned f = *found;
            __syncthreads();
            if (f != 0xffffffffu) return (long)f;
        }
        return -1;
    }
    // A batch with no deleted sample inside it (every patch batch: the
    // deletions lie before the patch) is a plain correlation over a window
    // staged in LDS: the N - 1 samples before j that are not deleted, then
    // samples j .. j + cnt - 1; lane t sums win[t .. t + N - 1] with the scan's
    // dot2 arithmetic (int32 wrap-around, equal to corr_all_value's sums).
    // Otherwise (the three register values at the end of a call can follow a
    // detection two samples back) each lane walks the stream itself.
    __device__ void eval(long j, int cnt, int k) {
        __syncthreads();  // det[] recorded, the previous batch read
        const int kd0 = corr_all_before(det, k, j);
        const bool inside = kd0 < k && det[kd0] < j + cnt - 1;
        if (!inside) {
            const int W = N - 1;
            for (int u = threadIdx.x; u < W + cnt; u += kAllBlock)
                win[u] = u < W ? corr_fetch(in, hist, corr_all_back(det, kd0, j, W - u), W) : in[j + (u - W)];
            __syncthreads();
            if ((int)threadIdx.x < cnt) {
                const uint32_t *x = win + threadIdx.x;
                // the taps through a wave-uniform constant view: scalar loads (common.h).
                // readfirstlane returns int: each half goes through uint32_t, or a low
                // half with bit 31 set would sign-extend over the high one
                const uint64_t ta = (uint64_t)(uintptr_t)(ptaps + 2 * pad);
                const uint32_t ta_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ta);
                const uint32_t ta_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ta >> 32));
                ConstPtr<uint32_t> tp = const_view<uint32_t>((const void *)(uintptr_t)(((uint64_t)ta_hi << 32) | ta_lo));
                int32_t r = 0, q = 0, en = 0;
#pragma unroll 8
                for (int m = 0; m < N; ++m) {
                    const short2_t s = __builtin_bit_cast(short2_t, x[m]);
                    r = __builtin_amdgcn_sdot2(s, __builtin_bit_cast(short2_t, tp[2 * m]), r, false);
                    q = __builtin_amdgcn_sdot2(s, __builtin_bit_cast(short2_t, tp[2 * m + 1]), q, false);
                    en = __builtin_amdgcn_sdot2(s, s, en, false);
                }
                cb[threadIdx.x] = corr_value(r, q, cs);
                eb[threadIdx.x] = (uint32_t)en >> ((unsigned)((int)cs / 2) & 31u);
            }
        } else if ((int)threadIdx.x < cnt) {
            const long jj = j + threadIdx.x;
            const uint32_t *in_ = in, *hist_ = hist;
            const long NSm1 = N - 1;
            uint32_t c, e;
            corr_all_value([=](long p) { return corr_fetch(in_, hist_, p, NSm1); }, coef, N, cs, det,
                           corr_all_before(det, k, jj), jj, c, e);
            cb[threadIdx.x] = c;
            eb[threadIdx.x] = e;
        }
        __syncthreads();
    }
    __device__ uint32_t c(int t) const { return cb[t]; }
    __device__ uint32_t e(int t) const { return eb[t]; }
    __device__ int batch() const { return kAllBlock; }
    __device__ int first_hit(int cnt, uint32_t c2, uint32_t c1, uint32_t e1) {
        if (threadIdx.x == 0) *found = 0xffffffffu;
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            uint32_t a2, a1, ae;
            corr_all_triple(cb, eb, (int)threadIdx.x, c2, c1, e1, a2, a1, ae);
            if (corr_hit(a2, a1, cb[threadIdx.x], ae)) atomicMin(found, threadIdx.x);
        }
        __syncthreads();
        const unsigned f = *found;
        __syncthreads();
        return f == 0xffffffffu ? -1 : (int)f;
    }
    __device__ void record(int k, long q) {
        if (threadIdx.x == 0) det[k] = (int)q;
    }
};

__global__ __launch_bounds__(kAllBlock) void corr_all_resolve(const CorrAllArgs A) {
    const CorrChanArgs &H = A.ch;
    __shared__ uint32_t cb[kAllBlock], eb[kAllBlock];
    __shared__ unsigned found;
    const int c = blockIdx.x;
    const uint32_t *in = H.in + (long)c * H.in_stride, *hist = H.hist[c];
    int *det = A.det + (long)c * A.max_hits;
    CorrAllDev x;
    x.in = in;
    x.hist = hist;
    x.coef = H.coef[c];
    x.map64 = (const unsigned long long *)(A.map + (long)c * A.map_stride);
    x.nwords = A.map_stride / 4;
    x.det = det;
    x.N = H.N;
    x.cs = H.cs[c];
    for (int k = 0; k < 3; ++k) {
        x.pc[k] = H.prev[c][k];
        x.pe[k] = H.prev[c][3 + k];
    }
    extern __shared__ __attribute__((aligned(16))) uint32_t win[];
    x.ptaps = H.ptaps[c];
    x.pad = H.NP - H.N;
    x.win = win;
    x.cb = cb;
    x.eb = eb;
    x.found = &found;
    CorrAllResult r;
    corr_all_walk(x, H.n, H.N, A.max_hits, r);
    __syncthreads();  // det[] complete
    if (threadIdx.x == 0) {
        uint32_t *row = A.res + (long)kAllRow * c;
        row[0] = (uint32_t)r.hits;
        row[1] = (uint32_t)r.consumed;
        for (int k = 0; k < 3; ++k) {
            row[2 + k] = r.corr[k];
            row[5 + k] = r.energy[k];
        }
    }
    const long NSm1 = H.N - 1;
    // history: the last N - 1 samples processed and not deleted
    uint32_t *ho = H.hist_out[c];
    for (long k = threadIdx.x; k < NSm1; k += kAllBlock)
        ho[k] = corr_fetch(in, hist, corr_all_back(det, r.hits, r.consumed, NSm1 - k), NSm1);
    // bitSamples of every detection (correlators.h:278-288 at S = 1): the ring
    // read backwards from the peak sample; its oldest slot holds the detected sample
    uint32_t *bo = A.bits + (long)c * A.max_hits * H.N;
    for (long g = threadIdx.x; g < (long)r.hits * H.N; g += kAllBlock) {
        const int h = (int)(g / H.N), m = (int)(g % H.N);
        const long q = det[h];
        bo[g] = corr_fetch(in, hist, m == 0 ? q : corr_all_back(det, h, q, H.N - m), NSm1);
    }
}

namespace {
PathCounter g_kernel_calls, g_loop_calls;

// detections lie at least two samples apart (the sample after one cannot be a peak)
size_t hits_cap(size_t n, int max_hits) { return std::min<size_t>((size_t)max_hits, n / 2 + 1); }

int all_kernels(const srcdsp_corr_t *hs, int channels, const uint32_t *d_in, size_t in_stride, long n, int max_hits,
                int *n_hits, int *corr_index, int16_t *bits_host, size_t *consumed, hipStream_t s) {
    srcdsp_corr_state &lead = hs[0]->c;
    const size_t C = (size_t)channels, N = lead.N;
    const size_t H = hits_cap((size_t)n, max_hits);  // rows the kernels can fill
    constexpr long TO = (long)kCBlock * kCR;
    const size_t tiles = (size_t)((n + TO - 1) / TO), map_stride = tiles * kCBlock;
    // hs[0]'s scratch: res[C][kAllRow] | det[C][H] | bits[C][H][N] | map[C][map_stride] (16-bit);
    // the pinned mirror takes the first three
    const size_t w_res = kAllRow * C, w_det = C * H, w_bits = C * H * N;
    int rc = lead.bank.reserve(4 * (w_res + w_det + w_bits) + 2 * C * map_stride + 16);
    if (rc) return rc;
    uint32_t *d_res = lead.bank.dev<uint32_t>();
    int *d_det = (int *)(d_res + w_res);
    uint32_t *d_bits = (uint32_t *)(d_det + w_det);
    uint16_t *d_map = (uint16_t *)(((uintptr_t)(d_bits + w_bits) + 15) & ~(uintptr_t)15);
    uint32_t *h_res = lead.bank.host<uint32_t>();
    int *h_det = (int *)(h_res + w_res);
    uint32_t *h_bits = (uint32_t *)(h_det + w_det);
    for (int c = 0; c < channels; ++c) {
        rc = hs[c]->c.order.before(s);
        if (rc) return rc;
    }
    const size_t smem = 4 * (size_t)corr_scan_lds_words((int)lead.NP);
    for (int c0 = 0; c0 < channels; c0 += kMaxBatch) {
        const int nc = std::min(kMaxBatch, channels - c0);
        CorrAllArgs A{};
        corr_chan_args(A.ch, hs + c0, nc, d_in + (size_t)c0 * in_stride, in_stride, n);
        A.max_hits = (int)H;
        A.map = d_map + map_stride * c0;
        A.map_stride = (long)map_stride;
        A.det = d_det + H * c0;
        A.res = d_res + (size_t)kAllRow * c0;
        A.bits = d_bits + H * N * c0;
        hipLaunchKernelGGL(corr_all_map, dim3((unsigned)tiles, (unsigned)nc), dim3(kCBlock), smem, s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(corr_all_resolve, dim3((unsigned)nc), dim3(kAllBlock), 4 * (N - 1 + kAllBlock), s, A);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_res, d_res, 4 * (w_res + w_det), hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    bool any = false;
    for (size_t c = 0; c < C; ++c) {  // the bitSamples rows made, one copy per channel, one synchronisation
        const size_t k = h_res[kAllRow * c];
        if (k == 0) continue;
        // without bits_host only the last row is needed (the handle's bitSamples)
        const size_t first = bits_host ? 0 : k - 1;
        SRCDSP_HIP_TRY(hipMemcpyAsync(h_bits + (c * H + first) * N, d_bits + (c * H + first) * N, 4 * N * (k - first),
                                      hipMemcpyDeviceToHost, s));
        any = true;
    }
    if (any) SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    for (int ch = 0; ch < channels; ++ch) {
        srcdsp_corr_state &c = hs[ch]->c;
        const uint32_t *row = h_res + (size_t)kAllRow * ch;
        const size_t k = row[0];
        corr_commit_regs(c, row);
        n_hits[ch] = (int)k;
        consumed[ch] = row[1];
        for (size_t q = 0; q < k; ++q) corr_index[(size_t)ch * max_hits + q] = h_det[ch * H + q] - 1;
        if (k) {
            memcpy(c.bits.data(), h_bits + (ch * H + k - 1) * N, 4 * N);
            if (bits_host) memcpy(bits_host + 2 * (size_t)ch * max_hits * N, h_bits + ch * H * N, 4 * N * k);
        }
        rc = c.order.after(s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

// the definition itself: srcdsp_corr_step on the remainders
int all_loop(srcdsp_corr_t h, const uint32_t *d_in, size_t n, int max_hits, int *n_hits, int *corr_index,
             int16_t *bits_host, size_t *consumed, hipStream_t s) {
    const size_t N = h->c.N;
    size_t off = 0;
    int k = 0;
    while (off < n && k < max_hits) {
        int found = 0, ci = 0;
        const int rc = srcdsp_corr_step(h, d_in + off, n - off, &found, &ci, s);
        if (rc) return rc;
        if (!found) {
            off = n;
            break;
        }
        corr_index[k] = (int)off + ci;
        if (bits_host) memcpy(bits_host + 2 * N * (size_t)k, h->c.bits.data(), 4 * N);
        ++k;
        off += (size_t)(ci + 2);
    }
    *n_hits = k;
    *consumed = off;
    return SRCDSP_OK;
}
}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_corr_step_all_batched(const srcdsp_corr_t *hs, int channels, const void *d_in, size_t in_stride,
                                            size_t n, int max_hits, int *n_hits, int *corr_index, int16_t *bits_host,
                                            size_t *consumed, void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && n_hits != nullptr && corr_index != nullptr && consumed != nullptr &&
                         channels >= 1,
                     "corr_step_all: no handles or result arrays");
    SRCDSP_ARG_CHECK(max_hits >= 1, "corr_step_all: max_hits must be at least 1");
    int rc = check_handles(hs, channels, "corr_step_all");
    if (rc) return rc;
    const srcdsp_corr_state &c0 = hs[0]->c;
    bool kernels = corr_fused_shape(c0);
    for (int c = 1; c < channels; ++c) {
        SRCDSP_ARG_CHECK(hs[c]->c.N == c0.N && hs[c]->c.S == c0.S, "corr_step_all: correlators must share N and S");
        kernels = kernels && corr_fused_shape(hs[c]->c);
    }
    if (n > 0x7fffffffUL) {
        set_error("corr_step_all: input longer than INT_MAX samples (correlators.h:212 uses int)");
        return SRCDSP_ERR_SIZE;
    }
    for (int c = 0; c < channels; ++c) {
        n_hits[c] = 0;
        consumed[c] = 0;
    }
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in != nullptr, "corr_step_all: null input");
    if (!kernels) {
        g_loop_calls.hit();
        const size_t N = c0.N;
        for (int c = 0; c < channels && !rc; ++c)
            rc = all_loop(hs[c], (const uint32_t *)chan_row(d_in, c, in_stride), n, max_hits, n_hits + c,
                          corr_index + (size_t)c * max_hits,
                          bits_host ? bits_host + 2 * (size_t)c * max_hits * N : nullptr, consumed + c,
                          (hipStream_t)stream);
        return rc;
    }
    g_kernel_calls.hit();
    return all_kernels(hs, channels, (const uint32_t *)d_in, in_stride, (long)n, max_hits, n_hits, corr_index,
                       bits_host, consumed, (hipStream_t)stream);
}

SRCDSP_API int srcdsp_corr_step_all(srcdsp_corr_t h, const void *d_in, size_t n, int max_hits, int *n_hits,
                                    int *corr_index, int16_t *bits_host, size_t *consumed, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr, "corr_step_all: null handle");
    return srcdsp_corr_step_all_batched(&h, 1, d_in, 0, n, max_hits, n_hits, corr_index, bits_host, consumed, stream);
}

SRCDSP_API int srcdsp_corr_step_all_host(srcdsp_corr_t h, const void *in, size_t n, int max_hits, int *n_hits,
                                         int *corr_index, int16_t *bits_host, size_t *consumed) {
    SRCDSP_ARG_CHECK(h != nullptr && (in != nullptr || n == 0), "corr_step_all_host: null argument");
    if (n == 0 || n > 0x7fffffffUL || max_hits < 1 || !n_hits || !corr_index || !consumed)  // refused or empty: no staging
        return srcdsp_corr_step_all(h, in, n, max_hits, n_hits, corr_index, bits_host, consumed, nullptr);
    srcdsp_corr_state &c = h->c;
    const int rc = corr_stage_in(c, in, n);
    if (rc) return rc;
    return srcdsp_corr_step_all(h, c.stage.d_buf, n, max_hits, n_hits, corr_index, bits_host, consumed,
                                c.stage.stream);
}

SRCDSP_API int srcdsp_corr_all_stats(unsigned long *kernel_calls, unsigned long *loop_calls) {
    g_kernel_calls.read(kernel_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

}  // extern "C"
