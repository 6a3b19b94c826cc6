// corr_tail.h -- the end of a correlator step, written once: everything that
// follows once a scan has left `best` (the first sample at which the peak test
// fired, or kCorrNone).
//   device : corr_tail -- the three corr / energy registers at the last
//            processed sample (reaching back into the previous call's where
//            the call was shorter than three samples or hit at index 0..2),
//            the new history with the detected sample dropped, bitSamples,
//            and one result row that leaves the kernel final;
//   host   : corr_commit -- that row into the handle.
// corr_step_tail (corr.hip, any stride, every scan path and priming) and
// corr_bank_finish (corr_bank.hip, one workgroup per channel) are this code;
// so is the per-channel argument block of the bank and all-detections launches.
// corr_all_resolve keeps a tail of its own: it walks a stream with deleted
// samples (corr_all_walk.h).
#pragma once
#include <cstring>

#include "corr_state.h"
#include "fir_device.h"

namespace srcdsp {

constexpr unsigned kCorrNone = 0xffffffffu;  // `best` of a scan that detected nothing
constexpr int kCorrRow = 8;                  // result row: best, pad, corr(last - 0..2), energy(last - 0..2)
constexpr int kCorrTailBlock = 256;

// Workgroup `wg` of the `nwg` that share one channel's tail (kCorrTailBlock
// lanes each; wg and every argument are block-uniform).  b = the scan's
// `best`; last = b on a detection, else n - 1.  prev = corr[0..2],
// energy[0..2] carried into the call.
//  * workgroup 0: corr and energy at last - 0..2, each a direct sum over the N
//    taps with corr_eval's arithmetic (int32 wrap-around sums, so equal to the
//    scans' sliding energy); a position before the call takes the carried
//    register (correlators.h:228-230, 248-250);
//  * all workgroups: the history, the last N S - 1 samples of the effective
//    stream -- the detected sample is not kept (correlators.h:291 breaks
//    without advancing `top`) -- and on a detection bitSamples
//    (correlators.h:278-288): the ring read backwards from the peak sample
//    b - 1 with stride S; at S == 1 the oldest slot already holds the detected
//    sample (the ring wrapped onto it).
__device__ __forceinline__ void corr_tail(const uint32_t *__restrict__ in, long n, const uint32_t *__restrict__ hist,
                                          uint32_t *__restrict__ hist_out, const int32_t *__restrict__ coef,
                                          unsigned N, unsigned S, unsigned cs, const uint32_t *prev, unsigned b,
                                          uint32_t *__restrict__ row, uint32_t *__restrict__ bits, unsigned wg,
                                          unsigned nwg) {
    const bool hit = b != kCorrNone;
    const long last = hit ? (long)b : n - 1;
    const long NSm1 = (long)N * S - 1;
    if (wg == 0) {
        __shared__ uint32_t red[3][3][kCorrTailBlock];
        for (int k = 0; k < 3; ++k) {
            uint32_t tr = 0, ti = 0, e = 0;
            const long i = last - k;
            if (i >= 0)
                for (unsigned m = threadIdx.x; m < N; m += kCorrTailBlock) {
                    const uint32_t w = corr_fetch(in, hist, i - (long)(N - 1 - m) * S, NSm1);
                    const int32_t hr = sext16(w), hi = sext16_hi(w);
                    const int32_t cr = coef[2 * m], ci = coef[2 * m + 1];
                    tr += (uint32_t)hr * (uint32_t)cr - (uint32_t)hi * (uint32_t)ci;
                    ti += (uint32_t)hr * (uint32_t)ci + (uint32_t)hi * (uint32_t)cr;
                    e += (uint32_t)hr * (uint32_t)hr + (uint32_t)hi * (uint32_t)hi;
                }
            red[k][0][threadIdx.x] = tr;
            red[k][1][threadIdx.x] = ti;
            red[k][2][threadIdx.x] = e;
        }
        __syncthreads();
        for (int w = kCorrTailBlock / 2; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w)
                for (int k = 0; k < 3; ++k)
                    for (int q = 0; q < 3; ++q) red[k][q][threadIdx.x] += red[k][q][threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x < 3) {
            const int k = threadIdx.x;
            const long i = last - k;  // i < 0: carried register -i - 1 (0 or 1, as n >= 1)
            const int32_t sr = (int32_t)red[k][0][0] >> (cs & 31u), si = (int32_t)red[k][1][0] >> (cs & 31u);
            const int32_t ar = sr >> 2, ai = si >> 2;
            row[2 + k] = i >= 0 ? (uint32_t)ar * (uint32_t)ar + (uint32_t)ai * (uint32_t)ai : prev[-i - 1];
            row[5 + k] = i >= 0 ? red[k][2][0] >> ((unsigned)((int)cs / 2) & 31u) : prev[3 + (-i - 1)];
        }
        if (threadIdx.x == 0) {
            row[0] = b;
            row[1] = 0;
        }
    }
    const long t0 = (long)wg * kCorrTailBlock + threadIdx.x, step = (long)nwg * kCorrTailBlock;
    const long last_eff = hit ? (long)b - 1 : n - 1;
    for (long k = t0; k < NSm1; k += step) hist_out[k] = corr_fetch(in, hist, last_eff - NSm1 + 1 + k, NSm1);
    if (hit)
        for (long m = t0; m < (long)N; m += step) {
            const long d = ((long)N - 1 - m) * S;
            bits[m] = corr_fetch(in, hist, d == NSm1 ? (long)b : (long)b - 1 - d, NSm1);
        }
}

// ------------------------------------------------- per-channel launch arguments
// What the bank and the all-detections launches both carry for their channels
// (by value, beside their own result pointers: 3.8 KB of the 4 KB kernel arguments)
struct CorrChanArgs {
    const uint32_t *in;  // channel c reads in + c * in_stride (0: one shared input)
    long in_stride, n;
    int N, NP;
    const uint32_t *hist[kMaxBatch];
    uint32_t *hist_out[kMaxBatch];
    const uint32_t *ptaps[kMaxBatch];
    const int32_t *coef[kMaxBatch];
    unsigned cs[kMaxBatch];
    uint32_t prev[kMaxBatch][6];  // corr[0..2], energy[0..2] carried from the previous call
};

// channels hs[0 .. nc) of one launch; `in` is the first of them's row
inline void corr_chan_args(CorrChanArgs &A, const srcdsp_corr_t *hs, int nc, const uint32_t *in, size_t in_stride,
                           long n) {
    A.in = in;
    A.in_stride = (long)in_stride;
    A.n = n;
    A.N = (int)hs[0]->c.N;
    A.NP = (int)hs[0]->c.NP;
    for (int k = 0; k < nc; ++k) {
        const srcdsp_corr_state &c = hs[k]->c;
        hist_pair(c, A.hist[k], A.hist_out[k]);
        A.ptaps[k] = c.d_ptaps;
        A.coef[k] = c.d_coef;
        A.cs[k] = (unsigned)c.coeff_scaling;
        for (int q = 0; q < 3; ++q) {
            A.prev[k][q] = c.corr[q];
            A.prev[k][3 + q] = c.energy[q];
        }
    }
}

// -------------------------------------------------------------- host commit
// the registers of a result row (words 2..7) into the handle; the history the
// tail wrote becomes current
inline void corr_commit_regs(srcdsp_corr_state &c, const uint32_t *row) {
    for (int k = 0; k < 3; ++k) {
        c.corr[k] = row[2 + k];
        c.energy[k] = row[5 + k];
    }
    if (c.NS > 1) c.cur ^= 1;
}

// one step's result row (and, on a detection, its bitSamples row) into the
// handle and the caller's found / corr_index; records the step on s
inline int corr_commit(srcdsp_corr_state &c, const uint32_t *row, const uint32_t *bits, int *found, int *corr_index,
                       hipStream_t s) {
    corr_commit_regs(c, row);
    const bool hit = row[0] != kCorrNone;
    *found = hit ? 1 : 0;
    if (hit) {
        memcpy(c.bits.data(), bits, 4 * (size_t)c.N);
        *corr_index = (int)row[0] - 1;
    }
    return c.order.after(s);
}

}  // namespace srcdsp
