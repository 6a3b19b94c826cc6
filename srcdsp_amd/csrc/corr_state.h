// corr_state.h -- the correlator handle, its host staging and the geometry of
// its dot2 tiles, shared by corr.hip (the single-channel calls), corr_bank.hip
// (srcdsp_corr_step_batched) and corr_all.hip (srcdsp_corr_step_all).
#pragma once
#include <vector>

#include "ops.h"

namespace srcdsp {

typedef short short2_t __attribute__((ext_vector_type(2)));

struct srcdsp_corr_state {
    unsigned N = 0, S = 1, NS = 0;
    unsigned NP = 0;             // N rounded up to 16 (the dot2 tap array is front-padded with zero taps)
    int32_t *d_coef = nullptr;   // conj(pattern), N complex<int32_t> (2N int32)
    std::vector<int32_t> h_coef;
    uint32_t *d_ptaps = nullptr; // packed int16 pairs for v_dot2: (p.re,p.im),(-p.im,p.re) per tap, NP taps
    bool taps16 = false;         // every pattern component fits int16 (always true when the
                                 // reference's energy assert holds)
    uint32_t *d_hist[2] = {nullptr, nullptr};  // last NS-1 effective samples (packed ci16)
    int cur = 0;
    GrowBuf corr_vals{GrowBuf::kDevice}, en_vals{GrowBuf::kDevice};  // per-sample scratch of the segmented kernels
    // the single-channel scans' `best` word
    unsigned *d_best = nullptr;
    // the tail's results, device and pinned host mirror: a result row and a
    // bitSamples row of this handle's own steps, or per channel of the batched
    // calls it led (hs[0] of srcdsp_corr_step_batched / _all_batched)
    GrowBuf bank;
    // CorrState (correlators.h:59-81)
    uint32_t energy[3] = {0, 0, 0}, corr[3] = {0, 0, 0};
    uint32_t coeffs_energy = 0;
    int coeff_scaling = 0;
    double threshold_factor = 0;
    std::vector<int16_t> bits;  // bitSamples, N complex<int16_t>
    Ordering order;
    HostStage stage;
};

// effective stream sample j of a call: the input from 0 on, the NSm1 history
// samples before it, zeros before those
__device__ __forceinline__ uint32_t corr_fetch(const uint32_t *in, const uint32_t *hist, long j, long NSm1) {
    return j >= 0 ? in[j] : (j + NSm1 >= 0 ? hist[j + NSm1] : 0u);
}

constexpr int kCR = 16;       // outputs per lane
constexpr int kCBlock = 256;  // lanes per workgroup
// corr_scan_s1 at 5 waves per SIMD (<= 96 VGPRs, no spills): -1.4 % against 4
// (profiles/tuning/r04_corr_ab.txt)
#ifndef SRCDSP_CORR_MINW
#define SRCDSP_CORR_MINW 5
#endif
// Dynamic LDS of the dot2 tiles: the staged window, corr_lds_words(NP) words
// (chunks of 16 samples + 4 pad words); the fused scan appends its chunk sums,
// kCBlock + NP/16 words.  At the largest NP, 8192: 61.6 KB + 3.0 KB (gfx950
// gives a workgroup up to 160 KB).
constexpr unsigned kCorrDot2MaxTaps = 8192;
__host__ __device__ constexpr int corr_lds_words(int NP) { return ((kCBlock * kCR + NP + 1) / kCR + 2) * (kCR + 4); }
__host__ __device__ constexpr int corr_scan_lds_words(int NP) { return corr_lds_words(NP) + kCBlock + NP / 16; }

// the fused scan serves this handle (S == 1, int16-range pattern, NP taps stageable)
inline bool corr_fused_shape(const srcdsp_corr_state &c) {
    return c.taps16 && c.NP <= kCorrDot2MaxTaps && c.S == 1;
}

// the *_host entry points: n host samples into the handle's pinned stage and
// on to its device buffer (c.stage.d_buf), on the handle's own stream
inline int corr_stage_in(srcdsp_corr_state &c, const void *in, size_t n) {
    const int rc = c.stage.reserve(4 * n, 4 * n);
    if (rc) return rc;
    host_copy(c.stage.h_buf, in, 4 * n);
    SRCDSP_HIP_TRY(hipMemcpyAsync(c.stage.d_buf, c.stage.h_buf, 4 * n, hipMemcpyHostToDevice, c.stage.stream));
    return SRCDSP_OK;
}

}  // namespace srcdsp

struct srcdsp_corr { srcdsp::srcdsp_corr_state c; };
