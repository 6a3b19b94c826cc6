// corr.hip -- dsptl::FixedPatternCorrelator<int16_t, int32_t, N, S>
// (correlators.h:54-316) on gfx950.
//
// The reference walks the input one sample at a time and stops at the first
// detection.  Everything it computes per sample depends only on the window of
// N*S samples ending there, so the step is split into
//   1. corr_eval   : every sample's scaled correlation |C_i>>2|^2 and scaled
//                    window energy, in parallel (int32 wrap-around arithmetic
//                    as the reference's complex<int32_t>/uint32 registers);
//   2. corr_detect : the 3-point peak + threshold test of correlators.h:262-268
//                    on each index, reduced to the FIRST index with atomicMin;
//   3. corr_step_tail : the state update, on the device (corr_tail.h) -- the
//                    registers, the N*S-1 sample history (the detected sample
//                    is dropped: the reference `break`s without advancing
//                    `top`, correlators.h:291), bitSamples; the host copies one
//                    result row back (and the bitSamples row on a detection)
//                    and commits it to the handle.
// At S == 1 steps 1 and 2 are one launch, corr_scan_s1 (corr_scan_kernels.h).
// The double-precision threshold sqrt(c) > sqrt(e)*2.7 is evaluated exactly:
// sqrt(e) > 300 <=> e > 90000 for integer e, and the correctly rounded sqrt of
// a uint32 is obtained from the hardware estimate by an exact 128-bit
// neighbour check, so no tolerance is involved.
#include <algorithm>
#include <vector>

#include "ops.h"
#include "fir_device.h"
#include "corr_hit.h"
#include "corr_state.h"         // the handle, corr_fetch, the dot2 tile geometry
#include "corr_scan_kernels.h"  // the fused scan's tile (shared with corr_bank.hip and corr_all.hip)
#include "corr_tail.h"          // the end of a step (shared with corr_bank.hip) and the host commit

namespace srcdsp {

// the detection test (correlators.h:262-268): corr_hit / corr_hit_exact in corr_hit.h

// ------------------------------------------------------------------ kernels
constexpr int kCorrBlock = 256;
constexpr size_t kCorrEvalMaxSmem = 64 * 1024;  // corr_eval's staged window + taps; longer: corr_eval_g
constexpr unsigned kCorrMaxGridY = 65535;       // corr_eval_dot2 runs one stride phase per grid row

// one output per lane; the block's window span and the taps are staged in LDS
__global__ __launch_bounds__(kCorrBlock) void corr_eval(const uint32_t *__restrict__ in, long n, long i_begin,
                                                        long i_end, const uint32_t *__restrict__ hist,
                                                        const int32_t *__restrict__ coef, unsigned N, unsigned S,
                                                        unsigned cs, uint32_t *__restrict__ corr_out,
                                                        uint32_t *__restrict__ en_out, const unsigned *stop) {
    if ((long)*stop < i_begin) return;  // an earlier segment already detected
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const long NSm1 = (long)N * S - 1;
    const long span = kCorrBlock + NSm1;  // samples i0-NSm1 .. i0+255
    uint32_t *xs = sm;
    int2 *cs2 = (int2 *)(sm + ((span + 3) & ~3l));
    const long i0 = i_begin + (long)blockIdx.x * kCorrBlock;
    for (long k = threadIdx.x; k < span; k += kCorrBlock) {
        long j = i0 - NSm1 + k;
        xs[k] = j < n ? corr_fetch(in, hist, j, NSm1) : 0u;
    }
    for (unsigned m = threadIdx.x; m < N; m += kCorrBlock) cs2[m] = make_int2(coef[2 * m], coef[2 * m + 1]);
    __syncthreads();
    const long i = i0 + threadIdx.x;
    if (i >= i_end) return;
    uint32_t tr = 0, ti = 0, e = 0;
    // window sample of tap m: x[i - (N-1-m) S]  ->  xs[threadIdx.x + (S-1) + m S]
    const uint32_t *xw = xs + threadIdx.x + (S - 1);
    for (unsigned m = 0; m < N; ++m) {
        const uint32_t w = xw[m * S];
        const int32_t hr = sext16(w), hi = sext16_hi(w);
        const int2 c = cs2[m];
        tr += (uint32_t)hr * (uint32_t)c.x - (uint32_t)hi * (uint32_t)c.y;
        ti += (uint32_t)hr * (uint32_t)c.y + (uint32_t)hi * (uint32_t)c.x;
        e += (uint32_t)hr * (uint32_t)hr + (uint32_t)hi * (uint32_t)hi;
    }
    const int32_t sr = (int32_t)tr >> (cs & 31u), si = (int32_t)ti >> (cs & 31u);  // scale32 :244
    const int32_t ar = sr >> 2, ai = si >> 2;                                       // :250
    corr_out[i] = (uint32_t)ar * (uint32_t)ar + (uint32_t)ai * (uint32_t)ai;
    en_out[i] = e >> ((unsigned)((int)cs / 2) & 31u);                                // :245
}

// -------------------------------------------------- register-tiled eval
// For stride 1 the correlation is a complex FIR over the last N samples:
//   C_i = sum_m x[i-(N-1)+m] * conj(p[m]).
// With packed complex<int16_t> words both real products of a tap are one
// v_dot2_i32_i16 (int16 x int16 -> int32, wrap-around accumulate, as the
// reference's complex<int32_t> arithmetic):
//   Re = dot2(x, (p.re, p.im)),  Im = dot2(x, (-p.im, p.re)).
// Each lane owns CR consecutive outputs and slides a register window over the
// taps (16 taps per chunk: CR+15 window words, 4 new ds_read_b128 per chunk for
// 2*16*CR dot2).  Window energy: direct sum for the lane's first output
// (one dot2(x,x) per tap), then E_{i+1} = E_i + |x_{i+1}|^2 - |x_{i+1-N}|^2.
// Taps (2N packed words) are scalar loads through a constant view.  The LDS
// image gets one 16-B pad per lane chunk (CR words), so the 16 lanes of a
// ds_read_b128 group touch 16 distinct bank slots.
// Any stride S and tap count N: outputs i = k S + ph of one phase ph (grid.y)
// correlate the phase stream x_ph[k] = x[k S + ph] with the pattern, a stride-1
// correlation of that stream, so each workgroup stages one phase's samples
// (a strided gather, through L2) and runs the stride-1 tiles on them.  The
// taps are front-padded with zero taps to NP = 16 ceil(N/16) (exact: a zero
// tap adds 0); the window energy covers the N real taps only (the padded
// positions' |x|^2 are taken off the direct sum, and the sliding update drops
// the oldest real sample).  (kCR, kCBlock, corr_lds_words: corr_state.h)

// corr_eval's arithmetic for windows too long to stage (N*S + 255 samples
// past kCorrEvalMaxSmem of LDS, e.g. S in the thousands): one output per lane,
// window samples and taps read through the cache (adjacent lanes read
// adjacent samples, so every tap is one coalesced load per wave)
__global__ __launch_bounds__(kCorrBlock) void corr_eval_g(const uint32_t *__restrict__ in, long n, long i_begin,
                                                          long i_end, const uint32_t *__restrict__ hist,
                                                          const int32_t *__restrict__ coef, unsigned N, unsigned S,
                                                          unsigned cs, uint32_t *__restrict__ corr_out,
                                                          uint32_t *__restrict__ en_out, const unsigned *stop) {
    if ((long)*stop < i_begin) return;
    const long i = i_begin + (long)blockIdx.x * kCorrBlock + threadIdx.x;
    if (i >= i_end) return;
    const long NSm1 = (long)N * S - 1;
    uint32_t tr = 0, ti = 0, e = 0;
    // tap m multiplies x[i - (N-1-m) S]
    long j = i - (long)(N - 1) * S;
    for (unsigned m = 0; m < N; ++m, j += S) {
        const uint32_t w = j < n ? corr_fetch(in, hist, j, NSm1) : 0u;
        const int32_t hr = sext16(w), hi = sext16_hi(w);
        const int32_t cr = coef[2 * m], ci = coef[2 * m + 1];
        tr += (uint32_t)hr * (uint32_t)cr - (uint32_t)hi * (uint32_t)ci;
        ti += (uint32_t)hr * (uint32_t)ci + (uint32_t)hi * (uint32_t)cr;
        e += (uint32_t)hr * (uint32_t)hr + (uint32_t)hi * (uint32_t)hi;
    }
    const int32_t sr = (int32_t)tr >> (cs & 31u), si = (int32_t)ti >> (cs & 31u);  // scale32 :244
    const int32_t ar = sr >> 2, ai = si >> 2;                                       // :250
    corr_out[i] = (uint32_t)ar * (uint32_t)ar + (uint32_t)ai * (uint32_t)ai;
    en_out[i] = e >> ((unsigned)((int)cs / 2) & 31u);                                // :245
}

__global__ __launch_bounds__(kCBlock) void corr_eval_dot2(const uint32_t *__restrict__ in, long n, long i_begin,
                                                           long i_end, const uint32_t *__restrict__ hist,
                                                           const uint32_t *__restrict__ ptaps, int N, int NP, int S,
                                                           unsigned cs, uint32_t *__restrict__ corr_out,
                                                           uint32_t *__restrict__ en_out, const unsigned *stop) {
    if ((long)*stop < i_begin) return;  // an earlier segment already detected
    extern __shared__ __attribute__((aligned(16))) uint32_t xs[];
    constexpr int TO = kCBlock * kCR;
    const int ph = blockIdx.y;
    const long NSm1 = (long)N * S - 1;
    // this phase's outputs of the segment: k in [kb, ke), i = k S + ph
    const long kb = (i_begin - ph + S - 1) / S, ke = (i_end - ph + S - 1) / S;
    const long k0 = kb + (long)blockIdx.x * TO;  // first output of the tile (phase stream)
    if (k0 >= ke) return;
    const long base = k0 - (NP - 1);             // first phase-stream sample the tile needs
    const int span = TO + NP - 1;
    const int pad = NP - N;
    // LDS word of tile sample l (l = sample - base): lp = l + 1 (aligns the lane
    // windows' new words to 16 B), one 4-word pad per kCR = 16 words, i.e.
    // 20-word chunks of which the last 4 are padding
    static_assert(kCR == 16, "LDS chunk geometry assumes 16 outputs per lane");
    auto lw = [&](int l) { int lp = l + 1; return lp + 4 * (lp / kCR); };
    for (int l = threadIdx.x; l < span; l += kCBlock) {
        const long j = (base + l) * S + ph;
        uint32_t w = 0;
        if (j < n) w = j >= 0 ? in[j] : (j + NSm1 >= 0 ? hist[j + NSm1] : 0u);
        xs[lw(l)] = w;
    }
    __syncthreads();
    const int t = threadIdx.x;
    // lane window W[j] = sample base + t*kCR + j  ->  LDS lw(t*kCR + j)
    int32_t ar[kCR], ai[kCR];
#pragma unroll
    for (int r = 0; r < kCR; ++r) ar[r] = ai[r] = 0;
    int32_t e0 = 0;
    const int lb = t * kCR;  // lane base in sample units
    // Window words j = 0..30 of a 16-tap chunk: j < 15 were loaded by the
    // previous chunk (its words 16..30), j >= 15 are the chunk's 16 new words.
    // Two register sets alternate roles (unrolled by 2), so sliding the window
    // costs no moves.
    uint32_t A[kCR + 15], B[kCR + 15];
#pragma unroll
    for (int j = 0; j < kCR - 1; ++j) B[16 + j] = xs[lw(lb + j)];
    ConstPtr<uint32_t> tp = const_view<uint32_t>(ptaps);
    auto chunk = [&](int m0, uint32_t(&cur)[kCR + 15], const uint32_t(&prev)[kCR + 15]) {
        asm volatile("" : "+s"(tp));
        uint32_t pw[32];  // this chunk's 16 taps (2 x s_load_dwordx16)
#pragma unroll
        for (int k = 0; k < 32; ++k) pw[k] = tp[2 * m0 + k];
        // new words: the whole 16-word LDS chunk t+1+m0/16 = uint4 slots 5(t+1+m0/16)..+3
        const uint4 *src = (const uint4 *)xs + 5 * (t + 1 + (m0 >> 4));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint4 q = src[g];
            cur[kCR - 1 + 4 * g + 0] = q.x;
            cur[kCR - 1 + 4 * g + 1] = q.y;
            cur[kCR - 1 + 4 * g + 2] = q.z;
            cur[kCR - 1 + 4 * g + 3] = q.w;
        }
        auto word = [&](int j) { return j < kCR - 1 ? prev[16 + j] : cur[j]; };
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const uint32_t p0 = pw[2 * mm], p1 = pw[2 * mm + 1];
            const short2_t x0 = __builtin_bit_cast(short2_t, word(mm));
            e0 = __builtin_amdgcn_sdot2(x0, x0, e0, false);
#pragma unroll
            for (int r = 0; r < kCR; ++r) {
                const short2_t x = __builtin_bit_cast(short2_t, word(mm + r));
                ar[r] = __builtin_amdgcn_sdot2(x, __builtin_bit_cast(short2_t, p0), ar[r], false);
                ai[r] = __builtin_amdgcn_sdot2(x, __builtin_bit_cast(short2_t, p1), ai[r], false);
            }
        }
    };
    int m0 = 0;
    for (; m0 + 32 <= NP; m0 += 32) {  // NP % 16 == 0
        chunk(m0, A, B);
        chunk(m0 + 16, B, A);
    }
    if (m0 < NP) chunk(m0, A, B);
    // outputs, energies (sliding) and stores; the direct sum ran over the NP
    // window words, the first pad of them before the real window
    uint32_t e = (uint32_t)e0;
    for (int q = 0; q < pad; ++q) {
        const short2_t a = __builtin_bit_cast(short2_t, xs[lw(lb + q)]);
        e -= (uint32_t)__builtin_amdgcn_sdot2(a, a, 0, false);
    }
    for (int r = 0; r < kCR; ++r) {
        const long k = k0 + lb + r;
        if (r > 0) {  // E_{k} = E_{k-1} + |x_k|^2 - |x_{k-N}|^2 (phase stream)
            const uint32_t xn = xs[lw(lb + r + NP - 1)], xo = xs[lw(lb + r - 1 + pad)];
            const short2_t a = __builtin_bit_cast(short2_t, xn), b = __builtin_bit_cast(short2_t, xo);
            e += (uint32_t)__builtin_amdgcn_sdot2(a, a, 0, false) - (uint32_t)__builtin_amdgcn_sdot2(b, b, 0, false);
        }
        if (k < ke) {
            const long i = k * S + ph;
            const int32_t sr = ar[r] >> (cs & 31u), si = ai[r] >> (cs & 31u);
            const int32_t qr = sr >> 2, qi = si >> 2;
            corr_out[i] = (uint32_t)qr * (uint32_t)qr + (uint32_t)qi * (uint32_t)qi;
            en_out[i] = e >> ((unsigned)((int)cs / 2) & 31u);
        }
    }
}

// ------------------------------------ S == 1: one launch, detection fused
// corr_scan_tile (corr_scan_kernels.h) on tile blockIdx.x of the one channel
__global__ __launch_bounds__(kCBlock, SRCDSP_CORR_MINW) void corr_scan_s1(const uint32_t *__restrict__ in, long n,
                                                         const uint32_t *__restrict__ hist,
                                                         const uint32_t *__restrict__ ptaps, int N, int NP, unsigned cs,
                                                         uint32_t c_prev0, uint32_t c_prev1, uint32_t e_prev0,
                                                         unsigned *best) {
    corr_scan_tile(in, n, hist, ptaps, N, NP, cs, c_prev0, c_prev1, e_prev0, best, (long)blockIdx.x);
}

__global__ void corr_detect(const uint32_t *__restrict__ corr, const uint32_t *__restrict__ en, long i_begin,
                            long i_end, uint32_t c_prev0, uint32_t c_prev1, uint32_t e_prev0, unsigned *best) {
    // skip when an EARLIER segment detected (a hit of this segment is >= i_begin,
    // so blocks of this launch never stop each other)
    if ((long)*(volatile unsigned *)best < i_begin) return;
    for (long i = i_begin + (long)blockIdx.x * blockDim.x + threadIdx.x; i < i_end;
         i += (long)gridDim.x * blockDim.x) {
        const uint32_t c0 = corr[i];
        const uint32_t c1 = i >= 1 ? corr[i - 1] : c_prev0;
        const uint32_t c2 = i >= 2 ? corr[i - 2] : (i == 1 ? c_prev0 : c_prev1);
        const uint32_t e1 = i >= 1 ? en[i - 1] : e_prev0;
        if (corr_hit(c2, c1, c0, e1)) atomicMin(best, (unsigned)i);
    }
}

// the end of every single-channel step and of priming: corr_tail (corr_tail.h)
// at *best, the history and bitSamples copies spread over the grid
struct CorrPrev {
    uint32_t w[6];  // corr[0..2], energy[0..2] carried from the previous call
};
__global__ __launch_bounds__(kCorrTailBlock) void corr_step_tail(const uint32_t *__restrict__ in, long n,
                                                                 const uint32_t *__restrict__ hist,
                                                                 uint32_t *__restrict__ hist_out,
                                                                 const int32_t *__restrict__ coef, unsigned N,
                                                                 unsigned S, unsigned cs, const CorrPrev prev,
                                                                 const unsigned *__restrict__ best,
                                                                 uint32_t *__restrict__ row,
                                                                 uint32_t *__restrict__ bits) {
    corr_tail(in, n, hist, hist_out, coef, N, S, cs, prev.w, *best, row, bits, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------- host side
// scan = false: stream the samples with no detection test (corr_prime): no
// scan at all, `best` stays kCorrNone and the tail leaves the registers and
// the history of the last sample.
// trace (CREATE_DEBUG_FILES, correlators.h:253-257): host arrays of n_
// entries receive corrValue[0] / energyValue[0] after each processed sample
// (*trace_n of them: corrIndex + 2 on a detection, else n_); the segmented
// kernels run, since only they keep per-sample values.
struct CorrTrace {
    uint32_t *corr = nullptr, *energy = nullptr;
    size_t *count = nullptr;
};

static int corr_run(srcdsp_corr_state &c, const uint32_t *d_in, size_t n_, int *found, int *corr_index,
                    hipStream_t s, bool scan = true, const CorrTrace *trace = nullptr) {
    *found = 0;
    if (trace) *trace->count = 0;
    if (n_ == 0) return SRCDSP_OK;
    const long n = (long)n_;
    if (n > 0x7fffffffL) {
        set_error("corr_step: input longer than INT_MAX samples (correlators.h:212 uses int)");
        return SRCDSP_ERR_SIZE;
    }
    // the tail's results: a result row and a bitSamples row on the device, and their pinned mirror
    int rc = c.bank.reserve(4 * (kCorrRow + (size_t)c.N));
    if (rc) return rc;
    uint32_t *const d_row = c.bank.dev<uint32_t>(), *const d_bits = d_row + kCorrRow;
    uint32_t *const h_row = c.bank.host<uint32_t>(), *const h_bits = h_row + kCorrRow;
    rc = c.order.before(s);
    if (rc) return rc;
    const long NSm1 = (long)c.NS - 1;
    const uint32_t *hist = c.d_hist[c.cur];
    const unsigned cs = (unsigned)c.coeff_scaling;
    // dot2 tiles for int16-range patterns (48 <= N <= kCorrDot2MaxTaps at
    // S > 1: below 48 taps there the strided staging costs more than the taps,
    // 0.277 vs 0.468 ms at N = 31, S = 3 on 2^24 samples); at S = 1 (config 5
    // and every N <= kCorrDot2MaxTaps) one launch scans with detection fused
    const bool dot2 = c.taps16 && c.NP <= kCorrDot2MaxTaps && c.S <= kCorrMaxGridY &&
                      (c.N >= 48 || c.S == 1);
    // the fused scan keeps no per-sample values, which a trace needs: the
    // segmented kernels write corr/energy per sample for corr_detect
    const bool fused = dot2 && c.S == 1 && !trace;
    if (scan && !fused) {
        rc = c.corr_vals.reserve(4 * n_);
        if (!rc) rc = c.en_vals.reserve(4 * n_);
        if (rc) return rc;
    }
    uint32_t *const d_corr = c.corr_vals.dev<uint32_t>(), *const d_en = c.en_vals.dev<uint32_t>();
    SRCDSP_HIP_TRY(hipMemsetAsync(c.d_best, 0xff, 4, s));
    if (scan && fused) {  // one launch, detection fused, in-flight early exit
        constexpr long TO = (long)kCBlock * kCR;
        const long blocks = (n + TO - 1) / TO;
        const size_t smem = 4 * (size_t)corr_scan_lds_words((int)c.NP);
        hipLaunchKernelGGL(corr_scan_s1, dim3((unsigned)blocks), dim3(kCBlock), smem, s, d_in, n, hist, c.d_ptaps,
                           (int)c.N, (int)c.NP, cs, c.corr[0], c.corr[1], c.energy[0], c.d_best);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    // The segmented path: S > 1, patterns past the int16 range or past
    // kCorrDot2MaxTaps taps, and the traces.
    // The reference stops at the first detection (break, correlators.h:291).
    // All segments are queued at once; each launch returns at its start when
    // an earlier segment's detect kernel has recorded a hit, so the scan stops
    // one segment after the detection with no host round trip in between.
    const long seg = std::max<long>(1L << 22, (n + 15) / 16);
    for (long sb = scan && !fused ? 0 : n; sb < n; sb += seg) {
        const long se = std::min(n, sb + seg);
        if (dot2) {  // grid.y = phase of the stride
            constexpr long TO = (long)kCBlock * kCR;
            const long per_phase = (se - sb + c.S - 1) / c.S;
            const long blocks = (per_phase + TO - 1) / TO;
            const size_t smem = 4 * (size_t)corr_lds_words((int)c.NP);
            hipLaunchKernelGGL(corr_eval_dot2, dim3((unsigned)blocks, c.S), dim3(kCBlock), smem, s, d_in, n, sb, se,
                               hist, c.d_ptaps, (int)c.N, (int)c.NP, (int)c.S, cs, d_corr, d_en,
                               (const unsigned *)c.d_best);
        } else {
            const size_t smem = 4 * (size_t)((kCorrBlock + NSm1 + 3) & ~3l) + 8 * (size_t)c.N;
            const long blocks = (se - sb + kCorrBlock - 1) / kCorrBlock;
            if (smem <= kCorrEvalMaxSmem)
                hipLaunchKernelGGL(corr_eval, dim3((unsigned)blocks), dim3(kCorrBlock), smem, s, d_in, n, sb, se, hist,
                                   c.d_coef, c.N, c.S, cs, d_corr, d_en, (const unsigned *)c.d_best);
            else
                hipLaunchKernelGGL(corr_eval_g, dim3((unsigned)blocks), dim3(kCorrBlock), 0, s, d_in, n, sb, se, hist,
                                   c.d_coef, c.N, c.S, cs, d_corr, d_en, (const unsigned *)c.d_best);
        }
        SRCDSP_HIP_TRY(hipGetLastError());
        const int db = (int)std::max<long>(1, std::min<long>((se - sb + 255) / 256, 4096));
        hipLaunchKernelGGL(corr_detect, dim3(db), dim3(256), 0, s, d_corr, d_en, sb, se, c.corr[0], c.corr[1],
                           c.energy[0], c.d_best);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    // the tail: workgroup 0 the registers and the row, all of them the history and bitSamples copies
    const CorrPrev prev{{c.corr[0], c.corr[1], c.corr[2], c.energy[0], c.energy[1], c.energy[2]}};
    const long copy = std::max<long>(NSm1, c.N);
    const unsigned tb = (unsigned)std::min<long>((copy + kCorrTailBlock - 1) / kCorrTailBlock, 1024);
    hipLaunchKernelGGL(corr_step_tail, dim3(tb), dim3(kCorrTailBlock), 0, s, d_in, n, hist, c.d_hist[c.cur ^ 1],
                       (const int32_t *)c.d_coef, c.N, c.S, cs, prev, (const unsigned *)c.d_best, d_row, d_bits);
    SRCDSP_HIP_TRY(hipGetLastError());
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_row, d_row, 4 * kCorrRow, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    const bool hit = h_row[0] != kCorrNone;
    if (hit) SRCDSP_HIP_TRY(hipMemcpyAsync(h_bits, d_bits, 4 * (size_t)c.N, hipMemcpyDeviceToHost, s));
    if (trace) {  // every processed sample's registers (the segmented kernels computed them all up to `last`)
        const size_t cnt = hit ? (size_t)h_row[0] + 1 : n_;
        SRCDSP_HIP_TRY(hipMemcpyAsync(trace->corr, d_corr, 4 * cnt, hipMemcpyDeviceToHost, s));
        SRCDSP_HIP_TRY(hipMemcpyAsync(trace->energy, d_en, 4 * cnt, hipMemcpyDeviceToHost, s));
        *trace->count = cnt;
    }
    if (hit || trace) SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    return corr_commit(c, h_row, h_bits, found, corr_index, s);
}

}  // namespace srcdsp

using namespace srcdsp;

// The build's test switches, reported by a kernel of this library (so a
// process holding two copies of the library -- the product and a test build,
// tests/test_gpu_corr_hit.py -- can tell which copy's kernels a call ran).
__global__ void corr_build_flags_kernel(unsigned *out) {
    if (threadIdx.x == 0) {
#ifdef SRCDSP_CORR_ALWAYS_EXACT
        *out = SRCDSP_BUILD_CORR_ALWAYS_EXACT;
#else
        *out = 0u;
#endif
    }
}

extern "C" {

SRCDSP_API int srcdsp_build_flags(unsigned *flags) {
    SRCDSP_ARG_CHECK(flags != nullptr, "build_flags: null flags");
    unsigned *d = nullptr;
    if (hipMalloc(&d, sizeof(unsigned)) != hipSuccess) {
        set_error("build_flags: device allocation failed");
        return SRCDSP_ERR_HIP;
    }
    hipLaunchKernelGGL(corr_build_flags_kernel, dim3(1), dim3(64), 0, nullptr, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(flags, d, sizeof(unsigned), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) {
        set_error(hipGetErrorString(e));
        return SRCDSP_ERR_HIP;
    }
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_corr_create(srcdsp_corr_t *out, unsigned N, unsigned S) {
    SRCDSP_ARG_CHECK(out != nullptr, "corr_create: null out");
    *out = nullptr;
    SRCDSP_ARG_CHECK(N >= 1 && S >= 1 && (unsigned long)N * S <= (1ul << 24), "corr_create: bad N/S");
    auto *h = new srcdsp_corr();
    srcdsp_corr_state &c = h->c;
    c.N = N;
    c.S = S;
    c.NS = N * S;
    c.NP = (N + 15) / 16 * 16;
    c.h_coef.assign(2 * N, 0);
    c.bits.assign(2 * N, 0);
    int rc = c.order.init();
    if (!rc) rc = c.stage.init();
    if (rc) {
        delete h;
        return rc;
    }
    const size_t hb = 4 * (size_t)std::max(1u, c.NS - 1);
    if (hipMalloc(&c.d_coef, 8 * (size_t)N) != hipSuccess || hipMemset(c.d_coef, 0, 8 * (size_t)N) != hipSuccess ||
        hipMalloc(&c.d_ptaps, 8 * (size_t)c.NP) != hipSuccess || hipMemset(c.d_ptaps, 0, 8 * (size_t)c.NP) != hipSuccess ||
        hipMalloc(&c.d_hist[0], hb) != hipSuccess || hipMalloc(&c.d_hist[1], hb) != hipSuccess ||
        hipMemset(c.d_hist[0], 0, hb) != hipSuccess || hipMalloc(&c.d_best, 4) != hipSuccess) {
        set_error("corr_create: device allocation failed");
        srcdsp_corr_destroy(h);
        return SRCDSP_ERR_HIP;
    }
    *out = h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_corr_destroy(srcdsp_corr_t h) {
    if (!h) return SRCDSP_OK;
    srcdsp_corr_state &c = h->c;
    (void)c.order.sync();
    for (void *p : {(void *)c.d_coef, (void *)c.d_ptaps, (void *)c.d_hist[0], (void *)c.d_hist[1], (void *)c.d_best})
        if (p) (void)hipFree(p);
    c.corr_vals.destroy();
    c.en_vals.destroy();
    c.bank.destroy();
    c.order.destroy();
    c.stage.destroy();
    delete h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_corr_clone(srcdsp_corr_t h, srcdsp_corr_t *out) {
    SRCDSP_ARG_CHECK(h != nullptr && out != nullptr, "corr_clone: null argument");
    *out = nullptr;
    srcdsp_corr_state &s = h->c;
    int rc = s.order.sync();
    if (rc) return rc;
    srcdsp_corr_t n = nullptr;
    rc = srcdsp_corr_create(&n, s.N, s.S);
    if (rc) return rc;
    srcdsp_corr_state &c = n->c;
    c.h_coef = s.h_coef;
    c.taps16 = s.taps16;
    for (int k = 0; k < 3; ++k) {
        c.energy[k] = s.energy[k];
        c.corr[k] = s.corr[k];
    }
    c.coeffs_energy = s.coeffs_energy;
    c.coeff_scaling = s.coeff_scaling;
    c.threshold_factor = s.threshold_factor;
    c.bits = s.bits;
    const size_t hb = 4 * (size_t)std::max(1u, s.NS - 1);
    if (hipMemcpy(c.d_coef, s.d_coef, 8 * (size_t)s.N, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(c.d_ptaps, s.d_ptaps, 8 * (size_t)s.NP, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(c.d_hist[0], s.d_hist[s.cur], hb, hipMemcpyDeviceToDevice) != hipSuccess) {
        srcdsp_corr_destroy(n);
        set_error("corr_clone: device copy failed");
        return SRCDSP_ERR_HIP;
    }
    c.cur = 0;
    *out = n;
    return SRCDSP_OK;
}

// setPattern (correlators.h:167-194)
SRCDSP_API int srcdsp_corr_set_pattern(srcdsp_corr_t h, const int32_t *p, double th) {
    SRCDSP_ARG_CHECK(h != nullptr && p != nullptr, "corr_set_pattern: null argument");
    srcdsp_corr_state &c = h->c;
    double tmp = 0;
    for (unsigned i = 0; i < c.N; ++i) {
        const int32_t re = p[2 * i], im = (int32_t)(0u - (uint32_t)p[2 * i + 1]);  // conjugate
        c.h_coef[2 * i] = re;
        c.h_coef[2 * i + 1] = im;
        tmp += (double)(int32_t)((uint32_t)re * (uint32_t)re + (uint32_t)im * (uint32_t)im);
    }
    if (!(tmp <= 1073217600)) {
        set_error("setPattern: pattern energy above 1073217600 (correlators.h:185 assert)");
        return SRCDSP_ERR_ARG;
    }
    int rc = c.order.sync();
    if (rc) return rc;
    c.coeffs_energy = (uint32_t)(uint64_t)(int64_t)tmp;
    c.threshold_factor = th * std::sqrt((double)c.coeffs_energy);
    c.coeff_scaling = cvt_d2i_x86(std::floor(std::log2(std::sqrt((double)c.coeffs_energy))));
    SRCDSP_HIP_TRY(hipMemcpy(c.d_coef, c.h_coef.data(), 8 * (size_t)c.N, hipMemcpyHostToDevice));
    c.taps16 = true;
    std::vector<uint32_t> pk(2 * (size_t)c.NP, 0u);  // front-padded with NP - N zero taps
    for (unsigned i = 0; i < c.N; ++i) {
        const int32_t pr = p[2 * i], pi = p[2 * i + 1];
        if (pr < -32767 || pr > 32767 || pi < -32767 || pi > 32767) c.taps16 = false;
        const size_t m = (size_t)(c.NP - c.N) + i;
        pk[2 * m] = ((uint32_t)pr & 0xffffu) | ((uint32_t)pi << 16);       // Re = x.re*p.re + x.im*p.im
        pk[2 * m + 1] = ((uint32_t)(-pi) & 0xffffu) | ((uint32_t)pr << 16);  // Im = -x.re*p.im + x.im*p.re
    }
    SRCDSP_HIP_TRY(hipMemcpy(c.d_ptaps, pk.data(), 8 * (size_t)c.NP, hipMemcpyHostToDevice));
    return SRCDSP_OK;
}

// reset (correlators.h:146-159): registers, history and bitSamples cleared
SRCDSP_API int srcdsp_corr_reset(srcdsp_corr_t h) {
    SRCDSP_ARG_CHECK(h != nullptr, "corr_reset: null handle");
    srcdsp_corr_state &c = h->c;
    int rc = c.order.sync();
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) c.energy[k] = c.corr[k] = 0;
    std::fill(c.bits.begin(), c.bits.end(), 0);
    const size_t hb = 4 * (size_t)std::max(1u, c.NS - 1);
    // on the handle's own stream: no wait on other streams' work
    SRCDSP_HIP_TRY(hipMemsetAsync(c.d_hist[c.cur], 0, hb, c.stage.stream));
    SRCDSP_HIP_TRY(hipStreamSynchronize(c.stage.stream));
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_corr_prime(srcdsp_corr_t h, const void *d_in, size_t n, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && (d_in != nullptr || n == 0), "corr_prime: null argument");
    int found = 0, idx = 0;
    return corr_run(h->c, (const uint32_t *)d_in, n, &found, &idx, (hipStream_t)stream, false);
}

SRCDSP_API int srcdsp_corr_step(srcdsp_corr_t h, const void *d_in, size_t n, int *found, int *corr_index,
                                void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && found != nullptr && corr_index != nullptr, "corr_step: null argument");
    SRCDSP_ARG_CHECK(d_in != nullptr || n == 0, "corr_step: null input");
    return corr_run(h->c, (const uint32_t *)d_in, n, found, corr_index, (hipStream_t)stream);
}

SRCDSP_API int srcdsp_corr_step_host(srcdsp_corr_t h, const void *in, size_t n, int *found, int *corr_index) {
    SRCDSP_ARG_CHECK(h != nullptr && found != nullptr && corr_index != nullptr, "corr_step_host: null argument");
    *found = 0;
    if (n == 0) return SRCDSP_OK;
    srcdsp_corr_state &c = h->c;
    const int rc = corr_stage_in(c, in, n);
    if (rc) return rc;
    return corr_run(c, (const uint32_t *)c.stage.d_buf, n, found, corr_index, c.stage.stream);
}

SRCDSP_API int srcdsp_corr_step_trace(srcdsp_corr_t h, const void *d_in, size_t n, int *found, int *corr_index,
                                      uint32_t *corr_out, uint32_t *energy_out, size_t *count, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && found != nullptr && corr_index != nullptr && count != nullptr,
                     "corr_step_trace: null argument");
    SRCDSP_ARG_CHECK(d_in != nullptr || n == 0, "corr_step_trace: null input");
    SRCDSP_ARG_CHECK(n == 0 || (corr_out != nullptr && energy_out != nullptr), "corr_step_trace: null trace array");
    const CorrTrace t{corr_out, energy_out, count};
    return corr_run(h->c, (const uint32_t *)d_in, n, found, corr_index, (hipStream_t)stream, true, &t);
}

SRCDSP_API int srcdsp_corr_step_host_trace(srcdsp_corr_t h, const void *in, size_t n, int *found, int *corr_index,
                                           uint32_t *corr_out, uint32_t *energy_out, size_t *count) {
    SRCDSP_ARG_CHECK(h != nullptr && found != nullptr && corr_index != nullptr && count != nullptr,
                     "corr_step_host_trace: null argument");
    SRCDSP_ARG_CHECK(n == 0 || (in != nullptr && corr_out != nullptr && energy_out != nullptr),
                     "corr_step_host_trace: null argument");
    *found = 0;
    *count = 0;
    if (n == 0) return SRCDSP_OK;
    srcdsp_corr_state &c = h->c;
    const int rc = corr_stage_in(c, in, n);
    if (rc) return rc;
    const CorrTrace t{corr_out, energy_out, count};
    return corr_run(c, (const uint32_t *)c.stage.d_buf, n, found, corr_index, c.stage.stream, true, &t);
}

SRCDSP_API int srcdsp_corr_get_bit_samples(srcdsp_corr_t h, int16_t *bits) {
    SRCDSP_ARG_CHECK(h != nullptr && bits != nullptr, "corr_get_bit_samples: null argument");
    memcpy(bits, h->c.bits.data(), 4 * (size_t)h->c.N);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_corr_get_status(srcdsp_corr_t h, uint32_t *e3, uint32_t *c3, uint32_t *ce, int *cs,
                                      double *tf) {
    SRCDSP_ARG_CHECK(h != nullptr, "corr_get_status: null handle");
    const srcdsp_corr_state &c = h->c;
    for (int k = 0; k < 3; ++k) {
        if (e3) e3[k] = c.energy[k];
        if (c3) c3[k] = c.corr[k];
    }
    if (ce) *ce = c.coeffs_energy;
    if (cs) *cs = c.coeff_scaling;
    if (tf) *tf = c.threshold_factor;
    return SRCDSP_OK;
}

}  // extern "C"
