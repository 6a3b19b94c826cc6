// corr_scan_kernels.h -- the fused S == 1 correlator scan as device functions,
// shared by corr_scan_s1 (corr.hip, one channel per launch), corr_bank_s1
// (corr_bank.hip, one channel per grid row) and corr_all_map (corr_all.hip).
// The scan stores no per-sample values: the registers after it are the tail's
// (corr_tail.h).
#pragma once
#include <algorithm>

#include "corr_state.h"
#include "fir_device.h"
#include "corr_hit.h"

namespace srcdsp {

// ------------------------------------ S == 1: one launch, detection fused
// corr_eval_dot2's arithmetic at S = 1 (taps front-padded to NP) over the whole call in ONE launch, with the
// peak/threshold test of correlators.h:262-268 evaluated by each block on its
// own 4096 outputs and reduced to the first hit with atomicMin(best).
//  * the test at a block's first two outputs needs corr/energy of the two
//    samples before it: wave 0 computes those two outputs itself (16 taps per
//    lane from L2, wave reduction), or takes the previous call's registers at
//    index 0;
//  * a block whose first output lies past a recorded hit returns at once, and
//    a running block re-reads `best` every 256 taps and stops computing once
//    a hit before it is known -- the scan ends near the first detection, as
//    the reference's `break` does, with no host round trip.
__device__ __forceinline__ uint32_t corr_value(int32_t ar, int32_t ai, unsigned cs) {
    const int32_t sr = ar >> (cs & 31u), si = ai >> (cs & 31u);  // scale32 :244
    const int32_t qr = sr >> 2, qi = si >> 2;                    // :250
    return (uint32_t)qr * (uint32_t)qr + (uint32_t)qi * (uint32_t)qi;
}

__device__ __forceinline__ unsigned load_best(const unsigned *best) {
    return __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One tile (outputs tile * 4096 .. + 4095) of one channel's scan: `in`, `hist`,
// `ptaps`, the carried registers and `best` are that channel's, all
// block-uniform.  Dynamic LDS: corr_scan_lds_words(NP) words.
// kAll (corr_all.hip's candidate pass): no early exit and no `best`; every
// output is tested and each lane stores the 16-bit mask of its 16 outputs
// (bit r: the test fires at output i0 + 16 t + r) at map[tile * kCBlock + t].
template <bool kAll = false>
__device__ __forceinline__ void corr_scan_tile(const uint32_t *__restrict__ in, long n,
                                               const uint32_t *__restrict__ hist,
                                               const uint32_t *__restrict__ ptaps, int N, int NP, unsigned cs,
                                               uint32_t c_prev0, uint32_t c_prev1, uint32_t e_prev0, unsigned *best,
                                               long tile, uint16_t *__restrict__ map = nullptr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t xs[];
    __shared__ uint32_t prev_c[kCBlock + 1][2], prev_e[kCBlock + 1];
    __shared__ unsigned dead_any, best0;
    constexpr int TO = kCBlock * kCR;
    const long i0 = tile * TO;  // first output of the tile
    if constexpr (!kAll) {
        if (threadIdx.x == 0) best0 = load_best(best);
        __syncthreads();
        if ((long)best0 < i0) return;  // a hit before this tile is already known (block-uniform)
    }
    // taps front-padded with NP - N zero taps (NP = 16 ceil(N/16), as corr_eval_dot2)
    const int pad = NP - N;
    // tile sample l (input word i0 - (NP - 1) + l, l = 0 .. TO + NP - 2) -> LDS word
    // lp + 4 (lp / 16), lp = l + 1: chunks of 16 samples + 4 pad words
    // Staging by 16-B granules: LDS chunk c (20 words, the last 4 padding)
    // holds tile samples 16c - 1 .. 16c + 14, i.e. input words j0 + 16c + 4q +
    // (0..3), j0 = i0 - NP: 16-aligned, so an aligned input is read with one
    // dwordx4 per granule; granules that reach before sample 0 or past n, and
    // misaligned inputs, go word by word (history before 0, zeros past n).
    // The alignment is the channel row's own (rows of a bank may differ).
    const int NC = (TO + NP) / kCR;  // chunks: tile samples -1 .. TO + NP - 2
    const long j0 = i0 - NP;
    const bool al16 = ((uintptr_t)in & 15u) == 0;
    uint4 *xs4 = (uint4 *)xs;
    for (int gq = threadIdx.x; gq < 4 * NC; gq += kCBlock) {
        const int c = gq >> 2, q = gq & 3;
        const long j = j0 + 16L * c + 4 * q;
        uint4 v;
        if (al16 && j >= 0 && j + 4 <= n) {
            v = *(const uint4 *)(in + j);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long jk = j + k;
                w[k] = jk < n ? (jk >= 0 ? in[jk] : (jk + (N - 1) >= 0 ? hist[jk + (N - 1)] : 0u)) : 0u;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        xs4[5 * c + q] = v;
    }
    if (threadIdx.x == 0) dead_any = 0;
    __syncthreads();
    const int t = threadIdx.x;
    int32_t ar[kCR], ai[kCR];
#pragma unroll
    for (int r = 0; r < kCR; ++r) ar[r] = ai[r] = 0;
    int32_t e0 = 0;
    const int lb = t * kCR;
    // The window energy of each lane's first output from 16-sample chunk sums
    // instead of one dot2(x, x) per tap beside the 32 correlation dot2.  Lane
    // t's window is tile samples lb .. lb + NP - 1 (lb = 16 t); LDS chunks
    // t .. t + NP/16 - 1 hold samples lb - 1 .. lb + NP - 2, so the sum of their
    // chunk sums, less |x[lb - 1]|^2, plus |x[lb + NP - 1]|^2 (word 0 of chunk
    // t + NP/16).  A chunk sum reads its chunk as 4 ds_read_b128 (conflict-free
    // at the 80-B chunk stride).  Wrap-around uint32 sums: equal to the direct sum.
    {
        uint32_t *csum = xs + corr_lds_words(NP);  // kCBlock + NP/16 words (dynamic, sized by the host)
        const int NCk = NP / 16;
        auto sq = [](uint32_t w) {
            const short2_t a = __builtin_bit_cast(short2_t, w);
            return (uint32_t)__builtin_amdgcn_sdot2(a, a, 0, false);
        };
        for (int g = t; g < kCBlock + NCk - 1; g += kCBlock) {
            uint32_t sg = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
                u4v_t v = *(const u4v_t *)&xs4[5 * g + q];
                asm volatile("" : "+v"(v));  // one ds_read_b128 (not 4-B pieces, 4-way conflicting at the 80-B stride)
                sg += sq(v.x) + sq(v.y) + sq(v.z) + sq(v.w);
            }
            csum[g] = sg;
        }
        __syncthreads();
        uint32_t eu = sq(xs[20 * (t + NCk)]) - sq(xs[20 * t]);
        for (int g = 0; g < NCk; ++g) eu += csum[t + g];
        e0 = (int32_t)eu;
    }
    // Each 16-tap chunk reads its whole 31-word window from LDS (LDS chunks
    // c0 = t + m0/16 and c0 + 1: 8 ds_read_b128, words j = -1 .. 30 of the
    // lane window) instead of carrying the previous chunk's 15 words in
    // registers: the carried words came back from the compiler's early reads
    // through 15 v_mov per 32 taps, the extra reads cost LDS slots only.
    ConstPtr<uint32_t> tp = const_view<uint32_t>(ptaps);
    auto chunk = [&](int m0) {
        asm volatile("" : "+s"(tp));
        uint32_t pw[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) pw[k] = tp[2 * m0 + k];
        const uint4 *src = (const uint4 *)xs + 5 * (t + (m0 >> 4));
        uint32_t W[32];  // W[j + 1] = window word j
        typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            // chunk c0 granules 0..3, chunk c0 + 1 granules 0..3; each a whole
            // ds_read_b128 (W[0] is unused: left alone the compiler reads chunk
            // c0 as 4-B pieces, which the 80-B lane stride does not spread)
            u4v_t q = *(const u4v_t *)(src + (g < 4 ? g : g + 1));
            asm volatile("" : "+v"(q));
            W[4 * g + 0] = q.x;
            W[4 * g + 1] = q.y;
            W[4 * g + 2] = q.z;
            W[4 * g + 3] = q.w;
        }
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const uint32_t p0 = pw[2 * mm], p1 = pw[2 * mm + 1];
#pragma unroll
            for (int r = 0; r < kCR; ++r) {
                const short2_t x = __builtin_bit_cast(short2_t, W[mm + r + 1]);
                ar[r] = __builtin_amdgcn_sdot2(x, __builtin_bit_cast(short2_t, p0), ar[r], false);
                ai[r] = __builtin_amdgcn_sdot2(x, __builtin_bit_cast(short2_t, p1), ai[r], false);
            }
        }
    };
    bool dead = false;
    for (int m0 = 0, it = 0; m0 < NP; m0 += 16, ++it) {  // NP % 16 == 0
        chunk(m0);
        if (!kAll && (it & 15) == 15) {  // every 256 taps: has a hit before this tile been found?
            const unsigned bb = __builtin_amdgcn_readfirstlane(load_best(best));
            if ((long)bb < i0) {
                dead = true;
                break;
            }
        }
    }
    // the two outputs before the tile (for the test at its first two indices)
    if (t < 64) {
        uint32_t ex_c[2] = {c_prev0, c_prev1}, ex_e = e_prev0;
        if (i0 > 0 && !dead) {
            int32_t r1 = 0, q1 = 0, r2 = 0, q2 = 0, en1 = 0;
            for (int m = t; m < N; m += 64) {  // output i0-1-u: sample i0-1-u-(N-1)+m
                const uint32_t xa = corr_fetch(in, hist, i0 - N + m, N - 1);      // u = 0
                const uint32_t xb = corr_fetch(in, hist, i0 - N - 1 + m, N - 1);  // u = 1
                const short2_t sa = __builtin_bit_cast(short2_t, xa), sb = __builtin_bit_cast(short2_t, xb);
                const short2_t p0 = __builtin_bit_cast(short2_t, (uint32_t)tp[2 * (m + pad)]);
                const short2_t p1 = __builtin_bit_cast(short2_t, (uint32_t)tp[2 * (m + pad) + 1]);
                r1 = __builtin_amdgcn_sdot2(sa, p0, r1, false);
                q1 = __builtin_amdgcn_sdot2(sa, p1, q1, false);
                r2 = __builtin_amdgcn_sdot2(sb, p0, r2, false);
                q2 = __builtin_amdgcn_sdot2(sb, p1, q2, false);
                en1 = __builtin_amdgcn_sdot2(sa, sa, en1, false);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                r1 += __shfl_xor(r1, off);
                q1 += __shfl_xor(q1, off);
                r2 += __shfl_xor(r2, off);
                q2 += __shfl_xor(q2, off);
                en1 += __shfl_xor(en1, off);
            }
            ex_c[0] = corr_value(r1, q1, cs);
            ex_c[1] = corr_value(r2, q2, cs);
            ex_e = (uint32_t)en1 >> ((unsigned)((int)cs / 2) & 31u);
        }
        if (t == 0) {
            prev_c[0][0] = ex_c[0];
            prev_c[0][1] = ex_c[1];
            prev_e[0] = ex_e;
        }
    }
    // this lane's correlation values and (sliding) energies, tested as they are
    // formed: outputs 2..15 need only the lane's own values, so only outputs 0
    // and 1 (which need the previous lane's last values) wait for the barrier,
    // and three values per lane live across it instead of 32 (at 5 waves per
    // SIMD the 32 spilled to scratch: 2.25 x the algorithmic HBM bytes)
    // LDS words of the sliding energy, from per-lane bases (no per-output
    // index arithmetic): the sample entering output r's window is tile sample
    // lb + r + NP - 1, word 20 (t + NP/16) + r; the one leaving is tile sample
    // lb + r - 1 + pad, word 20 t + q + 4 (q >> 4) with q = r + pad (uniform)
    const uint32_t *xn_base = xs + 20 * (t + NP / 16), *xo_base = xs + 20 * t;
    auto xo_word = [&](int q) { return xo_base[q + 4 * (q >> 4)]; };
    uint32_t e = (uint32_t)e0;  // the direct sum ran over NP window words, the first pad before the real window
    for (int q = 0; q < pad; ++q) {  // tile samples lb .. lb + pad - 1 (q + 1 <= 15: one LDS chunk)
        const short2_t a = __builtin_bit_cast(short2_t, xo_base[q + 1]);
        e -= (uint32_t)__builtin_amdgcn_sdot2(a, a, 0, false);
    }
    // outputs of this lane inside the call: r < nrem (int compares, no 64-bit index per output)
    const int nrem = (int)std::min<long>(kCR, n - (i0 + lb));
    uint32_t c_0 = 0, c_1 = 0, e_0 = 0;  // outputs 0 and 1, for the tests after the barrier
    uint32_t cm2 = 0, cm1 = 0, em1 = 0;  // the two outputs before r, the energy before r
    int hit = -1;                        // first hit among outputs 2..15 (lane-relative)
    unsigned mask = 0;                   // kAll: every hit among the lane's outputs
#pragma unroll
    for (int r = 0; r < kCR; ++r) {
        if (r > 0) {  // E_i = E_{i-1} + |x_i|^2 - |x_{i-N}|^2
            const uint32_t xn = xn_base[r], xo = xo_word(r + pad);
            const short2_t a = __builtin_bit_cast(short2_t, xn), b = __builtin_bit_cast(short2_t, xo);
            e += (uint32_t)__builtin_amdgcn_sdot2(a, a, 0, false) - (uint32_t)__builtin_amdgcn_sdot2(b, b, 0, false);
        }
        const uint32_t c = corr_value(ar[r], ai[r], cs), ev = e >> ((unsigned)((int)cs / 2) & 31u);
        if (r == 0) {
            c_0 = c;
            e_0 = ev;
        } else if (r == 1) {
            c_1 = c;
        } else if constexpr (kAll) {
            if (r < nrem && corr_hit(cm2, cm1, c, em1)) mask |= 1u << r;
        } else if (!dead && hit < 0 && r < nrem && corr_hit(cm2, cm1, c, em1)) {
            hit = r;
        }
        cm2 = cm1;
        cm1 = c;
        em1 = ev;
    }
    prev_c[t + 1][0] = cm1;  // output 15
    prev_c[t + 1][1] = cm2;  // output 14
    prev_e[t + 1] = em1;
    if (dead) dead_any = 1;
    __syncthreads();
    if (dead_any) return;  // outputs past a known hit: nothing to record
    const uint32_t pc1 = prev_c[t][0], pc2 = prev_c[t][1], pe1 = prev_e[t];
    if constexpr (kAll) {
        if (1 < nrem && corr_hit(pc1, c_0, c_1, e_0)) mask |= 2u;
        if (0 < nrem && corr_hit(pc2, pc1, c_0, pe1)) mask |= 1u;
        map[tile * kCBlock + t] = (uint16_t)mask;
        return;
    }
    if (1 < nrem && corr_hit(pc1, c_0, c_1, e_0)) hit = 1;
    if (0 < nrem && corr_hit(pc2, pc1, c_0, pe1)) hit = 0;
    if (hit >= 0) atomicMin(best, (unsigned)(i0 + lb + hit));
}

}  // namespace srcdsp
