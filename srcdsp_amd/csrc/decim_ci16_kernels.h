// decim_ci16_kernels.h -- the persistent complex<int16_t> decimators:
// decim_stream_ci16 (|c| < 2^23 taps, v_mad_i32_i24) and decim_dot2_ci16
// (int16-range taps, v_dot2 tap pairs), both optionally with the NCO mixer
// fused into the staging pass.  See decim.hip for the semantics.
#pragma once
#include "fir_device.h"

namespace srcdsp {

// Persistent complex<int16_t> x int32-tap decimator (M = 4), optionally with
// the NCO mixer of mixers.h fused into the staging pass (config 4).
// Same skeleton as decim_stream_cf32: a 4-sample polyphase group is one
// 16-B granule (4 packed words); one pad granule per lane chunk (R even) keeps
// the lanes' ds_read_b128 conflict-free; next tile prefetched into VGPRs.
// Products c*x with |c| < 2^23 (host-checked) are exact as v_mad_i32_i24 and
// the int32 accumulation wraps like the reference's complex<int32_t>.
// For the kernel and its launcher: halo samples of NT taps (whole 4-tap
// polyphase steps) and input samples per tile.
__host__ __device__ constexpr int ci16_halo(int NT) { return 4 * ceildiv(NT, 4); }
__host__ __device__ constexpr int ci16_spt(int BLOCK, int R) { return 4 * BLOCK * R; }

template <int NT, int R, int BLOCK, bool MIX, int MINW>
__global__ __launch_bounds__(BLOCK, MINW) void decim_stream_ci16(DecimLaunch a) {
    static_assert(R % 2 == 0, "padded layout assumes an even lane chunk");
    constexpr int NQ = ci16_halo(NT) / 4;
    constexpr int TO = ci16_spt(BLOCK, R) / 4;
    constexpr int TG = TO + NQ;  // granules of 4 samples
    constexpr int PR = R;
    constexpr int KPAD = ceildiv(NQ, PR);
    constexpr int LG = TG + (TG + KPAD * PR) / PR + 1;
    constexpr int PER = ceildiv(TG, BLOCK);
    constexpr int TABMAX = MIX ? 4096 : 1;
    __shared__ uint4 lds[LG];
    __shared__ int16_t tab[TABMAX];

    const int ch = blockIdx.y;
    const uint32_t *in = (const uint32_t *)a.in + ch * a.in_stride;
    const uint32_t *hist = (const uint32_t *)a.hist_in[ch];
    uint32_t *out = (uint32_t *)a.out + ch * a.out_stride;
    const long n_in = a.n_in;
    const int H = NT - 1;
    const int t = threadIdx.x;
    const unsigned N = a.mix_N, fr = a.mix_freq;
    const long nb = gridDim.x;
    const long b = xcd_tile(blockIdx.x, nb);
    const long per = a.ntiles / nb, rem = a.ntiles % nb;
    const long t_begin = b * per + (b < rem ? b : rem);
    const long t_end = t_begin + per + (b < rem ? 1 : 0);

    if constexpr (MIX) {
        for (int i = t; i < (int)N; i += BLOCK) tab[i] = a.mix_table[i];
        __syncthreads();
    }
    auto adv = [&](unsigned p, unsigned d) { p += d; return p >= N ? p - N : p; };
    // 32-bit phase arithmetic only: (base + (k mod N) * fr) mod N with k, fr < 2^16
    auto phase_add = [&](unsigned base, unsigned k) { return (base + (k % N) * fr) % N; };
    auto mix = [&](uint32_t w, unsigned ph) { return mix_sample(w, tab, N, ph); };
    if (t_begin == 0 && t_end > 0) {  // new history = last H samples of (history ++ mixed input)
        uint32_t *ho = (uint32_t *)a.hist_out[ch];
        for (int k = t; k < H; k += BLOCK) {
            long idx = n_in - H + k;
            uint32_t w = idx >= 0 ? in[idx] : hist[H + idx];
            if constexpr (MIX)  // mix_phase_hist = phase of sample n_in - H (>= 0 whenever idx >= 0)
                if (idx >= 0) w = mix(w, idx < k ? phase_add(a.mix_phase0, (unsigned)idx)
                                                 : phase_add(a.mix_phase_hist, (unsigned)k));
            ho[k] = w;
        }
    }
    // per-lane phase offsets of the staged granules: sample b0 + 4g, g = t + i*BLOCK
    const unsigned d_lane = MIX ? phase_add(0, 4 * t) : 0;
    const unsigned d_i = MIX ? phase_add(0, 4 * BLOCK) : 0;
    // phase of a tile's first staged sample (b0 = 4*tile*TO - 4*NQ)
    auto tile_phase = [&](long tile) {
        return (a.mix_phase_tile0 + ((unsigned)(tile % N)) * a.mix_dtile) % N;
    };

    uint4 v[PER];
    auto mix4 = [&](uint4 &w, unsigned ph) {
        w.x = mix(w.x, ph); ph = adv(ph, fr);
        w.y = mix(w.y, ph); ph = adv(ph, fr);
        w.z = mix(w.z, ph); ph = adv(ph, fr);
        w.w = mix(w.w, ph);
    };
    auto stage_load = [&](long tile) {  // tile >= 1
        const long b0 = 4 * tile * TO - 4 * NQ;
        const long remb = (n_in - b0) * 4;
        const unsigned nrec = (unsigned)(remb > 0xfffffff0L ? 0xfffffff0L : (remb < 0 ? 0 : remb));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(in + b0), 0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if (g < TG) {
                auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * g, 0, 0);
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    // mix the staged words in registers before they go to LDS.  Past the input
    // end the range-checked loads returned 0, and mixing 0 gives 0, so no
    // per-lane bound checks are needed (tiles >= 1 have no negative indices).
    auto stage_mix = [&](long tile) {
        if constexpr (MIX) {
            unsigned ph = adv(tile_phase(tile), d_lane);
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (t + i * BLOCK < TG) mix4(v[i], ph);
                ph = adv(ph, d_i);
            }
        }
    };
    if (t_begin < t_end) {
        if (t_begin == 0) {  // tile 0: halo from the (already mixed) history
            const long b0 = -4 * NQ;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = t + i * BLOCK;
                const long s = b0 + 4 * (long)g;
                if (g < TG) {
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w[j] = fetch(in, hist, s + j, n_in, H);
                        if constexpr (MIX)
                            if (s + j >= 0 && s + j < n_in) w[j] = mix(w[j], phase_add(a.mix_phase0, (unsigned)(s + j)));
                    }
                    v[i] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
        } else {
            stage_load(t_begin);
        }
    }
    const int Bt = NQ + KPAD + (PR + 1) * t;
    for (long tile = t_begin; tile < t_end; ++tile) {
        SRCDSP_LDS_BARRIER();
        // mixing here (after the barrier, once the prefetch has landed) keeps
        // the compiler from hoisting it into the FMA loop (register spills)
        if (tile != 0) stage_mix(tile);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = t + i * BLOCK;
            if (g < TG) lds[g + (g - NQ + KPAD * PR) / PR] = v[i];
        }
        SRCDSP_LDS_BARRIER();
        if (tile + 1 < t_end) stage_load(tile + 1);

        ConstPtr<int32_t> tp = const_view<int32_t>(a.coef);
        asm volatile("" : "+s"(tp));
        int32_t Xr[4 * (NQ + R)], Xi[4 * (NQ + R)];
        int32_t yr[R], yi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) yr[r] = yi[r] = 0;
        auto load_group = [&](int e) {
            const uint4 g = lds[Bt + e + floordiv(e, PR)];
            const int o = 4 * e + 4 * NQ;
            Xr[o + 0] = sext16(g.x); Xi[o + 0] = sext16_hi(g.x);
            Xr[o + 1] = sext16(g.y); Xi[o + 1] = sext16_hi(g.y);
            Xr[o + 2] = sext16(g.z); Xi[o + 2] = sext16_hi(g.z);
            Xr[o + 3] = sext16(g.w); Xi[o + 3] = sext16_hi(g.w);
        };
#pragma unroll
        for (int e = -1; e < R; ++e) load_group(e);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (q + 1 < NQ) load_group(-q - 2);
            if ((q & 3) == 0) asm volatile("" : "+s"(tp));
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int k = 4 * q + p;
                if (k < NT) {
                    const int32_t c = tp[k];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int o = 4 * (r - q) - p + 4 * NQ;
                        yr[r] += __mul24(c, Xr[o]);
                        yi[r] += __mul24(c, Xi[o]);
                    }
                }
            }
        }
        const long n0 = tile * TO + (long)t * R;
        const unsigned sh = a.shift;
        if (n0 + R <= a.n_out && R == 4) {
            *(uint4 *)(out + n0) = make_uint4(pack16(limit16(yr[0], sh), limit16(yi[0], sh)),
                                              pack16(limit16(yr[1], sh), limit16(yi[1], sh)),
                                              pack16(limit16(yr[2], sh), limit16(yi[2], sh)),
                                              pack16(limit16(yr[3], sh), limit16(yi[3], sh)));
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (n0 + r < a.n_out) out[n0 + r] = pack16(limit16(yr[r], sh), limit16(yi[r], sh));
        }
    }
}

// ------------------------------------------------- ci16 x int16-range taps
// Persistent complex<int16_t> decimator (M = 4) on v_dot2_i32_i16: each dot2
// is TWO taps of one component.  The staged samples are split into a real
// and an imaginary plane of packed int16 pairs (x[2e], x[2e+1]); with the taps
// paired as P_j = (lo c[2j], hi c[2j-1]) (c[-1] = c[NT] = 0) output r of a
// lane (input sample 4r of its chunk) is
//   y_r = sum_{j=0}^{J-1} dot2(D[2r - j], P_j),  D[d] = plane dword d,
// so a lane's 4 outputs slide ONE register window down the plane by one dword
// per tap pair: 8 dot2 per pair, one ds_read_b128 per plane every 4 pairs.
// Products int16 x int16 and the int32 accumulation wrap exactly as the
// reference's complex<int32_t> arithmetic (host checks |c| <= 32767).
// Fused mixer (MIX): the LDS table holds (lo T[(k+N/4)%N], hi T[k]) = (lr, li);
// re = dot2(x, (lr, -li)), im = dot2(swap(x), (lr, li)).
// The plane layout in LDS: dot2_slot (fir_device.h).
//
// Mixer table forms (TABM; 0 = no table, the unmixed kernel):
//  1 (TAB2, any period: taken when the sequence period Pe of form 3 is above
//    4096, as for an odd N / gcd(freq, N) above 1024): the (lr, li) word of
//    phase k at k, the N-word table stored twice (2N words), so the
//    address of sample j of staged granule i is one add of a wave-uniform
//    tile/granule phase (SGPR) and a per-lane constant (4t + j)*freq mod N --
//    no per-sample modulo.  The lanes' words sit 4*freq apart: bank conflicts
//    unless freq is odd*16;
//  3 (two-word sequence table, Pe <= kSeq2Max): the words of input SAMPLE s at
//    s mod Pe (Pe = lcm(N / gcd(freq, N), 4); sample s's phase (phi0 + s*freq)
//    mod N depends on s mod Pe only), stored twice (2 Pe words), so a lane's 4
//    samples are 4 consecutive words at any freq.  Both dot2 operands of each
//    sample are stored, A = (lr, -li) in one table and B = (li, lr)
//    in a second one kSeq2Off words further: re = dot2(x, A), im = dot2(x, B)
//    with no negate or half swap per sample (two conflict-free ds_read_b128
//    per granule).  |lr|, |li| <= 16383 (the LUT's amplitude), so -li fits.
//  4 (two-word sequence table stored once, Pe <= kSeq2Off): as 3 with each
//    table held once (Pe words),
//    the granule's index m + lo (< 2 Pe) wrapped by one subtract and one min.
//  5 (two-word sequence in REGISTERS, Pe | SPT, 512 lanes): when the period
//    divides the tile's input span (config 4: N = 4096, any frequency, Pe a
//    power of two <= 4096), staged granule g = t + i BLOCK of every tile after
//    the first holds samples (4 t + (i odd ? 2048 : 0) + j - HS) mod Pe, so a
//    lane needs only 2 x 4 (A, B) word pairs: made once from the global LUT
//    into 16 VGPRs, no LDS table, no table fill, no table read per granule
//    (round 5's first form stored the table rotated by -HS in LDS and read
//    8 ds_read_b128 per lane-tile; form 4 spends 4 VALU per granule on the
//    index).  Tile 0 and the history read the global LUT per sample.
// Products via VOP3 dot2 and the pair clamp above.
constexpr int kSeq2Off = 4096, kSeq2Max = kSeq2Off / 2;
template <int NT, int BLOCK, bool MIX, int MINW, int TABM = 0, int MD = 4>
__global__ __launch_bounds__(BLOCK, MINW) void decim_dot2_ci16(DecimLaunch a) {
    static_assert(MIX ? (TABM == 1 || TABM == 3 || TABM == 4 || TABM == 5) : TABM == 0,
                  "mixer table forms 1, 3, 4, 5; none without the mixer");
    // doubled phase table; sequence tables (3, 4, 5); 4: stored once; 5: in registers
    constexpr bool TAB2 = TABM == 1, SEQT = TABM >= 3, SEQ1 = TABM == 4, SEQR = TABM == 5;
    static_assert(!SEQR || BLOCK == 512, "the rotated table's two lane bases assume 4 BLOCK = 2048 samples per round");
    constexpr bool RT = NT == 0;                  // the tap count at run time (a.ntaps <= kDot2MaxTaps)
    static_assert(MD == 1 || MD == 2 || MD == 4 || MD == 8 || MD == 16, "M dividing the 16-sample lane chunk");
    static_assert(MD == 4 || RT, "tap counts are compiled in at M = 4 only");
    constexpr int R = dot2_r(MD);                 // outputs per lane (a lane chunk: 16 samples)
    constexpr int TO = BLOCK * R;                 // outputs per tile
    constexpr int SPT = dot2_spt(BLOCK, MD);      // input samples per tile
    // compile-time geometry: the tap count's, or (RT) the largest tap count's,
    // which sizes the prefetch registers and the LDS image (its row length NC
    // then fixed, so every window read is a per-lane base plus immediates)
    constexpr int JC = dot2_pairs(NT, kDot2MaxTaps);
    constexpr int HSC = dot2_halo(NT, kDot2MaxTaps);
    constexpr int PER = ceildiv((SPT + HSC) / 4, BLOCK);
    constexpr int PG = (SPT + HSC) / 8;           // plane granules
    constexpr int NC0 = ceildiv(PG, 2);
    constexpr int NC = NC0 + ((4 - NC0 % 8) + 8) % 8;  // slots per plane row, = 4 (mod 8)
    constexpr int LSLOTS = 4 * NC;
    constexpr int TABMAX = (MIX && !SEQR) ? 8192 : 1;  // SEQR: the lane's words in registers
    static_assert(HSC % 16 == 0 && 2 * (JC - 1) <= HSC, "halo geometry");
    static_assert(BLOCK % 16 == 0, "column-major plane layout");
    // tap pairs (RT: padded with zero pairs to whole 4-pair steps), halo
    // samples (lane-chunk aligned; RT: one more plane granule pair, so the
    // window read one step ahead stays inside the image), staged granules
    const int J = RT ? dot2_pairs(NT, a.ntaps) : JC;
    const int HS = RT ? dot2_halo(NT, a.ntaps) : HSC;  // the launcher's dot2_halo(NT, ntaps)
    const int HG = HS / 8;                        // halo plane granules (even)
    const int TG = (SPT + HS) / 4;                // staged 16-B sample granules
    __shared__ uint4 lds[LSLOTS];
    __shared__ __attribute__((aligned(16))) uint32_t ctab[TABMAX];
#ifdef SRCDSP_PHASE_CLOCK
    unsigned long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 1, 0};
#endif
    SRCDSP_PH(ph_start);

    const int ch = blockIdx.y;
    const uint32_t *in = (const uint32_t *)a.in + ch * a.in_stride;
    const uint32_t *hist = (const uint32_t *)a.hist_in[ch];
    uint32_t *out = (uint32_t *)a.out + ch * a.out_stride;
    const long n_in = a.n_in;
    const int H = RT ? a.ntaps - 1 : NT - 1;
    const int t = threadIdx.x;
    const unsigned N = a.mix_N, fr = a.mix_freq;
    const long nb = gridDim.x;
    const long b = xcd_tile(blockIdx.x, nb);
    const long per = a.ntiles / nb, rem = a.ntiles % nb;
    const long t_begin = b * per + (b < rem ? b : rem);
    const long t_end = t_begin + per + (b < rem ? 1 : 0);

    const unsigned Pe = SEQT ? a.mix_pe : 1u;
    // SEQR: every tile's staged granule t + i BLOCK reads the same 4 samples'
    // table words -- index (4 t + (i odd ? 2048 : 0) + j - HS) mod Pe -- so the
    // lane keeps its two granules' words (A = (lr, -li), B = (li, lr)) in 16
    // registers, made once from the global LUT (one 64-bit modulo per parity,
    // then a phase step per sample), and no table lives in LDS
    uint32_t rA[2][4] = {}, rB[2][4] = {};
    if constexpr (MIX && SEQR) {
        const int16_t *tab = a.mix_table;
        const unsigned hs = (unsigned)((long)HS % (long)Pe);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned m = (4u * t + (h ? 2048u % Pe : 0u) + Pe - hs) % Pe;  // sample offset of word j = 0
            unsigned k = (unsigned)(((unsigned long)a.mix_phase0 + (unsigned long)m * fr) % N);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned ic = k + N / 4;
                ic = ic >= N ? ic - N : ic;
                rA[h][j] = ((uint32_t)(uint16_t)tab[ic]) | ((uint32_t)(uint16_t)(-tab[k]) << 16);
                rB[h][j] = ((uint32_t)(uint16_t)tab[k]) | ((uint32_t)(uint16_t)tab[ic] << 16);
                k += fr;
                k = k >= N ? k - N : k;
            }
        }
    }
    if constexpr (MIX && !SEQR) {
        const int16_t *tab = a.mix_table;
        const int nw = SEQ1 ? (int)Pe : SEQT ? 2 * (int)Pe : 2 * (int)N;
        // SEQT: entry i holds the phase of sample i, (phi0 + i fr) mod N --
        // periodic in Pe, so i needs no reduction; one 64-bit
        // modulo per lane, then a step of BLOCK entries is one add and one
        // conditional subtract (a modulo per entry was ~100 VALU: ~8 per wave
        // tile of config 4 over a workgroup's tiles)
        unsigned kseq = 0, kstep = 0;
        if constexpr (SEQT) {
            kseq = (unsigned)(((unsigned long)a.mix_phase0 + (unsigned long)t * fr) % N);
            kstep = (unsigned)(((unsigned long)BLOCK * fr) % N);
        }
        for (int i = t; i < nw; i += BLOCK) {
            unsigned k;
            if constexpr (SEQT) {
                k = kseq;
                kseq += kstep;
                kseq = kseq >= N ? kseq - N : kseq;
            } else {
                k = (unsigned)i < N ? (unsigned)i : (unsigned)i - N;
            }
            unsigned ic = k + N / 4;
            ic = ic >= N ? ic - N : ic;
            if constexpr (SEQT) {  // A = (lr, -li), B = (li, lr)
                ctab[i] = ((uint32_t)(uint16_t)tab[ic]) | ((uint32_t)(uint16_t)(-tab[k]) << 16);
                ctab[kSeq2Off + i] = ((uint32_t)(uint16_t)tab[k]) | ((uint32_t)(uint16_t)tab[ic] << 16);
            } else {
                ctab[i] = ((uint32_t)(uint16_t)tab[ic]) | ((uint32_t)(uint16_t)tab[k] << 16);
            }
        }
        __syncthreads();
    }
    auto adv = [&](unsigned p, unsigned d) { p += d; const unsigned q = p - N; return q < p ? q : p; };
    auto phase_add = [&](unsigned base, unsigned k) { return (base + (k % N) * fr) % N; };
    auto mix1 = [&](uint32_t w, unsigned ph) {
        int32_t re, im;
        if constexpr (SEQR) {  // no LDS table: ph is the phase itself, the words from the global LUT
            unsigned ic = ph + N / 4;
            ic = ic >= N ? ic - N : ic;
            const int16_t lr = a.mix_table[ic], li = a.mix_table[ph];
            re = clamp_s14(sdot2(w, ((uint32_t)(uint16_t)lr) | ((uint32_t)(uint16_t)(-li) << 16), 0));
            im = clamp_s14(sdot2(w, ((uint32_t)(uint16_t)li) | ((uint32_t)(uint16_t)lr << 16), 0));
        } else if constexpr (SEQT) {
            re = clamp_s14(sdot2(w, ctab[ph], 0));
            im = clamp_s14(sdot2(w, ctab[kSeq2Off + ph], 0));
        } else {
            mix_dot2(w, ctab[ph], re, im);
        }
        return pack16(re, im);
    };
    // input sample s >= 0 of this call, mixed (any table form)
    auto mix_at = [&](uint32_t w, long s) {
        if constexpr (SEQR) return mix1(w, phase_add(a.mix_phase0, (unsigned)(s % (long)N)));
        else if constexpr (SEQT) return mix1(w, (unsigned)(s % (long)Pe));
        else return mix1(w, phase_add(a.mix_phase0, (unsigned)(s % (long)N)));
    };
    if (t_begin == 0 && t_end > 0) {  // new history = last H samples of (history ++ mixed input)
        uint32_t *ho = (uint32_t *)a.hist_out[ch];
        for (int k = t; k < H; k += BLOCK) {
            long idx = n_in - H + k;
            uint32_t w = idx >= 0 ? in[idx] : hist[H + idx];
            if constexpr (MIX)
                if (idx >= 0) w = mix_at(w, idx);
            ho[k] = w;
        }
    }
    // TAB2: phase offsets of the lane's granule in a round (its first sample)
    // and of one round of BLOCK granules
    const unsigned d_lane = MIX && TAB2 ? phase_add(0, 4 * t) : 0;
    const unsigned d_i = MIX ? phase_add(0, 4 * BLOCK) : 0;
    auto tile_phase = [&](long tile) {  // phase of the tile's first staged sample tile*SPT - HS
        return (a.mix_phase_tile0 + ((unsigned)(tile % N)) * a.mix_dtile) % N;
    };

    // staged granule of round i (one 16-B granule per lane per round), -1 past the tile
    auto sg = [&](int i) { const int g = t + i * BLOCK; return g < TG ? g : -1; };
    uint4 v[PER];
    auto stage_load = [&](long tile) {  // tile >= 1
        const long b0 = (long)SPT * tile - HS;
        const long remb = (n_in - b0) * 4;
        const unsigned nrec = (unsigned)(remb > 0xfffffff0L ? 0xfffffff0L : (remb < 0 ? 0 : remb));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(in + b0), 0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = sg(i);
            if (g >= 0) {
                auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * g, 0, 0);
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    // staged granule g -> plane granule g>>1, half g&1
    auto lds_half = [&](int g, int plane) {
        const int G = g >> 1;
        return (uint2 *)&lds[dot2_slot<NC>(G, plane)] + (g & 1);
    };
    auto put = [&](int g, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
        *lds_half(g, 0) = make_uint2(lo16_pair(w0, w1), lo16_pair(w2, w3));
        *lds_half(g, 1) = make_uint2(hi16_pair(w0, w1), hi16_pair(w2, w3));
    };
    // the mixed granule's sums, clamped, into its halves of both planes
    auto put_planes = [&](int g, const int32_t (&r)[4], const int32_t (&i)[4]) {
        *lds_half(g, 0) = clamp_granule_s14(r);
        *lds_half(g, 1) = clamp_granule_s14(i);
    };
    // TAB2: per-lane byte offsets of the 4 samples of a staged granule (sample
    // 0's is d_lane, which stays ahead of d_i: in any other order the compiler
    // schedules the prologue differently from the build that was measured)
    unsigned lj[4] = {0, 0, 0, 0};
    if constexpr (MIX && TAB2)
#pragma unroll
        for (int j = 0; j < 4; ++j) lj[j] = 4u * (j == 0 ? d_lane : phase_add(0, 4 * t + j));
    auto put_mixed2 = [&](int g, uint4 w, unsigned sb) {  // sb: granule phase * 4 (uniform)
        const uint32_t *tb = ctab;
        auto ld = [&](int j) { return *(const uint32_t *)((const char *)tb + (sb + lj[j])); };
        int32_t re[4], im[4];
        mix_granule_c(w, make_uint4(ld(0), ld(1), ld(2), ld(3)), re, im);
        put_planes(g, re, im);
    };
    // SEQT: the granule's 4 words at ctab[m + lane offset], m = (first staged
    // sample of the granule row) mod Pe (uniform); lane offset 4t mod Pe
    const unsigned lo_t = SEQT ? (4u * t) % Pe : 0u;
    auto put_mixed_seq = [&](int g, uint4 w, unsigned m, unsigned lo) {
        unsigned ix = m + lo;  // < 2 Pe; a multiple of 4 words
        if constexpr (SEQ1) {
            const unsigned jx = ix - Pe;
            ix = jx < ix ? jx : ix;  // ix mod Pe (v_sub + v_min)
        }
        // one 16-B read per table (the compiler, not knowing the alignment,
        // would split it into 4-way-conflicting ds_read2_b32)
        const uint4 A = *(const uint4 *)__builtin_assume_aligned(&ctab[ix], 16);
        const uint4 B = *(const uint4 *)__builtin_assume_aligned(&ctab[kSeq2Off + ix], 16);
        int32_t re[4], im[4];
        mix_granule_ab(w, A, B, re, im);
        put_planes(g, re, im);
    };
    // SEQR: the round's parity picks the lane's register words
    auto put_mixed_seqr = [&](int g, uint4 w, int h) {
        const uint32_t(&A)[4] = rA[h];
        const uint32_t(&B)[4] = rB[h];
        int32_t re[4], im[4];
        mix_granule_ab(w, make_uint4(A[0], A[1], A[2], A[3]), make_uint4(B[0], B[1], B[2], B[3]), re, im);
        put_planes(g, re, im);
    };
    auto advp = [&](unsigned p, unsigned d) { p += d; const unsigned q = p - Pe; return q < p ? q : p; };
    // SEQT: (tile*SPT - HS) mod Pe of the workgroup's current tile
    unsigned m_tile = 0;
    if constexpr (MIX && SEQT && !SEQR)
        if (t_begin < t_end) m_tile = (unsigned)((t_begin * (long)SPT - HS + 4 * (long)Pe * (1 + HS / 4)) % (long)Pe);
    if (t_begin < t_end) {
        if (t_begin == 0) {  // tile 0: halo from the (already mixed) history; mixed here, written below
            const long b0 = -HS;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = sg(i);
                const long s0 = b0 + 4 * (long)g;
                if (g >= 0) {
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w[j] = fetch(in, hist, s0 + j, n_in, H);
                        if constexpr (MIX)
                            if (s0 + j >= 0 && s0 + j < n_in) w[j] = mix_at(w[j], s0 + j);
                    }
                    v[i] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
        } else {
            stage_load(t_begin);
        }
    }
    SRCDSP_PH(ph_loop);
    SRCDSP_PH_ADD(0, ph_loop - ph_start);
    for (long tile = t_begin; tile < t_end; ++tile) {
        SRCDSP_PH(ph0);
        SRCDSP_LDS_BARRIER();
        SRCDSP_PH(ph1);
        if (MIX && SEQR && tile != 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = sg(i);
                if (g >= 0) put_mixed_seqr(g, v[i], i & 1);
            }
        } else if (MIX && SEQT && tile != 0) {
            unsigned m = m_tile;  // wave-uniform
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = sg(i);
                if (g >= 0) put_mixed_seq(g, v[i], m, lo_t);
                m = advp(m, a.mix_pe_drow);
            }
        } else if (MIX && tile != 0) {  // the remaining form, TAB2
            unsigned sp = tile_phase(tile);  // wave-uniform
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = t + i * BLOCK;
                if (g < TG) put_mixed2(g, v[i], 4u * sp);
                sp = adv(sp, d_i);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = sg(i);
                if (g >= 0) put(g, v[i].x, v[i].y, v[i].z, v[i].w);
            }
        }
        SRCDSP_PH(ph2);
        SRCDSP_LDS_BARRIER();
        if constexpr (MIX && SEQT && !SEQR) m_tile = advp(m_tile, a.mix_pe_dtile);
        if (tile + 1 < t_end) stage_load(tile + 1);
        SRCDSP_PH(ph3);

        ConstPtr<uint32_t> tp = const_view<uint32_t>(a.coef);
        asm volatile("" : "+s"(tp));
        typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
        const unsigned sh = a.shift;
        // limitScale16 of an accumulator pair (dnsampling_filters.h:167-168);
        // Q14 taps: shift 14 (the common case), a saturating pack
        auto quant = [&](auto &yr_, auto &yi_, uint32_t *w_, int n_, int stride_) {
            if ((sh & 31u) != 0) {
#pragma unroll
                for (int k = 0; k < n_; ++k) w_[k * stride_] = limit16_pair_sh(yr_[k], yi_[k], sh);
            } else {
#pragma unroll
                for (int k = 0; k < n_; ++k) w_[k * stride_] = pack16(limit16(yr_[k], sh), limit16(yi_[k], sh));
            }
        };
        uint32_t w[R];
        if constexpr (!RT) {
            int32_t yr[R], yi[R];  // started by the first tap pair's inline-0 dot2 (no v_mov)
            // window: Dr[d + OFF], d in [-(4*NG), 8), NG = granules below the lane base
            constexpr int NG = ceildiv(JC - 1, 4);
            constexpr int OFF = 4 * NG;
            uint32_t Dr[OFF + 8], Di[OFF + 8];
            auto load_g = [&](int c) {  // plane granule lb + c -> dwords d = 4c .. 4c+3
                // granule lb + c = 2t + HG + c: row c & 1, column t + (HG + c) >> 1
                const int o = (c & 1) * NC + ((HG + c) >> 1);
                u4v_t gr = *(const u4v_t *)&lds[t + o];
                u4v_t gi = *(const u4v_t *)&lds[t + o + 2 * NC];
                // keep every read a whole ds_read_b128: at the window edges the
                // compiler would load only the words used, as ds_read2_b32 /
                // ds_read_b96, whose 4-B lane groups the layout does not spread
                asm volatile("" : "+v"(gr), "+v"(gi));
                Dr[OFF + 4 * c + 0] = gr[0]; Dr[OFF + 4 * c + 1] = gr[1]; Dr[OFF + 4 * c + 2] = gr[2]; Dr[OFF + 4 * c + 3] = gr[3];
                Di[OFF + 4 * c + 0] = gi[0]; Di[OFF + 4 * c + 1] = gi[1]; Di[OFF + 4 * c + 2] = gi[2]; Di[OFF + 4 * c + 3] = gi[3];
            };
            load_g(0);
            load_g(1);
#pragma unroll
            for (int j = 0; j < JC; ++j) {
                if ((j & 3) == 1) load_g(-1 - (j >> 2));
                if ((j & 15) == 0) asm volatile("" : "+s"(tp));
                const uint32_t P = tp[j];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (j == 0) {
                        yr[r] = sdot2_0(Dr[OFF + 2 * r], P);
                        yi[r] = sdot2_0(Di[OFF + 2 * r], P);
                    } else {
                        yr[r] = sdot2(Dr[OFF + 2 * r - j], P, yr[r]);
                        yi[r] = sdot2(Di[OFF + 2 * r - j], P, yi[r]);
                    }
                }
            }
            quant(yr, yi, w, R, 1);
        } else {
            // Run-time tap count: steps of 4 pairs.  Output r of a lane sits at
            // sample r M of the lane chunk; pair j multiplies (x[rM - 2j],
            // x[rM - 2j + 1]), i.e. plane dword rM/2 - j for even rM and, for
            // odd rM (M = 1), the odd-aligned pair built from dwords a and a+1,
            // a = (rM - 1)/2 - j, as (hi a, lo a+1) by one v_alignbit (reused
            // over the step's outputs).  Step q (pairs 4q..4q+3) reads window
            // granules -q-1 .. -q + EH/4 (EH = ceil((R-1) M/2)) and loads -q-2
            // for the next step: S >= EH/4 + 3 register slots (granule c in
            // slot c mod S, S even so granule parity is static) rotate with
            // static names over chunks of S steps (4S tap pairs, requested one
            // chunk ahead).  A chunk starting at step q0 reads granule e - q0
            // at column t + (HG - q0)/2 + floor(e/2) of row e & 1: one base per
            // chunk plus immediates.  At M = 1 (16 outputs per lane) the even
            // and the odd outputs run as two passes over the taps, 8
            // accumulator pairs each, in 256-lane workgroups at 3 waves per
            // SIMD (one pass of 16 spilled even at that 168-VGPR budget).
            constexpr int EH = ((R - 1) * MD + 1) / 2;
            constexpr int S = EH / 4 + 3 + (EH / 4 + 3) % 2;
            constexpr int U = S;
            constexpr int TPC = 4 * U;  // tap pairs per chunk
            constexpr int RSTEP = MD == 1 ? 2 : 1, RP = R / RSTEP;  // output stride and count of a pass
            static_assert(TPC <= dot2_pair_slack, "the pair array's zero slack covers a chunk read ahead");
            auto slot = [](int e) { return ((e % S) + S) % S; };
            auto chunk_base = [&](int q0) { return t + ((HG - q0) >> 1); };
            const int NS = J / 4;  // steps
            auto pass = [&](auto r0_tag) {
                constexpr int R0 = decltype(r0_tag)::value;  // first output of the pass
                int32_t yr[RP], yi[RP];
#pragma unroll
                for (int k = 0; k < RP; ++k) yr[k] = yi[k] = 0;
                uint32_t W[S][2][4];  // [slot][plane][dword]
                auto load_e = [&](int cb, int e) {
                    const int o = cb + (e & 1) * NC + (e >> 1);
                    u4v_t gr = *(const u4v_t *)&lds[o];
                    u4v_t gi = *(const u4v_t *)&lds[o + 2 * NC];
                    asm volatile("" : "+v"(gr), "+v"(gi));  // whole ds_read_b128 (as above)
                    uint32_t(&ww)[2][4] = W[slot(e)];
                    ww[0][0] = gr[0]; ww[0][1] = gr[1]; ww[0][2] = gr[2]; ww[0][3] = gr[3];
                    ww[1][0] = gi[0]; ww[1][1] = gi[1]; ww[1][2] = gi[2]; ww[1][3] = gi[3];
                };
                // the lgkmcnt wait for a window read then never waits on a fresh s_load
                uint32_t Tc[TPC], Tn[TPC];
                auto load_taps = [&](uint32_t(&T)[TPC], int q0) {
                    ConstPtr<uint32_t> tc = tp + 4 * q0;
                    asm volatile("" : "+s"(tc));
#pragma unroll
                    for (int i = 0; i < TPC; ++i) T[i] = tc[i];
                };
                load_taps(Tc, 0);
                auto chunk = [&](int q0, auto steps_tag) {
                    constexpr int SN = decltype(steps_tag)::value;  // steps in this chunk (U, or a tail 1..U-1)
                    const int cb = chunk_base(q0);
#pragma unroll
                    for (int s = 0; s < SN; ++s) {
                        load_e(cb, -s - 2);
                        if (SN == U && s == 0) load_taps(Tn, q0 + U);
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            const uint32_t P = Tc[4 * s + p];
#pragma unroll
                            for (int k = 0; k < RP; ++k) {
                                const int r = R0 + k * RSTEP;
                                auto dw = [&](int pl, int d) {
                                    const int e = floordiv(d, 4);
                                    return W[slot(e)][pl][d - 4 * e];
                                };
                                if ((r * MD) % 2 == 0) {
                                    const int d = r * MD / 2 - 4 * s - p;
                                    yr[k] = sdot2(dw(0, d), P, yr[k]);
                                    yi[k] = sdot2(dw(1, d), P, yi[k]);
                                } else {  // odd-aligned pair (x[2a+1], x[2a+2])
                                    const int d = (r * MD - 1) / 2 - 4 * s - p;
                                    yr[k] = sdot2(__builtin_amdgcn_alignbit(dw(0, d + 1), dw(0, d), 16), P, yr[k]);
                                    yi[k] = sdot2(__builtin_amdgcn_alignbit(dw(1, d + 1), dw(1, d), 16), P, yi[k]);
                                }
                            }
                        }
                    }
                    if constexpr (SN == U) {
#pragma unroll
                        for (int i = 0; i < TPC; ++i) Tc[i] = Tn[i];
                    }
                };
                {
                    const int cb = chunk_base(0);
#pragma unroll
                    for (int e = EH / 4; e >= -1; --e) load_e(cb, e);
                }
                int q0 = 0;
                for (; q0 + U <= NS; q0 += U) chunk(q0, std::integral_constant<int, U>{});
                // the tail: 1 .. U-1 steps (wave-uniform), one unrolled body per length
                auto tail = [&](auto self, auto k_tag) {
                    constexpr int K = decltype(k_tag)::value;
                    if constexpr (K < U) {
                        if (NS - q0 == K) chunk(q0, k_tag);
                        else self(self, std::integral_constant<int, K + 1>{});
                    }
                };
                tail(tail, std::integral_constant<int, 1>{});
                quant(yr, yi, w + R0, RP, RSTEP);
            };
            pass(std::integral_constant<int, 0>{});
            if constexpr (RSTEP == 2) pass(std::integral_constant<int, 1>{});
        }
        SRCDSP_PH(ph4);
        const long n0 = tile * TO + (long)t * R;
        if (n0 + R <= a.n_out) {
            if constexpr (R >= 4) {
#pragma unroll
                for (int r = 0; r < R; r += 4) *(uint4 *)(out + n0 + r) = make_uint4(w[r], w[r + 1], w[r + 2], w[r + 3]);
            } else if constexpr (R == 2) {
                *(uint2 *)(out + n0) = make_uint2(w[0], w[1]);
            } else {
                out[n0] = w[0];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (n0 + r < a.n_out) out[n0 + r] = w[r];
        }
        SRCDSP_PH(ph5);
        SRCDSP_PH_ADD(1, ph1 - ph0);
        SRCDSP_PH_ADD(2, ph2 - ph1);
        SRCDSP_PH_ADD(3, ph3 - ph2);
        SRCDSP_PH_ADD(4, ph4 - ph3);
        SRCDSP_PH_ADD(5, ph5 - ph4);
        SRCDSP_PH_ADD(7, 1);
    }
#ifdef SRCDSP_PHASE_CLOCK
    if ((t & 63) == 0)
        for (int k = 0; k < 8; ++k) atomicAdd(&phase_clock[k], ph_acc[k]);
#endif
}

}  // namespace srcdsp
