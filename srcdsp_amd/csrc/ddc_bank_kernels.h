// ddc_bank_kernels.h -- the DDC bank kernel: C NCO mixer -> decimate-by-4
// chains (mixers.h:169-188, dnsampling_filters.h:129-172) that share one
// channel filter, and optionally one input, in a single launch.
//
// ddc_bank_ci16 is decim_dot2_ci16's run-time-tap form (decim_ci16_kernels.h) with
// the channel as an inner loop: complex<int16_t> samples, int16-range taps as
// v_dot2 tap pairs over planar int16 LDS images, M = 4, any tap count <= 1024,
// a mixer table of N = 2^k <= 4096 entries.
//  * A persistent grid of 256-lane workgroups; workgroup (x, y) owns a
//    contiguous run of time tiles (1024 outputs = 4096 input samples) and the
//    channel group y (a.group channels; one channel when every channel has its
//    own input).
//  * A tile's raw span (4096 samples + the HS-sample halo) is fetched ONCE,
//    buffer-resource 16-byte loads, and stays in registers (6 granules per
//    lane) while the group's channels are served; the next tile's loads are
//    issued after the last channel's mixing pass, ahead of its tap loop.
//  * Per channel: the lane mixes its granules into the plane image (real and
//    imaginary int16 planes, the column-major layout of dot2_slot), the
//    workgroup synchronises, and each lane runs the tap loop for its 4
//    consecutive outputs: steps of 4 tap pairs, a window of three plane
//    granules per plane sliding one granule per step, the next granule read
//    one step ahead; taps are scalar loads shared by all channels.
//  * Mixer table: ONE general form for all channels, the N-word (cos, sin)
//    table in LDS, read per sample at the phase (phi0 + s*freq) & (N - 1)
//    (N a power of two: no modulo).  The word of phase k sits at
//    k ^ (k >> 5) ^ (k >> 10) (a bijection of [0, N) for N = 2^k), so the
//    lanes' reads, 4*freq words apart, spread over the banks for every
//    frequency word (the plain table serialises up to 32-way when 4*freq is a
//    multiple of 32).
//  * Tile 0's halo is the channel's own history (already mixed samples, zeros
//    before it); the workgroup that owns tile 0 writes the channel's new
//    history (the last N-1 samples of history ++ mixed input) into the other
//    ping-pong buffer.
// LDS: 20.25 KB plane image + 16 KB table = 36.25 KB, four workgroups per CU.
#pragma once
#include "fir_device.h"

namespace srcdsp {

constexpr int kBankBlock = 256;                // lanes
constexpr int kBankTO = 4 * kBankBlock;        // outputs per tile (4 per lane)
constexpr int kBankSPT = 4 * kBankTO;          // input samples per tile (M = 4)
constexpr int kBankMaxN = 4096;                // mixer table entries
constexpr int kBankGroup = 8;                  // channels per workgroup on a shared input
// tap pairs padded to whole 4-pair steps (dot2_rt_pairs); the halo covers the
// lowest window granule (one per step) and is a whole lane chunk (16 samples)
__host__ __device__ constexpr int bank_halo(int ntaps) { return 16 * ceildiv(dot2_rt_pairs(ntaps) / 4, 2); }
constexpr int kBankMaxHS = bank_halo(kDot2MaxTaps);
constexpr int kBankPER = ceildiv((kBankSPT + kBankMaxHS) / 4, kBankBlock);  // staged granules per lane
constexpr int kBankNC0 = ceildiv((kBankSPT + kBankMaxHS) / 8, 2);
constexpr int kBankNC = kBankNC0 + ((4 - kBankNC0 % 8) + 8) % 8;  // slots per plane row, = 4 (mod 8)

struct BankLaunch {
    const void *in;
    void *out;
    const uint32_t *cpair;       // the shared tap pairs (FirCore::d_cpair)
    const int16_t *table;        // the mixers' sine table (N entries)
    long n_in, n_out;
    long in_stride, out_stride;  // samples between channels; in_stride 0: one shared input
    long ntiles;
    int ntaps;
    unsigned shift;
    unsigned N;                  // power of two <= kBankMaxN
    int channels, group;         // grid.y = ceil(channels / group)
    uint32_t mix[kMaxBatch];     // per channel: phi0 | freq << 16
    const void *hist_in[kMaxBatch];
    void *hist_out[kMaxBatch];
};

__device__ __forceinline__ unsigned bank_swz(unsigned k) { return k ^ (k >> 5) ^ (k >> 10); }

__global__ __launch_bounds__(kBankBlock, 4) void ddc_bank_ci16(BankLaunch a) {
    constexpr int BLOCK = kBankBlock, TO = kBankTO, SPT = kBankSPT, NC = kBankNC, PER = kBankPER;
    __shared__ uint4 lds[4 * NC];
    __shared__ uint32_t lut[kBankMaxN];
    typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));

    const int t = threadIdx.x;
    const int H = a.ntaps - 1;
    const int NS = dot2_rt_pairs(a.ntaps) / 4;  // steps of 4 tap pairs
    const int HS = bank_halo(a.ntaps);
    const int HG = HS / 8;                      // halo plane granules (even)
    const int TG = (SPT + HS) / 4;              // staged 16-B sample granules
    const long n_in = a.n_in;
    const unsigned N = a.N, mask = N - 1;
    const int c_begin = blockIdx.y * a.group;
    const int c_end = c_begin + a.group < a.channels ? c_begin + a.group : a.channels;
    const uint32_t *in = (const uint32_t *)a.in + (long)c_begin * a.in_stride;

    const long nb = gridDim.x;
    const long b = xcd_tile(blockIdx.x, nb);
    const long per = a.ntiles / nb, rem = a.ntiles % nb;
    const long t_begin = b * per + (b < rem ? b : rem);
    const long t_end = t_begin + per + (b < rem ? 1 : 0);
    if (t_begin >= t_end) return;

    // the (lr, li) word of phase k: (lo T[(k + N/4) % N], hi T[k])
    for (unsigned k = t; k < N; k += BLOCK)
        lut[bank_swz(k)] = ((uint32_t)(uint16_t)a.table[(k + N / 4) & mask]) | ((uint32_t)(uint16_t)a.table[k] << 16);
    __syncthreads();

    // mixers.h:169-188 on 4 consecutive samples, the first at phase ph
    auto mix4 = [&](uint4 w, unsigned ph, unsigned fr, uint2 &re, uint2 &im) {
        auto word = [&](unsigned p) { return lut[bank_swz(p & mask)]; };
        int32_t r[4], i[4];
        mix_granule_c(w, make_uint4(word(ph), word(ph + fr), word(ph + 2 * fr), word(ph + 3 * fr)), r, i);
        re = clamp_granule_s14(r);
        im = clamp_granule_s14(i);
    };
    auto lds_half = [&](int g, int plane) { return (uint2 *)&lds[dot2_slot<NC>(g >> 1, plane)] + (g & 1); };

    // the tile's raw samples: granule g = t + i BLOCK holds samples
    // tile*SPT - HS + 4g .. + 3, zeros outside [0, n_in)
    uint4 v[PER];
    auto stage_load = [&](long tile) {
        const long b0 = (long)SPT * tile - HS;     // < 0 at tile 0 only
        const long bb = b0 < 0 ? 0 : b0;
        const int skip = (int)(bb - b0);           // samples of the halo before the input
        const long remb = (n_in - bb) * 4;
        const unsigned nrec = (unsigned)(remb > 0xfffffff0L ? 0xfffffff0L : remb);
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(in + bb), 0, nrec, 0x00020000);
        int tl = t;
        asm volatile("" : "+v"(tl));
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int g = tl + i * BLOCK;
            const int off = 16 * g - 4 * skip;
            v[i] = make_uint4(0, 0, 0, 0);
            if (g < TG && off >= 0) {
                auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    stage_load(t_begin);

    for (long tile = t_begin; tile < t_end; ++tile) {
        const long b0 = (long)SPT * tile - HS;
#pragma nounroll
        for (int c = c_begin; c < c_end; ++c) {
            const uint32_t pf = a.mix[c];
            const unsigned phi0 = pf & 0xffffu, fr = pf >> 16;
            const uint32_t *hist = (const uint32_t *)a.hist_in[c];
            if (tile == 0) {  // new history = last H samples of (history ++ mixed input)
                uint32_t *ho = (uint32_t *)a.hist_out[c];
                for (int k = t; k < H; k += BLOCK) {
                    const long idx = n_in - H + k;
                    uint32_t w;
                    if (idx >= 0) {
                        const uint32_t C = lut[bank_swz((phi0 + (unsigned)idx * fr) & mask)];
                        int32_t re, im;
                        mix_dot2(in[idx], C, re, im);
                        w = pack16(re, im);
                    } else {
                        w = hist[H + idx];
                    }
                    ho[k] = w;
                }
            }
            __syncthreads();  // the previous tap loop has read the image
            const unsigned ph_t = phi0 + (unsigned)b0 * fr;  // phase of the tile's first staged sample (mod N)
            // (the lane index made opaque per channel: the per-granule addresses
            // are recomputed, not kept in registers across the tap loop)
            int tv = t;
            asm volatile("" : "+v"(tv));
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int g = tv + i * BLOCK;
                if (g < TG) {
                    uint2 re, im;
                    mix4(v[i], ph_t + 4u * (unsigned)g * fr, fr, re, im);
                    *lds_half(g, 0) = re;
                    *lds_half(g, 1) = im;
                }
            }
            if (tile == 0) {  // tile 0's halo: the channel's history, already mixed (zeros before it)
                for (int g = tv; 4 * g < HS; g += BLOCK) {
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = H - HS + 4 * g + j;
                        w[j] = k >= 0 ? hist[k] : 0u;
                    }
                    *lds_half(g, 0) = make_uint2(lo16_pair(w[0], w[1]), lo16_pair(w[2], w[3]));
                    *lds_half(g, 1) = make_uint2(hi16_pair(w[0], w[1]), hi16_pair(w[2], w[3]));
                }
            }
            __syncthreads();
            // the raw registers are free after the group's last mixing pass
            if (c + 1 == c_end && tile + 1 < t_end) stage_load(tile + 1);

            // tap loop: output r of the lane sits at sample 4r of its chunk
            // (plane granule LG); pair j = 4q + p reads plane dword 2r - j
            ConstPtr<uint32_t> tp = const_view<uint32_t>(a.cpair);
            const int LG = HG + 2 * tv;
            struct Gran { u4v_t r, i; };  // one window granule of both planes
            Gran W0, W1, W2, W3;           // rotating, static names
            auto load_e = [&](Gran &w, int e) {
                const int G = LG + e;
                const int o = (G & 1) * NC + (G >> 1);
                w.r = *(const u4v_t *)&lds[o];
                w.i = *(const u4v_t *)&lds[o + 2 * NC];
                asm volatile("" : "+v"(w.r), "+v"(w.i));  // whole ds_read_b128
            };
            int32_t yr[4] = {0, 0, 0, 0}, yi[4] = {0, 0, 0, 0};
            // step q: granules -q+1 (hi), -q (mid), -q-1 (lo); -q-2 read ahead into nx
            auto step = [&](int q, const Gran &hi, const Gran &mid, const Gran &lo, Gran &nx) {
                if (q + 1 < NS) load_e(nx, -q - 2);
                ConstPtr<uint32_t> tc = tp + 4 * q;
                asm volatile("" : "+s"(tc));
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t P = tc[p];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = 2 * r - p + 4;  // 1 .. 10 over (lo, mid, hi)
                        const uint32_t xr = d < 4 ? lo.r[d] : (d < 8 ? mid.r[d - 4] : hi.r[d - 8]);
                        const uint32_t xi = d < 4 ? lo.i[d] : (d < 8 ? mid.i[d - 4] : hi.i[d - 8]);
                        yr[r] = sdot2(xr, P, yr[r]);
                        yi[r] = sdot2(xi, P, yi[r]);
                    }
                }
            };
            load_e(W0, 1);
            load_e(W1, 0);
            load_e(W2, -1);
            int q = 0;
#pragma nounroll
            for (; q + 4 <= NS; q += 4) {
                step(q, W0, W1, W2, W3);
                step(q + 1, W1, W2, W3, W0);
                step(q + 2, W2, W3, W0, W1);
                step(q + 3, W3, W0, W1, W2);
            }
            if (q < NS) {  // the last 1..3 steps (wave-uniform)
                step(q, W0, W1, W2, W3);
                if (q + 1 < NS) {
                    step(q + 1, W1, W2, W3, W0);
                    if (q + 2 < NS) step(q + 2, W2, W3, W0, W1);
                }
            }
            // limitScale16 of the accumulator pairs (dnsampling_filters.h:167-168)
            const unsigned sh = a.shift;
            uint32_t w[4];
            if ((sh & 31u) != 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = limit16_pair_sh(yr[r], yi[r], sh);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = pack16(limit16(yr[r], sh), limit16(yi[r], sh));
            }
            uint32_t *out = (uint32_t *)a.out + (long)c * a.out_stride;
            const long n0 = tile * TO + 4L * t;
            // (a row of the [C, n_out] output starts 16-byte aligned only when
            // n_out is a multiple of 4: wave-uniform test per channel)
            if (n0 + 4 <= a.n_out && ((uintptr_t)out & 15u) == 0) {
                *(uint4 *)(out + n0) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < a.n_out) out[n0 + r] = w[r];
            }
        }
    }
}

}  // namespace srcdsp
