// sdpsk_kernels.h -- the differential SDPSK demodulator's arithmetic, one
// source for the kernel (sdpsk.hip) and for the host: srcdsp_sdpsk_step_host
// and the stand-alone host program of the tests (tests/cpp/sdpsk_host.cpp).
// Nothing here needs the HIP headers.
//
// An extension with no reference class.  SymbolMapperSdpsk advances the phase
// by +90 degrees for a one and by -90 degrees for a zero (modulators.h:93-111),
// so a bit is the sign of Im(x[i] * conj(x[i - D])), D the samples per symbol.
//
// A sample is a packed word, lo = re, hi = im.  With v = carry ++ in[0..n),
// a = in[i] and b = v[i] (in[i - D], or carry[i] for i < D):
//   tq      = im(a) * re(b) - re(a) * im(b)       int32; |tq| <= 2^31 - 32768
//   soft[i] = limitScale<int8_t, int32_t>(tq, shift)        (dsp_complex.h:45-63)
//   bit[i]  = tq > 0 ? 1 : 0
//   carry'  = v[n .. n + D)      the last D samples seen, also when n < D
// limitScale is an arithmetic shift, then a clamp to [-128, 127].  bit[i] is the
// mapper's bit convention read backwards.  The carry is zero after create and
// reset, so the first D outputs after them are soft 0 and bit 0: a caller who
// wants a burst's first payload symbol starts the window D samples early and
// drops D outputs.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SRCDSP_SDPSK_HD __host__ __device__ inline
#else
#define SRCDSP_SDPSK_HD inline
#endif

namespace srcdsp {

constexpr unsigned kSdpskMaxD = 64;      // samples a handle carries at most
constexpr unsigned kSdpskMaxShift = 31;
constexpr int kSdpskBlock = 256;         // lanes of a workgroup
// Words a lane loads per tile, 16 bytes at a time: 4, 8 or 16.  Measured on one
// row of 2^26 and of 2^28 samples, soft bits alone and both outputs: 4 takes
// 1.08-1.22 of 8's time and 16 takes 1.01-1.11 (profiles/sdpsk_time.json)
#ifndef SRCDSP_SDPSK_LANE_WORDS
#define SRCDSP_SDPSK_LANE_WORDS 8
#endif
constexpr int kSdpskLaneWords = SRCDSP_SDPSK_LANE_WORDS;
static_assert(kSdpskLaneWords == 4 || kSdpskLaneWords == 8 || kSdpskLaneWords == 16, "words per lane: 4, 8 or 16");
constexpr int kSdpskTileWords = kSdpskBlock * kSdpskLaneWords;
constexpr long kSdpskMaxRows = 65535;    // rows of one launch (grid.y)

SRCDSP_SDPSK_HD int32_t sdpsk_re(uint32_t w) { return (int32_t)(int16_t)(uint16_t)(w & 0xffffu); }
SRCDSP_SDPSK_HD int32_t sdpsk_im(uint32_t w) { return (int32_t)(int16_t)(uint16_t)(w >> 16); }
// Im(a * conj(b)).  A product reaches +2^30 only as -32768 * -32768 and is never
// below -32768 * 32767, so the difference stays inside +-(2^31 - 32768)
SRCDSP_SDPSK_HD int32_t sdpsk_tq(uint32_t a, uint32_t b) {
    return sdpsk_im(a) * sdpsk_re(b) - sdpsk_re(a) * sdpsk_im(b);
}
// limitScale<int8_t, int32_t> (dsp_complex.h:45-63)
SRCDSP_SDPSK_HD int32_t sdpsk_soft(int32_t tq, unsigned shift) {
    const int32_t s = tq >> shift;
    return s > 127 ? 127 : (s < -128 ? -128 : s);
}
SRCDSP_SDPSK_HD uint32_t sdpsk_bit(int32_t tq) { return tq > 0 ? 1u : 0u; }
// v[i], 0 <= i < n + D: element i of carry ++ in
SRCDSP_SDPSK_HD uint32_t sdpsk_v(const uint32_t *carry, const uint32_t *in, long i, long D) {
    return i < D ? carry[i] : in[i - D];
}

// ---------------------------------------------------------------- host form
// one step on host buffers; soft or bits may be null; carry is updated
inline void sdpsk_host_run(uint32_t *carry, unsigned D, unsigned shift, const uint32_t *in, size_t n, int8_t *soft,
                           uint8_t *bits) {
    uint32_t next[kSdpskMaxD];
    for (unsigned k = 0; k < D; ++k) next[k] = sdpsk_v(carry, in, (long)(n + k), (long)D);
    for (size_t i = 0; i < n; ++i) {
        const int32_t tq = sdpsk_tq(in[i], sdpsk_v(carry, in, (long)i, (long)D));
        if (soft) soft[i] = (int8_t)sdpsk_soft(tq, shift);
        if (bits) bits[i] = (uint8_t)sdpsk_bit(tq);
    }
    for (unsigned k = 0; k < D; ++k) carry[k] = next[k];
}

}  // namespace srcdsp
