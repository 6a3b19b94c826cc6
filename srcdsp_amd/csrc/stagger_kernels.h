// stagger_kernels.h -- the OQPSK Q-rail stagger's arithmetic, one source for
// the kernels (stagger.hip, modulate_offset.hip) and for the host: the step of
// a handle that has never touched the device, and the stand-alone host program
// of the tests (tests/cpp/stagger_host.cpp).  Nothing here needs the HIP
// headers.
//
// An extension with no reference class: in reference terms a delay line of D
// output samples on the imaginary rail, between FilterUpsamplingFir::step
// (upsampling_filters.h:149-233) and Mixer::step (mixers.h:169-188).
//
// A sample is a packed word, lo = re, hi = im.  With v = carry ++ im(in[0..n))
// the virtual Q stream, out[i] = (re(in[i]), v[i]) and the new carry is
// v[n .. n + D): the last D imaginary halves seen, also when n < D.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SRCDSP_STAGGER_HD __host__ __device__ inline
#else
#define SRCDSP_STAGGER_HD inline
#endif

namespace srcdsp {

constexpr unsigned kStaggerMaxD = 64;  // values a handle carries at most
constexpr int kStaggerBlock = 256;     // lanes of a workgroup
constexpr int kStaggerLaneWords = 4;   // one 16-byte load and store per lane
constexpr int kStaggerTileWords = kStaggerBlock * kStaggerLaneWords;

// v[i], 0 <= i < n + D: element i of carry ++ im(in)
SRCDSP_STAGGER_HD uint32_t stagger_q(const int16_t *carry, const uint32_t *in, long i, long D) {
    return i < D ? (uint32_t)(uint16_t)carry[i] : in[i - D] >> 16;
}
// a sample's real half over a Q value (its low 16 bits)
SRCDSP_STAGGER_HD uint32_t stagger_word(uint32_t w, uint32_t q) { return (w & 0xffffu) | (q << 16); }
// out[i] of a step
SRCDSP_STAGGER_HD uint32_t stagger_out(const int16_t *carry, const uint32_t *in, long i, long D) {
    return stagger_word(in[i], stagger_q(carry, in, i, D));
}
// carry'[k], 0 <= k < D, after a step of n samples
SRCDSP_STAGGER_HD int16_t stagger_carry(const int16_t *carry, const uint32_t *in, long n, long k, long D) {
    return (int16_t)(uint16_t)stagger_q(carry, in, n + k, D);
}

// ---------------------------------------------------------------- host form
// one step on host buffers (in and out do not overlap); carry is updated
inline void stagger_host_run(int16_t *carry, unsigned D, const uint32_t *in, size_t n, uint32_t *out) {
    int16_t next[kStaggerMaxD];
    for (unsigned k = 0; k < D; ++k) next[k] = stagger_carry(carry, in, (long)n, (long)k, (long)D);
    for (size_t i = 0; i < n; ++i) out[i] = stagger_out(carry, in, (long)i, (long)D);
    for (unsigned k = 0; k < D; ++k) carry[k] = next[k];
}

}  // namespace srcdsp
