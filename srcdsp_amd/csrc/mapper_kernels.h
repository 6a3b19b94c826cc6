// mapper_kernels.h -- the symbol mappers' arithmetic (SymbolMapperSdpsk<int16_t>,
// modulators.h:82-131; SymbolMapperQpsk<int16_t>, modulators.h:147-198), one
// source for the kernels (mapper.hip, modulate.hip) and for the host: the
// step of a handle that has never touched the device, and the stand-alone
// host program of the tests (tests/cpp/mapper_host.cpp).  Nothing here needs
// the HIP headers.
//
// A bit is a byte and a one whenever it is non-zero (`bits[i] > 0` on a
// uint8_t).  A symbol is a packed word, lo = re, hi = im, of +-8192
// (ModAmplitude<int16_t>, modulators.h:34-39).
//
// SDPSK is the recurrence state += bit ? 1 : 3 (mod 4) over the whole stream.
// Its closed form state_i = (state_0 - (i + 1) + 2 ones_i) mod 4, ones_i the
// ones among bits[0..i], needs only the parity of ones_i: the scan is an XOR
// scan of one bit per input byte and a tile's carry-in is one bit.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SRCDSP_MAPPER_HD __host__ __device__ inline
#else
#define SRCDSP_MAPPER_HD inline
#endif

namespace srcdsp {

enum { MAPPER_SDPSK = 0, MAPPER_QPSK = 1 };

constexpr int kMapperLaneBits = 16;                               // one 16-byte load
constexpr int kMapperBlock = 256;                                 // lanes of a workgroup
constexpr int kMapperTileBits = kMapperLaneBits * kMapperBlock;  // bits one workgroup tile covers
constexpr uint32_t kMapperPos = 0x2000u, kMapperNeg = 0xE000u;   // +-8192 as int16

// bit k of the result: byte k of w is non-zero
SRCDSP_MAPPER_HD uint32_t mapper_nz4(uint32_t w) {
    const uint32_t t = ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u) >> 7;  // bits 0, 8, 16, 24
    return ((t * 0x00204081u) >> 21) & 0xfu;
}
// the 16-bit mask of a lane's 16 bytes, given as 4 little-endian words
SRCDSP_MAPPER_HD uint32_t mapper_nz16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return mapper_nz4(w0) | (mapper_nz4(w1) << 4) | (mapper_nz4(w2) << 8) | (mapper_nz4(w3) << 12);
}
// the same from memory: bytes b[0..avail) of the lane's 16, the rest zeros
SRCDSP_MAPPER_HD uint32_t mapper_nz16_bytes(const uint8_t *b, long avail) {
    uint32_t m = 0;
    for (int k = 0; k < kMapperLaneBits; ++k)
        if (k < avail && b[k] != 0) m |= 1u << k;
    return m;
}

// the scan's combine step: parities add modulo 2
SRCDSP_MAPPER_HD uint32_t mapper_combine(uint32_t a, uint32_t b) { return a ^ b; }

// in-lane inclusive XOR scan of a 16-bit mask: bit k = parity of bits 0..k
SRCDSP_MAPPER_HD uint32_t mapper_prefix16(uint32_t m) {
    m ^= m << 1;
    m ^= m << 2;
    m ^= m << 4;
    m ^= m << 8;
    return m & 0xffffu;
}
SRCDSP_MAPPER_HD uint32_t mapper_parity16(uint32_t m) { return (mapper_prefix16(m) >> 15) & 1u; }

// SDPSK state after bit i of a call that started in state0; par: the parity
// of the ones among bits[0..i]
SRCDSP_MAPPER_HD uint32_t mapper_sdpsk_state(uint32_t state0, unsigned long i, uint32_t par) {
    return (uint32_t)((unsigned long)state0 - (i + 1ul) + 2ul * par) & 3u;
}
// map[] of modulators.h:93-96: (A,A), (-A,A), (-A,-A), (A,-A)
SRCDSP_MAPPER_HD uint32_t mapper_sdpsk_word(uint32_t state) {
    const uint32_t re = ((state ^ (state >> 1)) & 1u) ? kMapperNeg : kMapperPos;
    const uint32_t im = (state & 2u) ? kMapperNeg : kMapperPos;
    return re | (im << 16);
}
// QPSK (modulators.h:177): state = first bit of the pair << 1 | second bit;
// map[] of :158-161: (-A,-A), (-A,A), (A,-A), (A,A)
SRCDSP_MAPPER_HD uint32_t mapper_qpsk_state(uint32_t first, uint32_t second) {
    return ((first ? 1u : 0u) << 1) | (second ? 1u : 0u);
}
SRCDSP_MAPPER_HD uint32_t mapper_qpsk_word(uint32_t state) {
    const uint32_t re = (state & 2u) ? kMapperPos : kMapperNeg;
    const uint32_t im = (state & 1u) ? kMapperPos : kMapperNeg;
    return re | (im << 16);
}

// symbols of a call of n_bits
SRCDSP_MAPPER_HD size_t mapper_n_out(int kind, size_t n_bits) { return kind == MAPPER_QPSK ? n_bits / 2 : n_bits; }

// ---------------------------------------------------------------- host form
// The kernels' structure on the host: the stream in tiles of `tile_bits`, a
// first pass for the tiles' parities, their exclusive scan, then every tile
// from its carry-in alone, in groups of 16 bits as a lane takes them.
// Returns the end state.  (QPSK: tile_bits is even.)
inline uint32_t mapper_host_run(int kind, uint32_t state0, const uint8_t *bits, size_t n_bits, uint32_t *out,
                                size_t tile_bits = kMapperTileBits) {
    if (n_bits == 0) return state0;
    if (kind == MAPPER_QPSK) {
        for (size_t i0 = 0; i0 < n_bits; i0 += kMapperLaneBits) {
            const long avail = (long)(n_bits - i0);
            const uint32_t m = mapper_nz16_bytes(bits + i0, avail);
            for (int k = 0; k < kMapperLaneBits / 2 && 2 * k + 1 < avail; ++k)
                out[i0 / 2 + k] = mapper_qpsk_word(mapper_qpsk_state((m >> (2 * k)) & 1u, (m >> (2 * k + 1)) & 1u));
        }
        return mapper_qpsk_state(bits[n_bits - 2], bits[n_bits - 1]);
    }
    uint32_t carry = 0;  // parity of the ones before the tile: the exclusive scan, as it is formed
    for (size_t t0 = 0; t0 < n_bits; t0 += tile_bits) {
        const size_t tn = n_bits - t0 < tile_bits ? n_bits - t0 : tile_bits;
        uint32_t lane_carry = carry, tile_par = 0;
        for (size_t g0 = 0; g0 < tn; g0 += kMapperLaneBits) {
            const long avail = (long)(tn - g0);
            const uint32_t m = mapper_nz16_bytes(bits + t0 + g0, avail);
            const uint32_t p = mapper_prefix16(m);
            for (int k = 0; k < kMapperLaneBits && k < avail; ++k) {
                const size_t i = t0 + g0 + k;
                out[i] = mapper_sdpsk_word(mapper_sdpsk_state(state0, i, mapper_combine(lane_carry, (p >> k) & 1u)));
            }
            lane_carry = mapper_combine(lane_carry, mapper_parity16(m));
            tile_par = mapper_combine(tile_par, mapper_parity16(m));
        }
        carry = mapper_combine(carry, tile_par);
    }
    return mapper_sdpsk_state(state0, n_bits - 1, carry);
}

}  // namespace srcdsp
