// modulate_kernels.h -- what the two transmit chains from bits share
// (modulate.hip: mapper -> interpolator -> mixer; modulate_offset.hip: the same
// with the Q-rail stagger ahead of the mixer): the tile's input staging from
// bits, the launch description and the size rules of a chain.
#pragma once
#include <string>

#include "mapper_state.h"
#include "upmix_kernels.h"

namespace srcdsp {

// the tile's input words from bits
struct UpBitsIn {
    int kind;
    const uint8_t *bits;  // QPSK: the row's bits, 16-byte aligned
    const uint32_t *pk;   // SDPSK: the row's states, 16 per word
    __device__ __forceinline__ uint32_t at(long j) const {
        if (kind == MAPPER_QPSK) return mapper_qpsk_word(mapper_qpsk_state(bits[2 * j], bits[2 * j + 1]));
        return mapper_sdpsk_word((pk[j >> 4] >> (2 * (j & 15))) & 3u);
    }
    __device__ __forceinline__ void load5(long s0, uint32_t (&w)[5]) const {
        if (kind == MAPPER_QPSK) {
            const uint2 v = *(const uint2 *)(bits + 2 * s0);  // s0 is a multiple of 4
            const uint32_t e = *(const uint16_t *)(bits + 2 * s0 + 8);
            const uint32_t m = mapper_nz4(v.x) | (mapper_nz4(v.y) << 4) | (mapper_nz4(e) << 8);
#pragma unroll
            for (int k = 0; k < 5; ++k)
                w[k] = mapper_qpsk_word(mapper_qpsk_state((m >> (2 * k)) & 1u, (m >> (2 * k + 1)) & 1u));
        } else {
            const uint32_t x = pk[s0 >> 4] >> (2 * (s0 & 15));  // 4 states: s0 & 15 is 0, 4, 8 or 12
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = mapper_sdpsk_word((x >> (2 * k)) & 3u);
            w[4] = at(s0 + 4);
        }
    }
};

struct ModLaunch {
    UpmixLaunch up;        // in / in_stride unused: the input is bits
    int kind;
    const uint8_t *bits;
    long bits_stride;      // bytes between rows (0: shared)
    long n_bits;
    const uint32_t *pk;
    long pk_stride;        // words between rows
    uint32_t *st_out[kMaxBatch];  // QPSK: the mapper's end state (null: no bits, no change)
};

// words of a row of packed SDPSK states, rounded to whole 16-byte granules
inline size_t pk_row_words(size_t n_bits) {
    return ((n_bits + kMapperLaneBits - 1) / kMapperLaneBits + 3) & ~(size_t)3;
}

// every size and type rule of one chain, before anything changes
inline int modulate_check(const MapperState &mp, const srcdsp_up_state &u, size_t n_bits, size_t *n_sym,
                          size_t *n_out, bool flush, const char *who) {
    if (u.variant == UV_I16_I32) {
        set_error(std::string(who) + ": a real int16_t interpolator cannot take complex<int16_t> symbols");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    if (mp.kind == MAPPER_QPSK && n_bits % 2 != 0) {
        set_error(std::string(who) + ": a QPSK step takes an even number of bits (modulators.h:171)");
        return SRCDSP_ERR_SIZE;
    }
    *n_sym = mapper_n_out(mp.kind, n_bits);
    *n_out = (size_t)u.L * (*n_sym + (flush ? u.length / u.L : 0));
    return SRCDSP_OK;
}

}  // namespace srcdsp
