// modulate_kernels.h -- what the two transmit chains from bits share
// (modulate.hip: mapper -> interpolator -> mixer; modulate_offset.hip: the same
// with the Q-rail stagger ahead of the mixer): the tile's input staging from
// bits with its kernel prologue, the launch description, the mapper layer of a
// launch's begin and commit and the size rules of a chain.
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

// The bits source's kernel prologue: the tile's input of chain c; the call's
// first lane also writes the QPSK mapper's end state
__device__ __forceinline__ UpBitsIn mod_bits_row(const ModLaunch &Q, int c) {
    const int kind = Q.kind;
    const uint8_t *row = Q.bits + c * Q.bits_stride;
    if (kind == MAPPER_QPSK && blockIdx.x == 0 && threadIdx.x == 0 && Q.st_out[c])
        *Q.st_out[c] = mapper_qpsk_state(row[Q.n_bits - 2], row[Q.n_bits - 1]);  // modulators.h:177, the last pair
    return UpBitsIn{kind, row, Q.pk + c * Q.pk_stride};
}

// words of a row of packed SDPSK states, rounded to whole 16-byte granules
inline size_t pk_row_words(size_t n_bits) {
    return ((n_bits + kMapperLaneBits - 1) / kMapperLaneBits + 3) & ~(size_t)3;
}

// The mapper layer of a launch's two halves, on upmix_launch_begin /
// upmix_launch_commit (upmix_kernels.h; `more` as there).  Ahead of the kernel:
// the SDPSK mapper's launches, the launch description and every handle's begin
template <class More>
int mod_launch_begin(ModLaunch &Q, const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers,
                     int nc, const void *d_bits, size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits,
                     size_t n_sym, long n_total, bool iter, hipStream_t s, size_t *smem, More more) {
    MapperState &lead = maps[0]->m;
    Q.kind = lead.kind;
    Q.bits = (const uint8_t *)d_bits;
    Q.bits_stride = (long)bits_stride;
    Q.n_bits = (long)n_bits;
    if (Q.kind == MAPPER_SDPSK && n_bits) {
        const size_t rw = pk_row_words(n_bits);
        int rc = lead.sym.reserve(4 * rw * (size_t)nc);
        if (!rc) rc = mapper_launch(lead, maps, nc, d_bits, bits_stride, lead.sym.d, rw, n_bits, kMapperStates, s);
        if (rc) return rc;
        Q.pk = lead.sym.dev<uint32_t>();
        Q.pk_stride = (long)rw;
    }
    const bool qpsk_state = Q.kind == MAPPER_QPSK && n_bits;
    return upmix_launch_begin(Q.up, ups, mixers, nc, d_out, out_stride, n_sym, n_total, iter, s, smem, [&](int c) {
        int rc = more(c);
        if (!rc && qpsk_state) {
            MapperRowState row;
            rc = mapper_begin(maps[c]->m, s, row);
            Q.st_out[c] = row.out;
        }
        return rc;
    });
}

// Behind the kernel: the layer below, then every mapper's commit
template <class More>
int mod_launch_commit(const srcdsp_mapper_t *maps, const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int nc,
                      size_t n_bits, long n_total, hipStream_t s, More more) {
    const bool qpsk_state = maps[0]->m.kind == MAPPER_QPSK && n_bits;
    return upmix_launch_commit(ups, mixers, nc, n_total, s, [&](int c) {
        int rc = more(c);
        // SDPSK: the tile read the mapper's packed states, so the mapper's
        // next step (which may rewrite them) is ordered after the tile too
        if (!rc && n_bits) rc = qpsk_state ? mapper_commit(maps[c]->m, s) : maps[c]->m.order.after(s);
        return rc;
    });
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
