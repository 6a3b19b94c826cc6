// mapper.hip -- dsptl::SymbolMapperSdpsk<int16_t> (modulators.h:82-131) and
// dsptl::SymbolMapperQpsk<int16_t> (modulators.h:147-198) on gfx950:
// srcdsp_mapper_step and the bank srcdsp_mapper_step_batched (grid.y = row).
//
// A lane reads 16 bits as one 16-byte load and turns them into a 16-bit mask
// of ones (mapper_kernels.h).  QPSK is a pure function of a pair.  SDPSK is a
// recurrence over the whole stream whose closed form needs the parity of the
// ones before each bit: an XOR scan, in the lane with shifts, in the wave with
// a ballot and a popcount, in the workgroup through four LDS words.  Across
// workgroups the carry comes from two launches of their own, earlier on the
// same stream: mapper_tile_parity (one word per tile) and mapper_tile_scan
// (their exclusive scan, one workgroup per row, and the row's end state).  No
// workgroup ever waits on another; the bits are read twice.  A call of one
// tile needs neither and is one launch.
//
// The symbols of a wave are contiguous, so a lane's masks are passed through
// the wave (__shfl) to the lane whose 16-byte store they belong to: every
// store instruction of a wave writes one contiguous 1 KiB, non-temporal (the
// output is written once, 4 bytes per bit).
#include <algorithm>

#include "mapper_state.h"

namespace srcdsp {
namespace {

struct MapperLaunch {
    const uint8_t *bits;
    uint32_t *out;
    long n_bits;
    long bits_stride;  // bytes between rows (0: one row for all)
    long out_stride;   // words between rows
    uint32_t *par;     // [rows][tiles]: tile parities, then carry-ins
    long tiles;
    int vec_in, vec_out;  // rows 16-byte aligned: dwordx4 loads / stores
    MapperRowState st[kMaxBatch];
};

__device__ __forceinline__ uint32_t mapper_state0(const MapperLaunch &P, int c) {
    const int h = P.st[c].host;
    return h >= 0 ? (uint32_t)h : (*P.st[c].in & 3u);
}

// the mask of ones of this lane's 16 bits from bit i0 of a row of n
__device__ __forceinline__ uint32_t mapper_lane_mask(const uint8_t *row, long i0, long n, bool vec) {
    if (i0 >= n) return 0;
    if (vec && i0 + kMapperLaneBits <= n) {
        const uint4 v = *(const uint4 *)(row + i0);
        return mapper_nz16(v.x, v.y, v.z, v.w);
    }
    return mapper_nz16_bytes(row + i0, n - i0);
}

// exclusive XOR scan of one bit per lane over the workgroup, in lane order;
// *total: the workgroup's parity.  wp: kMapperBlock / 64 LDS words.
__device__ __forceinline__ uint32_t mapper_block_scan(uint32_t bit, uint32_t *wp, uint32_t *total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(bit != 0);
    uint32_t ex = (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) & 1u;
    if (lane == 0) wp[wave] = (uint32_t)__popcll(b) & 1u;
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (unsigned w = 0; w < kMapperBlock / 64; ++w) {
        const uint32_t v = wp[w];
        if (w < wave) ex = mapper_combine(ex, v);
        tot = mapper_combine(tot, v);
    }
    *total = tot;
    return ex;
}

// 4 consecutive words from word w0 of a row of n_out
__device__ __forceinline__ void mapper_store4(uint32_t *row, long w0, long n_out, const uint32_t (&w)[4], bool vec) {
    typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
    if (vec && w0 + 4 <= n_out) {
        u4v_t v;
        v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; v[3] = w[3];
        __builtin_nontemporal_store(v, (u4v_t *)(row + w0));
        return;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (w0 + u < n_out) row[w0 + u] = w[u];
}

__global__ __launch_bounds__(kMapperBlock) void mapper_tile_parity(const MapperLaunch P) {
    __shared__ uint32_t wp[kMapperBlock / 64];
    const int c = blockIdx.y;
    const long i0 = (long)blockIdx.x * kMapperTileBits + (long)kMapperLaneBits * threadIdx.x;
    const uint32_t m = mapper_lane_mask(P.bits + c * P.bits_stride, i0, P.n_bits, P.vec_in != 0);
    uint32_t tot;
    mapper_block_scan(mapper_parity16(m), wp, &tot);
    if (threadIdx.x == 0) P.par[c * P.tiles + blockIdx.x] = tot;
}

// one workgroup per row: the tiles' parities become their exclusive scan in
// place, and the row's end state goes to its device word
__global__ __launch_bounds__(kMapperBlock) void mapper_tile_scan(const MapperLaunch P) {
    __shared__ uint32_t wp[kMapperBlock / 64];
    const int c = blockIdx.x;
    uint32_t *par = P.par + c * P.tiles;
    const long per = (P.tiles + kMapperBlock - 1) / kMapperBlock;
    const long lo = min((long)threadIdx.x * per, P.tiles), hi = min(lo + per, P.tiles);
    uint32_t x = 0;
    for (long k = lo; k < hi; ++k) x = mapper_combine(x, par[k]);
    uint32_t tot;
    uint32_t ex = mapper_block_scan(x, wp, &tot);
    for (long k = lo; k < hi; ++k) {
        const uint32_t v = par[k];
        par[k] = ex;
        ex = mapper_combine(ex, v);
    }
    if (threadIdx.x == 0) *P.st[c].out = mapper_sdpsk_state(mapper_state0(P, c), (unsigned long)P.n_bits - 1ul, tot);
}

template <int KIND, int MODE>
__global__ __launch_bounds__(kMapperBlock) void mapper_stream(const MapperLaunch P) {
    const int c = blockIdx.y;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const long tile0 = (long)blockIdx.x * kMapperTileBits;
    const long i0 = tile0 + (long)kMapperLaneBits * t;
    const uint32_t m = mapper_lane_mask(P.bits + c * P.bits_stride, i0, P.n_bits, P.vec_in != 0);
    uint32_t *orow = P.out + c * P.out_stride;
    if constexpr (KIND == MAPPER_QPSK) {
        const long n_out = P.n_bits / 2;
        const long wbase = (tile0 + 64L * kMapperLaneBits * wave) / 2;  // the wave's first symbol
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // store j of lane l: symbols 4 (64 j + l) .. + 3 of the wave, the bits of lane 32 j + l / 2
            const uint32_t mm = (uint32_t)__shfl((int)m, (int)(32 * j + (lane >> 1)), 64);
            const uint32_t h = (mm >> (8 * (lane & 1u))) & 0xffu;
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                w[u] = mapper_qpsk_word(mapper_qpsk_state((h >> (2 * u)) & 1u, (h >> (2 * u + 1)) & 1u));
            mapper_store4(orow, wbase + 4L * (64 * j + lane), n_out, w, P.vec_out != 0);
        }
        // the last pair's state (modulators.h:177): both bits are in one lane
        const long last = P.n_bits - 2;
        if (last >= i0 && last < i0 + kMapperLaneBits) {
            const int k = (int)(last - i0);
            *P.st[c].out = mapper_qpsk_state((m >> k) & 1u, (m >> (k + 1)) & 1u);
        }
    } else {
        __shared__ uint32_t wp[kMapperBlock / 64];
        const uint32_t p = mapper_prefix16(m);
        uint32_t tot;
        uint32_t ex = mapper_block_scan(p >> 15, wp, &tot);
        if (P.tiles > 1) ex = mapper_combine(ex, P.par[c * P.tiles + blockIdx.x] & 1u);
        const uint32_t X = p ^ (ex ? 0xffffu : 0u);  // bit k: parity of the ones up to the lane's bit k
        const uint32_t s0 = mapper_state0(P, c);
        if constexpr (MODE == kMapperSymbols) {
            const long wbase = tile0 + 64L * kMapperLaneBits * wave;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // store j of lane l: symbols 4 (64 j + l) .. + 3 of the wave, the bits of lane 16 j + l / 4
                const uint32_t xx = (uint32_t)__shfl((int)X, (int)(16 * j + (lane >> 2)), 64);
                const uint32_t nib = (xx >> (4 * (lane & 3u))) & 0xfu;
                const long w0 = wbase + 4L * (64 * j + lane);
                uint32_t w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    w[u] = mapper_sdpsk_word(mapper_sdpsk_state(s0, (unsigned long)(w0 + u), (nib >> u) & 1u));
                mapper_store4(orow, w0, P.n_bits, w, P.vec_out != 0);
            }
        } else {
            uint32_t pk = 0;
#pragma unroll
            for (int k = 0; k < kMapperLaneBits; ++k)
                pk |= mapper_sdpsk_state(s0, (unsigned long)(i0 + k), (X >> k) & 1u) << (2 * k);
            if (i0 < P.n_bits) orow[i0 / kMapperLaneBits] = pk;
        }
        // a call of one tile has no scan launch: its end state from here
        if (P.tiles == 1 && t == 0) *P.st[c].out = mapper_sdpsk_state(s0, (unsigned long)P.n_bits - 1ul, tot);
    }
}

}  // namespace

int MapperState::touch() {
    if (d_state) return SRCDSP_OK;
    int rc = order.init();
    if (rc) return rc;
    SRCDSP_HIP_TRY(hipMalloc(&d_state, 2 * sizeof(uint32_t)));
    return SRCDSP_OK;
}

int MapperState::fetch() {
    if (!on_dev) return SRCDSP_OK;
    int rc = order.sync();
    if (rc) return rc;
    uint32_t v = 0;
    SRCDSP_HIP_TRY(hipMemcpy(&v, d_state + cur, sizeof v, hipMemcpyDeviceToHost));
    state = (int)(v & 3u);
    on_dev = false;
    return SRCDSP_OK;
}

int mapper_begin(MapperState &m, hipStream_t s, MapperRowState &row) {
    int rc = m.touch();
    if (!rc) rc = m.order.before(s);
    if (rc) return rc;
    row.in = m.d_state + m.cur;
    row.out = m.d_state + (m.cur ^ 1);
    row.host = m.on_dev ? -1 : m.state;
    return SRCDSP_OK;
}

int mapper_commit(MapperState &m, hipStream_t s) {
    m.cur ^= 1;
    m.on_dev = true;
    return m.order.after(s);
}

int mapper_launch(MapperState &lead, const srcdsp_mapper_t *hs, int nc, const void *d_bits, size_t bits_stride,
                  void *d_out, size_t out_stride, size_t n_bits, MapperOut mode, hipStream_t s) {
    const int kind = hs[0]->m.kind;
    MapperLaunch P{};
    P.bits = (const uint8_t *)d_bits;
    P.out = (uint32_t *)d_out;
    P.n_bits = (long)n_bits;
    P.bits_stride = (long)bits_stride;
    P.out_stride = (long)out_stride;
    P.tiles = (long)((n_bits + kMapperTileBits - 1) / kMapperTileBits);
    P.vec_in = aligned16(d_bits) && (nc == 1 || bits_stride % 16 == 0);
    P.vec_out = aligned16(d_out) && (nc == 1 || (out_stride * 4) % 16 == 0);
    const bool scan = kind == MAPPER_SDPSK && P.tiles > 1;
    if (scan) {
        int rc = lead.par.reserve(sizeof(uint32_t) * (size_t)nc * (size_t)P.tiles);
        if (rc) return rc;
        P.par = lead.par.dev<uint32_t>();
    }
    for (int c = 0; c < nc; ++c) {
        int rc = mapper_begin(hs[c]->m, s, P.st[c]);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)P.tiles, (unsigned)nc), block(kMapperBlock);
    if (scan) {
        hipLaunchKernelGGL(mapper_tile_parity, grid, block, 0, s, P);
        hipLaunchKernelGGL(mapper_tile_scan, dim3((unsigned)nc), block, 0, s, P);
    }
    if (kind == MAPPER_QPSK)
        hipLaunchKernelGGL((mapper_stream<MAPPER_QPSK, kMapperSymbols>), grid, block, 0, s, P);
    else if (mode == kMapperSymbols)
        hipLaunchKernelGGL((mapper_stream<MAPPER_SDPSK, kMapperSymbols>), grid, block, 0, s, P);
    else
        hipLaunchKernelGGL((mapper_stream<MAPPER_SDPSK, kMapperStates>), grid, block, 0, s, P);
    SRCDSP_HIP_TRY(hipGetLastError());
    for (int c = 0; c < nc; ++c) {
        int rc = mapper_commit(hs[c]->m, s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

}  // namespace srcdsp

using namespace srcdsp;

namespace {

// the size rule of a step (modulators.h:106 and :171 assert)
int mapper_check_size(int kind, size_t n_bits, size_t n_out, const char *who) {
    if (kind == MAPPER_QPSK ? n_bits != 2 * n_out : n_bits != n_out) {
        set_error(std::string(who) + ": n_out must equal n_bits (SDPSK, modulators.h:106) or n_bits / 2 with "
                                     "n_bits even (QPSK, modulators.h:171)");
        return SRCDSP_ERR_SIZE;
    }
    return SRCDSP_OK;
}

}  // namespace

extern "C" {

// the constructors (modulators.h:87-99, :152-165): the map is the kernels'
// arithmetic, the state 0.  No device call.
SRCDSP_API int srcdsp_mapper_create(srcdsp_mapper_t *out, int kind) {
    SRCDSP_ARG_CHECK(out != nullptr, "mapper_create: null out");
    *out = nullptr;
    SRCDSP_ARG_CHECK(kind == SRCDSP_MAPPER_SDPSK || kind == SRCDSP_MAPPER_QPSK,
                     "mapper_create: kind is SRCDSP_MAPPER_SDPSK or SRCDSP_MAPPER_QPSK");
    auto *h = new srcdsp_mapper();
    h->m.kind = kind;
    *out = h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_mapper_destroy(srcdsp_mapper_t h) {
    if (!h) return SRCDSP_OK;
    MapperState &m = h->m;
    if (m.d_state) {
        (void)m.order.sync();
        (void)hipFree(m.d_state);
        m.order.destroy();
    }
    m.par.destroy();
    m.sym.destroy();
    m.rows.destroy();
    if (m.stage.stream) m.stage.destroy();
    delete h;
    return SRCDSP_OK;
}

// a value copy (the reference classes are value types): kind and state
SRCDSP_API int srcdsp_mapper_clone(srcdsp_mapper_t h, srcdsp_mapper_t *out) {
    SRCDSP_ARG_CHECK(h != nullptr && out != nullptr, "mapper_clone: null argument");
    *out = nullptr;
    int rc = h->m.fetch();
    if (rc) return rc;
    auto *n = new srcdsp_mapper();
    n->m.kind = h->m.kind;
    n->m.state = h->m.state;
    *out = n;
    return SRCDSP_OK;
}

// reset() (modulators.h:120-123, :187-190)
SRCDSP_API int srcdsp_mapper_reset(srcdsp_mapper_t h) {
    SRCDSP_ARG_CHECK(h != nullptr, "mapper_reset: null handle");
    h->m.state = 0;
    h->m.on_dev = false;  // a step still in flight is ordered before the next one by the handle's event
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_mapper_get_state(srcdsp_mapper_t h, int *kind, int *state) {
    SRCDSP_ARG_CHECK(h != nullptr, "mapper_get_state: null handle");
    int rc = h->m.fetch();
    if (rc) return rc;
    if (kind) *kind = h->m.kind;
    if (state) *state = h->m.state;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_mapper_set_state(srcdsp_mapper_t h, int state) {
    SRCDSP_ARG_CHECK(h != nullptr, "mapper_set_state: null handle");
    SRCDSP_ARG_CHECK(state >= 0 && state <= 3, "mapper_set_state: state must be in 0..3");
    h->m.state = state;
    h->m.on_dev = false;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_mapper_geometry(int *tile_bits) {
    if (tile_bits) *tile_bits = kMapperTileBits;
    return SRCDSP_OK;
}

// C mappers in one call: row c is srcdsp_mapper_step(hs[c], ...)
SRCDSP_API int srcdsp_mapper_step_batched(const srcdsp_mapper_t *hs, int channels, const void *d_bits,
                                          size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits,
                                          void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && channels >= 1, "mapper_step_batched: no handles");
    int rc = check_handles(hs, channels, "mapper_step_batched");
    if (rc) return rc;
    const int kind = hs[0]->m.kind;
    for (int c = 1; c < channels; ++c)
        SRCDSP_ARG_CHECK(hs[c]->m.kind == kind, "mapper_step_batched: mappers must share a kind");
    if (kind == MAPPER_QPSK && n_bits % 2 != 0) {
        set_error("mapper_step_batched: a QPSK step takes an even number of bits (modulators.h:171)");
        return SRCDSP_ERR_SIZE;
    }
    SRCDSP_ARG_CHECK(bits_stride == 0 || bits_stride >= n_bits,
                     "mapper_step_batched: bits_stride must be 0 (shared) or >= n_bits");
    if (out_stride < mapper_n_out(kind, n_bits)) {
        set_error("mapper_step_batched: out_stride must hold a row of symbols");
        return SRCDSP_ERR_SIZE;
    }
    if (n_bits == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_bits != nullptr && d_out != nullptr, "mapper_step_batched: null buffer");
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = mapper_launch(hs[0]->m, hs + c0, std::min(kMaxBatch, channels - c0), chan_row(d_bits, c0, bits_stride, 1),
                           bits_stride, chan_row(d_out, c0, out_stride), out_stride, n_bits, kMapperSymbols,
                           (hipStream_t)stream);
    return rc;
}

// step() (modulators.h:103-117, :169-184) on device buffers
SRCDSP_API int srcdsp_mapper_step(srcdsp_mapper_t h, const void *d_bits, size_t n_bits, void *d_out, size_t n_out,
                                  void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr, "mapper_step: null handle");
    int rc = mapper_check_size(h->m.kind, n_bits, n_out, "mapper_step");
    if (rc) return rc;
    if (n_bits == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_bits != nullptr && d_out != nullptr, "mapper_step: null buffer");
    return mapper_launch(h->m, &h, 1, d_bits, 0, d_out, 0, n_bits, kMapperSymbols, (hipStream_t)stream);
}

// step() on host buffers.  A handle whose state is on the host maps on the
// host, with the kernels' own arithmetic (mapper_host_run); one whose state
// the device holds stages the bits over and runs the kernels.
SRCDSP_API int srcdsp_mapper_step_host(srcdsp_mapper_t h, const void *bits, size_t n_bits, void *out, size_t n_out) {
    SRCDSP_ARG_CHECK(h != nullptr, "mapper_step_host: null handle");
    MapperState &m = h->m;
    int rc = mapper_check_size(m.kind, n_bits, n_out, "mapper_step_host");
    if (rc) return rc;
    if (n_bits == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(bits != nullptr && out != nullptr, "mapper_step_host: null buffer");
    if (!m.d_state) {
        m.state = (int)mapper_host_run(m.kind, (uint32_t)m.state, (const uint8_t *)bits, n_bits, (uint32_t *)out);
        return SRCDSP_OK;
    }
    if (!m.stage.stream) {
        rc = m.stage.init();
        if (rc) return rc;
    }
    const size_t bal = (n_bits + 255) & ~(size_t)255, ob = 4 * n_out;
    rc = m.stage.reserve(std::max(n_bits, ob), bal + ob);
    if (rc) return rc;
    hipStream_t s = m.stage.stream;
    char *d_b = (char *)m.stage.d_buf, *d_o = d_b + bal;
    host_copy(m.stage.h_buf, bits, n_bits);
    SRCDSP_HIP_TRY(hipMemcpyAsync(d_b, m.stage.h_buf, n_bits, hipMemcpyHostToDevice, s));
    rc = mapper_launch(m, &h, 1, d_b, 0, d_o, 0, n_bits, kMapperSymbols, s);
    if (rc) return rc;
    SRCDSP_HIP_TRY(hipMemcpyAsync(m.stage.h_buf, d_o, ob, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    host_copy(out, m.stage.h_buf, ob);
    return SRCDSP_OK;
}

}  // extern "C"
