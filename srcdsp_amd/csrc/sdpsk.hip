// sdpsk.hip -- the differential SDPSK demodulator on gfx950: srcdsp_sdpsk_step,
// the bank srcdsp_sdpsk_step_batched (grid.y = row) and the host-buffer form.
// An extension with no reference class: the receiver of SymbolMapperSdpsk
// (modulators.h:82-131), bit = sign of Im(x[i] * conj(x[i - D])), soft bit =
// limitScale<int8_t, int32_t> of it (dsp_complex.h:45-63).  No PLL and no
// recurrence: every output is independent, a burst costs one memory pass.
//
// A plain streaming kernel, one workgroup per tile of kSdpskTileWords samples
// and row.  A lane loads kSdpskLaneWords samples as 16-byte words into LDS; the
// D samples before the tile (the previous tile's last D, or the carry for the
// call's first tile) are staged in front of them, and every lane reads its
// samples and their predecessors from LDS.  The 16-byte loads start at the
// 16-byte boundary at or below the tile's first sample, so a row at any sample
// offset (a bank fed from hit indices) is read with the same loads; the words
// of an edge chunk that lie outside the tile are not loaded.  A lane packs 4
// soft bits and 4 bits and stores each as one 32-bit word (byte by byte where
// the output row is off a 4-byte boundary, or at the row's end).  The last tile
// of a row writes the new carry, from LDS, into the handle's other carry
// buffer.  The arithmetic is sdpsk_kernels.h, shared with the host.
//
// A bank call uploads one table row per handle (input pointer, the two carry
// buffers) and records one event, which its handles share; nothing comes back
// to the host, so every step is asynchronous on its stream.
#include <algorithm>
#include <memory>
#include <vector>

#include "ops.h"
#include "sdpsk_kernels.h"

namespace srcdsp {

constexpr int kSdpskTabSlots = 4;

// The event recorded behind a step.  The handles of a bank call share one: an
// event of its own per handle (Ordering, as the other banks have it) costs a
// wait and a record per row on the host, 4.7 us per row measured, more than the
// kernel's time for a bank of short rows.
struct StepEvent {
    hipEvent_t ev = nullptr;
    ~StepEvent() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// A host object until it steps on the device (create makes no device call).
// The carry then lives in d_hist[cur], double-buffered like the stagger's: a
// step reads d_hist[cur] and writes d_hist[cur ^ 1].

struct SdpskState {
    unsigned D = 1, shift = 0;
    uint32_t h_carry[kSdpskMaxD] = {};  // the host copy: current unless on_dev
    bool on_dev = false;                // the last step left the carry in d_hist[cur]
    void *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    std::shared_ptr<StepEvent> done;    // behind the handle's last step on device buffers, or null
    // scratch of the bank calls this handle led: the row table on the device
    // and its pinned image, a ring of kSdpskTabSlots.  `done` is recorded behind
    // the launch that reads a slot; the call that takes the slot again waits for
    // it on the host before it rewrites the image
    struct Tab {
        GrowBuf buf;
        Ordering done;
    } tab[kSdpskTabSlots];
    unsigned tab_at = 0;

    int touch();  // the device buffers, once
    int sync();   // the host waits for the last step
    int fetch();  // waits for the last step; the carry back on the host
};

namespace {

struct SdpskRow {
    const uint32_t *in;
    const uint32_t *carry_in;
    uint32_t *carry_out;
};

struct SdpskLaunch {
    SdpskRow row0;         // the row of a launch of one
    const SdpskRow *rows;  // the table of a bank's launch, or null
    int8_t *soft;          // either may be null
    uint8_t *bits;
    long soft_stride, bits_stride;  // bytes between rows
    long n;
    int D;
    unsigned shift;
};

constexpr int kSdpskLds = (int)kSdpskMaxD + 4 + kSdpskTileWords;  // halo | alignment slack | tile
typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));

// one sample's outputs, byte by byte
__device__ __forceinline__ void sdpsk_store1(int8_t *soft, uint8_t *bits, long i, int32_t tq, unsigned shift) {
    if (soft) soft[i] = (int8_t)sdpsk_soft(tq, shift);
    if (bits) bits[i] = (uint8_t)sdpsk_bit(tq);
}

__global__ __launch_bounds__(kSdpskBlock) void sdpsk_rows(const SdpskLaunch P) {
    constexpr int T = kSdpskTileWords;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kSdpskLds];
    const long c = blockIdx.y;
    const SdpskRow r = P.rows ? P.rows[c] : P.row0;
    int8_t *soft = P.soft ? P.soft + c * P.soft_stride : nullptr;
    uint8_t *bits = P.bits ? P.bits + c * P.bits_stride : nullptr;
    const int lane = threadIdx.x, D = P.D;
    const long t0 = (long)blockIdx.x * T;
    const int cnt = (int)min((long)T, P.n - t0);  // samples of this tile, >= 1
    const bool last = blockIdx.x == gridDim.x - 1;
    const uint32_t *p = r.in + t0;
    const int m = (int)(((uintptr_t)p >> 2) & 3u);  // words p lies past a 16-byte boundary

#ifdef SRCDSP_SDPSK_UNALIGNED_SCALAR  // a tuning build: rows off 16 bytes go sample by sample (scripts/sdpsk_time.py)
    if (m != 0) {
        if (last && lane < D) r.carry_out[lane] = sdpsk_v(r.carry_in, r.in, P.n + lane, D);
        for (int w = lane; w < cnt; w += kSdpskBlock)
            sdpsk_store1(soft, bits, t0 + w, sdpsk_tq(p[w], sdpsk_v(r.carry_in, r.in, t0 + w, D)), P.shift);
        return;
    }
#endif

    // tile[w] = in[t0 + w] for 0 <= w < cnt, tile[w - D] its predecessor; chunk j
    // is the 16 bytes at p - m + 4 j, which lands on lds[kSdpskMaxD + 4 j]
    // Every load is issued before the first LDS write waits for one.
    uint32_t *tile = lds + kSdpskMaxD + m;
    u4v_t v[kSdpskLaneWords / 4];
#pragma unroll
    for (int k = 0; k < kSdpskLaneWords / 4; ++k) {
        const int w0 = 4 * (k * kSdpskBlock + lane) - m;
        if (w0 >= 0 && w0 + 4 <= cnt) {
            v[k] = *(const u4v_t *)(p + w0);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[k][u] = (w0 + u >= 0 && w0 + u < cnt) ? p[w0 + u] : 0u;
        }
    }
    const bool has_tail = lane < m && T - m + lane < cnt;  // the words past the last chunk
    const uint32_t tail = has_tail ? p[T - m + lane] : 0u;
    const uint32_t halo = lane < D ? sdpsk_v(r.carry_in, r.in, t0 + lane, D) : 0u;
#pragma unroll
    for (int k = 0; k < kSdpskLaneWords / 4; ++k) {
        const int w0 = 4 * (k * kSdpskBlock + lane) - m;
        if (w0 >= 0 && w0 + 4 <= cnt) {
            *(u4v_t *)(tile + w0) = v[k];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (w0 + u >= 0 && w0 + u < cnt) tile[w0 + u] = v[k][u];
        }
    }
    if (has_tail) tile[T - m + lane] = tail;
    if (lane < D) tile[lane - D] = halo;
    __syncthreads();

    // carry'[k] = v[n + k] = tile[n + k - D - t0]
    if (last && lane < D) r.carry_out[lane] = tile[cnt - D + lane];

    const bool soft_vec = soft && ((uintptr_t)soft & 3u) == 0, bits_vec = bits && ((uintptr_t)bits & 3u) == 0;
#pragma unroll
    for (int k = 0; k < kSdpskLaneWords / 4; ++k) {
        const int i0 = 4 * (k * kSdpskBlock + lane);
        if (i0 >= cnt) continue;
        int32_t tq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tq[u] = sdpsk_tq(tile[i0 + u], tile[i0 + u - D]);
        const bool full = i0 + 4 <= cnt;
        if (full && soft_vec) {
            uint32_t w = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) w |= ((uint32_t)sdpsk_soft(tq[u], P.shift) & 0xffu) << (8 * u);
            *(uint32_t *)(soft + t0 + i0) = w;
        } else if (soft) {
            for (int u = 0; u < 4 && i0 + u < cnt; ++u) soft[t0 + i0 + u] = (int8_t)sdpsk_soft(tq[u], P.shift);
        }
        if (full && bits_vec) {
            uint32_t w = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) w |= sdpsk_bit(tq[u]) << (8 * u);
            *(uint32_t *)(bits + t0 + i0) = w;
        } else if (bits) {
            for (int u = 0; u < 4 && i0 + u < cnt; ++u) bits[t0 + i0 + u] = (uint8_t)sdpsk_bit(tq[u]);
        }
    }
}

// The stream waits for the handle's last step (once per event: `waited` holds
// the events this call has waited for), a carry the host holds is sent to
// d_hist[cur], and the buffers the step reads and writes are named.
int sdpsk_begin(SdpskState &g, hipStream_t s, SdpskRow &row, std::vector<const StepEvent *> &waited) {
    int rc = g.touch();
    if (rc) return rc;
    if (!g.on_dev) {
        // a step still in flight may be writing d_hist[cur]: wait, then send the carry
        rc = g.sync();
        if (rc) return rc;
        SRCDSP_HIP_TRY(hipMemcpy(g.d_hist[g.cur], g.h_carry, g.D * sizeof(uint32_t), hipMemcpyHostToDevice));
        g.on_dev = true;
    }
    hist_pair(g, row.carry_in, row.carry_out);
    const StepEvent *e = g.done.get();
    if (e && (waited.empty() || waited.back() != e) && std::find(waited.begin(), waited.end(), e) == waited.end()) {
        SRCDSP_HIP_TRY(hipStreamWaitEvent(s, e->ev, 0));
        waited.push_back(e);
    }
    return SRCDSP_OK;
}

// One event behind the call's launches, shared by its handles; each handle's
// written carry becomes the current one.  The lead's event is used again when
// no other handle holds it.
int sdpsk_commit(SdpskState *const *gs, size_t channels, hipStream_t s) {
    std::shared_ptr<StepEvent> e = gs[0]->done;
    if (!e || e.use_count() > 2) {  // held by the lead and by `e`, and by nobody else
        e = std::make_shared<StepEvent>();
        SRCDSP_HIP_TRY(hipEventCreateWithFlags(&e->ev, hipEventDisableTiming));
    }
    SRCDSP_HIP_TRY(hipEventRecord(e->ev, s));
    for (size_t c = 0; c < channels; ++c) {
        gs[c]->cur ^= 1;
        gs[c]->done = e;
    }
    return SRCDSP_OK;
}

// channels >= 1 demodulators of one D and shift over n > 0 samples each, checked by the caller
int sdpsk_launch(SdpskState *const *gs, size_t channels, const uint32_t *d_in, size_t in_stride,
                 const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride, uint8_t *d_bits,
                 size_t bits_stride, hipStream_t s) {
    const size_t ntiles = (n + kSdpskTileWords - 1) / kSdpskTileWords;
    if (ntiles > 0x7fffffffUL) {
        set_error("sdpsk_step: more tiles than a launch takes");
        return SRCDSP_ERR_SIZE;
    }
    SdpskState &lead = *gs[0];
    SdpskLaunch P{};
    P.n = (long)n;
    P.D = (int)lead.D;
    P.shift = lead.shift;
    P.soft_stride = (long)soft_stride;
    P.bits_stride = (long)bits_stride;
    int rc = SRCDSP_OK;
    SdpskRow *tab = &P.row0;
    SdpskState::Tab *slot = nullptr;
    if (channels > 1) {
        slot = &lead.tab[lead.tab_at++ % kSdpskTabSlots];
        if (!slot->done.ev) rc = slot->done.init();
        if (!rc) rc = slot->done.sync();  // the launch that read this slot last
        if (!rc) rc = slot->buf.reserve(channels * sizeof(SdpskRow));
        if (rc) return rc;
        tab = slot->buf.host<SdpskRow>();
    }
    std::vector<const StepEvent *> waited;
    for (size_t c = 0; c < channels; ++c) {
        tab[c].in = d_in + c * in_stride + (in_offset ? in_offset[c] : 0);
        rc = sdpsk_begin(*gs[c], s, tab[c], waited);
        if (rc) return rc;
    }
    if (slot) SRCDSP_HIP_TRY(hipMemcpyAsync(slot->buf.d, tab, channels * sizeof(SdpskRow), hipMemcpyHostToDevice, s));
    for (size_t c0 = 0; c0 < channels; c0 += (size_t)kSdpskMaxRows) {
        const size_t nc = std::min((size_t)kSdpskMaxRows, channels - c0);
        P.rows = slot ? slot->buf.dev<const SdpskRow>() + c0 : nullptr;
        P.soft = d_soft ? d_soft + c0 * soft_stride : nullptr;
        P.bits = d_bits ? d_bits + c0 * bits_stride : nullptr;
        hipLaunchKernelGGL(sdpsk_rows, dim3((unsigned)ntiles, (unsigned)nc), dim3(kSdpskBlock), 0, s, P);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    if (slot) {
        rc = slot->done.after(s);
        if (rc) return rc;
    }
    return sdpsk_commit(gs, channels, s);
}

}  // namespace

int SdpskState::touch() {
    if (d_hist[0]) return SRCDSP_OK;
    void *p = nullptr;
    SRCDSP_HIP_TRY(hipMalloc(&p, 2 * kSdpskMaxD * sizeof(uint32_t)));
    d_hist[0] = p;
    d_hist[1] = (uint32_t *)p + kSdpskMaxD;
    return SRCDSP_OK;
}

int SdpskState::sync() {
    if (done) SRCDSP_HIP_TRY(hipEventSynchronize(done->ev));
    return SRCDSP_OK;
}

int SdpskState::fetch() {
    if (!on_dev) return SRCDSP_OK;
    int rc = sync();
    if (rc) return rc;
    SRCDSP_HIP_TRY(hipMemcpy(h_carry, d_hist[cur], D * sizeof(uint32_t), hipMemcpyDeviceToHost));
    on_dev = false;
    return SRCDSP_OK;
}

}  // namespace srcdsp

struct srcdsp_sdpsk { srcdsp::SdpskState g; };

using namespace srcdsp;

extern "C" {

// No device call: a handle is a host object until it steps on device buffers.
SRCDSP_API int srcdsp_sdpsk_create(srcdsp_sdpsk_t *out, unsigned D, unsigned shift) {
    SRCDSP_ARG_CHECK(out != nullptr, "sdpsk_create: null out");
    *out = nullptr;
    SRCDSP_ARG_CHECK(D >= 1 && D <= kSdpskMaxD, "sdpsk_create: the lag D is 1..64 samples");
    SRCDSP_ARG_CHECK(shift <= kSdpskMaxShift, "sdpsk_create: shift is 0..31");
    auto *h = new srcdsp_sdpsk();
    h->g.D = D;
    h->g.shift = shift;
    *out = h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_sdpsk_destroy(srcdsp_sdpsk_t h) {
    if (!h) return SRCDSP_OK;
    SdpskState &g = h->g;
    if (g.d_hist[0]) {
        (void)g.sync();
        (void)hipFree(g.d_hist[0]);
    }
    for (SdpskState::Tab &t : g.tab) {
        (void)t.done.sync();
        t.buf.destroy();
        t.done.destroy();
    }
    delete h;
    return SRCDSP_OK;
}

// a value copy: D, the shift and the carry
SRCDSP_API int srcdsp_sdpsk_clone(srcdsp_sdpsk_t h, srcdsp_sdpsk_t *out) {
    SRCDSP_ARG_CHECK(h != nullptr && out != nullptr, "sdpsk_clone: null argument");
    *out = nullptr;
    int rc = h->g.fetch();
    if (rc) return rc;
    auto *n = new srcdsp_sdpsk();
    n->g.D = h->g.D;
    n->g.shift = h->g.shift;
    std::copy(h->g.h_carry, h->g.h_carry + kSdpskMaxD, n->g.h_carry);
    *out = n;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_sdpsk_reset(srcdsp_sdpsk_t h) {
    SRCDSP_ARG_CHECK(h != nullptr, "sdpsk_reset: null handle");
    std::fill(h->g.h_carry, h->g.h_carry + kSdpskMaxD, 0u);
    h->g.on_dev = false;  // a step still in flight is waited for before the next one sends this carry
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_sdpsk_set_shift(srcdsp_sdpsk_t h, unsigned shift) {
    SRCDSP_ARG_CHECK(h != nullptr, "sdpsk_set_shift: null handle");
    SRCDSP_ARG_CHECK(shift <= kSdpskMaxShift, "sdpsk_set_shift: shift is 0..31");
    h->g.shift = shift;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_sdpsk_get_state(srcdsp_sdpsk_t h, unsigned *D, unsigned *shift, int16_t *carry) {
    SRCDSP_ARG_CHECK(h != nullptr, "sdpsk_get_state: null handle");
    int rc = h->g.fetch();
    if (rc) return rc;
    if (D) *D = h->g.D;
    if (shift) *shift = h->g.shift;
    if (carry) memcpy(carry, h->g.h_carry, h->g.D * sizeof(uint32_t));
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_sdpsk_geometry(int *tile_samples, unsigned *max_lag, int *workgroups) {
    if (tile_samples) *tile_samples = kSdpskTileWords;
    if (max_lag) *max_lag = kSdpskMaxD;
    if (workgroups) *workgroups = 0;  // not persistent: one workgroup per tile and row
    return SRCDSP_OK;
}

// C demodulators in one call: row c is srcdsp_sdpsk_step(hs[c], ...)
SRCDSP_API int srcdsp_sdpsk_step_batched(const srcdsp_sdpsk_t *hs, int channels, const void *d_in, size_t in_stride,
                                         const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride,
                                         uint8_t *d_bits, size_t bits_stride, void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && channels >= 1, "sdpsk_step_batched: no handles");
    int rc = check_handles(hs, channels, "sdpsk_step_batched");
    if (rc) return rc;
    for (int c = 1; c < channels; ++c)
        SRCDSP_ARG_CHECK(hs[c]->g.D == hs[0]->g.D && hs[c]->g.shift == hs[0]->g.shift,
                         "sdpsk_step_batched: demodulators must share D and the shift");
    if ((d_soft && soft_stride < n) || (d_bits && bits_stride < n)) {
        set_error("sdpsk_step_batched: an output stride must hold a row of n outputs");
        return SRCDSP_ERR_SIZE;
    }
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in != nullptr && (d_soft != nullptr || d_bits != nullptr), "sdpsk_step_batched: null buffer");
    std::vector<SdpskState *> gs((size_t)channels);
    for (int c = 0; c < channels; ++c) gs[(size_t)c] = &hs[c]->g;
    return sdpsk_launch(gs.data(), (size_t)channels, (const uint32_t *)d_in, in_stride, in_offset, n, d_soft,
                        soft_stride, d_bits, bits_stride, (hipStream_t)stream);
}

SRCDSP_API int srcdsp_sdpsk_step(srcdsp_sdpsk_t h, const void *d_in, size_t n, int8_t *d_soft, uint8_t *d_bits,
                                 void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr, "sdpsk_step: null handle");
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in != nullptr && (d_soft != nullptr || d_bits != nullptr), "sdpsk_step: null buffer");
    SdpskState *g = &h->g;
    return sdpsk_launch(&g, 1, (const uint32_t *)d_in, 0, nullptr, n, d_soft, n, d_bits, n, (hipStream_t)stream);
}

// The kernel's arithmetic on the host.  A handle that has not stepped on device
// buffers makes no HIP call; one whose carry the device holds takes it back
// first (waits for its last step).
SRCDSP_API int srcdsp_sdpsk_step_host(srcdsp_sdpsk_t h, const void *in, size_t n, int8_t *soft, uint8_t *bits) {
    SRCDSP_ARG_CHECK(h != nullptr, "sdpsk_step_host: null handle");
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(in != nullptr && (soft != nullptr || bits != nullptr), "sdpsk_step_host: null buffer");
    SdpskState &g = h->g;
    int rc = g.fetch();
    if (rc) return rc;
    sdpsk_host_run(g.h_carry, g.D, g.shift, (const uint32_t *)in, n, soft, bits);
    return SRCDSP_OK;
}

}  // extern "C"
