// stagger.hip -- the OQPSK Q-rail stagger on gfx950: srcdsp_stagger_step and
// the bank srcdsp_stagger_step_batched (grid.y = row).  An extension with no
// reference class: a delay line of D samples on the imaginary rail, which an
// offset-QPSK transmitter puts between FilterUpsamplingFir::step
// (upsampling_filters.h:149-233) and Mixer::step (mixers.h:169-188).
//
// A plain streaming kernel.  A lane loads 4 samples as 16 bytes and stores 4 as
// 16 bytes (non-temporal: the output is written once); the imaginary halves
// from D samples back are read from global memory again, 2 bytes each, which
// the lane D/4 before has just loaded (a cache hit), or from the carry for the
// row's first D samples.  The first D lanes of a row's first workgroup write
// the new carry into the handle's other buffer.  The arithmetic is
// stagger_kernels.h, shared with the host.
#include <algorithm>

#include "stagger_state.h"

namespace srcdsp {
namespace {

struct StaggerLaunch {
    const uint32_t *in;
    uint32_t *out;
    long n;
    long in_stride, out_stride;  // words between rows (in_stride 0: one row for all)
    int D;
    int vec;                     // rows 16-byte aligned: dwordx4 loads and stores
    const int16_t *carry_in[kMaxBatch];
    int16_t *carry_out[kMaxBatch];
};

__global__ __launch_bounds__(kStaggerBlock) void stagger_stream(const StaggerLaunch P) {
    const int c = blockIdx.y;
    const uint32_t *in = P.in + c * P.in_stride;
    uint32_t *out = P.out + c * P.out_stride;
    const int16_t *carry = P.carry_in[c];
    const long D = P.D;
    if (blockIdx.x == 0 && (long)threadIdx.x < D)
        P.carry_out[c][threadIdx.x] = stagger_carry(carry, in, P.n, threadIdx.x, D);
    const long i0 = ((long)blockIdx.x * kStaggerBlock + threadIdx.x) * kStaggerLaneWords;
    if (i0 >= P.n) return;
    if (P.vec && i0 + kStaggerLaneWords <= P.n) {
        typedef uint32_t u4v_t __attribute__((ext_vector_type(4)));
        const u4v_t v = *(const u4v_t *)(in + i0);
        u4v_t w;
#pragma unroll
        for (int u = 0; u < kStaggerLaneWords; ++u) w[u] = stagger_word(v[u], stagger_q(carry, in, i0 + u, D));
        __builtin_nontemporal_store(w, (u4v_t *)(out + i0));
        return;
    }
    for (long i = i0; i < i0 + kStaggerLaneWords && i < P.n; ++i) out[i] = stagger_out(carry, in, i, D);
}

// words [a, a + an) and [b, b + bn) share a byte
bool spans_overlap(const void *a, size_t an, const void *b, size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 4 * bn && b0 < a0 + 4 * an;
}

// nc <= kMaxBatch staggers of one D over n > 0 samples each, checked by the caller
int stagger_launch(const srcdsp_stagger_t *hs, int nc, const void *d_in, size_t in_stride, void *d_out,
                   size_t out_stride, size_t n, hipStream_t s) {
    StaggerLaunch P{};
    P.in = (const uint32_t *)d_in;
    P.out = (uint32_t *)d_out;
    P.n = (long)n;
    P.in_stride = (long)in_stride;
    P.out_stride = (long)out_stride;
    P.D = (int)hs[0]->g.D;
    P.vec = aligned16(d_in) && aligned16(d_out) &&
            (nc == 1 || ((in_stride * 4) % 16 == 0 && (out_stride * 4) % 16 == 0));
    for (int c = 0; c < nc; ++c) {
        int rc = stagger_begin(hs[c]->g, s, P.carry_in[c], P.carry_out[c]);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)((n + kStaggerTileWords - 1) / kStaggerTileWords), (unsigned)nc);
    hipLaunchKernelGGL(stagger_stream, grid, dim3(kStaggerBlock), 0, s, P);
    SRCDSP_HIP_TRY(hipGetLastError());
    for (int c = 0; c < nc; ++c) {
        int rc = stagger_commit(hs[c]->g, s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

}  // namespace

int StaggerState::touch() {
    if (d_hist[0]) return SRCDSP_OK;
    int rc = order.init();
    if (rc) return rc;
    void *p = nullptr;
    SRCDSP_HIP_TRY(hipMalloc(&p, 2 * kStaggerMaxD * sizeof(int16_t)));
    d_hist[0] = p;
    d_hist[1] = (int16_t *)p + kStaggerMaxD;
    return SRCDSP_OK;
}

int StaggerState::fetch() {
    if (!on_dev) return SRCDSP_OK;
    int rc = order.sync();
    if (rc) return rc;
    SRCDSP_HIP_TRY(hipMemcpy(h_carry, d_hist[cur], D * sizeof(int16_t), hipMemcpyDeviceToHost));
    on_dev = false;
    return SRCDSP_OK;
}

int stagger_begin(StaggerState &g, hipStream_t s, const int16_t *&in, int16_t *&out) {
    int rc = g.touch();
    if (rc) return rc;
    if (!g.on_dev) {
        // the host holds the carry (a new, reset or fetched handle): a step still
        // in flight may be writing d_hist[cur], so wait for it, then send the carry
        rc = g.order.sync();
        if (rc) return rc;
        SRCDSP_HIP_TRY(hipMemcpy(g.d_hist[g.cur], g.h_carry, g.D * sizeof(int16_t), hipMemcpyHostToDevice));
        g.on_dev = true;
    }
    return chan_begin(g, s, in, out);
}

int stagger_commit(StaggerState &g, hipStream_t s) { return chan_commit(g, s); }

}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

// No device call: a handle is a host object until it steps on device buffers.
SRCDSP_API int srcdsp_stagger_create(srcdsp_stagger_t *out, unsigned D) {
    SRCDSP_ARG_CHECK(out != nullptr, "stagger_create: null out");
    *out = nullptr;
    SRCDSP_ARG_CHECK(D >= 1 && D <= kStaggerMaxD, "stagger_create: the delay D is 1..64 samples");
    auto *h = new srcdsp_stagger();
    h->g.D = D;
    *out = h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_stagger_destroy(srcdsp_stagger_t h) {
    if (!h) return SRCDSP_OK;
    StaggerState &g = h->g;
    if (g.d_hist[0]) {
        (void)g.order.sync();
        (void)hipFree(g.d_hist[0]);
        g.order.destroy();
    }
    g.scratch.destroy();
    if (g.stage.stream) g.stage.destroy();
    delete h;
    return SRCDSP_OK;
}

// a value copy: D and the carry
SRCDSP_API int srcdsp_stagger_clone(srcdsp_stagger_t h, srcdsp_stagger_t *out) {
    SRCDSP_ARG_CHECK(h != nullptr && out != nullptr, "stagger_clone: null argument");
    *out = nullptr;
    int rc = h->g.fetch();
    if (rc) return rc;
    auto *n = new srcdsp_stagger();
    n->g.D = h->g.D;
    std::copy(h->g.h_carry, h->g.h_carry + kStaggerMaxD, n->g.h_carry);
    *out = n;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_stagger_reset(srcdsp_stagger_t h) {
    SRCDSP_ARG_CHECK(h != nullptr, "stagger_reset: null handle");
    std::fill(h->g.h_carry, h->g.h_carry + kStaggerMaxD, (int16_t)0);
    h->g.on_dev = false;  // a step still in flight is waited for before the next one sends this carry
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_stagger_get_state(srcdsp_stagger_t h, unsigned *D, int16_t *carry) {
    SRCDSP_ARG_CHECK(h != nullptr, "stagger_get_state: null handle");
    int rc = h->g.fetch();
    if (rc) return rc;
    if (D) *D = h->g.D;
    if (carry) std::copy(h->g.h_carry, h->g.h_carry + h->g.D, carry);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_stagger_geometry(int *tile_samples, unsigned *max_delay) {
    if (tile_samples) *tile_samples = kStaggerTileWords;
    if (max_delay) *max_delay = kStaggerMaxD;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_stagger_step(srcdsp_stagger_t h, const void *d_in, size_t n, void *d_out, void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr, "stagger_step: null handle");
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in != nullptr && d_out != nullptr, "stagger_step: null buffer");
    SRCDSP_ARG_CHECK(!spans_overlap(d_in, n, d_out, n), "stagger_step: d_in and d_out may not overlap");
    return stagger_launch(&h, 1, d_in, 0, d_out, 0, n, (hipStream_t)stream);
}

// C staggers in one call: row c is srcdsp_stagger_step(hs[c], ...)
SRCDSP_API int srcdsp_stagger_step_batched(const srcdsp_stagger_t *hs, int channels, const void *d_in,
                                           size_t in_stride, void *d_out, size_t out_stride, size_t n, void *stream) {
    SRCDSP_ARG_CHECK(hs != nullptr && channels >= 1, "stagger_step_batched: no handles");
    int rc = check_handles(hs, channels, "stagger_step_batched");
    if (rc) return rc;
    for (int c = 1; c < channels; ++c)
        SRCDSP_ARG_CHECK(hs[c]->g.D == hs[0]->g.D, "stagger_step_batched: staggers must share D");
    SRCDSP_ARG_CHECK(in_stride == 0 || in_stride >= n, "stagger_step_batched: in_stride must be 0 (shared) or >= n");
    if (out_stride < n) {
        set_error("stagger_step_batched: out_stride must hold a row of n samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_in != nullptr && d_out != nullptr, "stagger_step_batched: null buffer");
    const size_t last = (size_t)channels - 1;
    SRCDSP_ARG_CHECK(!spans_overlap(d_in, last * in_stride + n, d_out, last * out_stride + n),
                     "stagger_step_batched: d_in and d_out may not overlap");
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = stagger_launch(hs + c0, std::min(kMaxBatch, channels - c0), chan_row(d_in, c0, in_stride), in_stride,
                            chan_row(d_out, c0, out_stride), out_stride, n, (hipStream_t)stream);
    return rc;
}

// step on host buffers.  A handle whose carry is on the host runs on the host,
// with the kernel's own arithmetic (stagger_host_run); one whose carry the
// device holds stages the samples over and runs the kernel.
SRCDSP_API int srcdsp_stagger_step_host(srcdsp_stagger_t h, const void *in, size_t n, void *out) {
    SRCDSP_ARG_CHECK(h != nullptr, "stagger_step_host: null handle");
    if (n == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(in != nullptr && out != nullptr, "stagger_step_host: null buffer");
    SRCDSP_ARG_CHECK(!spans_overlap(in, n, out, n), "stagger_step_host: in and out may not overlap");
    StaggerState &g = h->g;
    if (!g.on_dev) {
        stagger_host_run(g.h_carry, g.D, (const uint32_t *)in, n, (uint32_t *)out);
        return SRCDSP_OK;
    }
    int rc = SRCDSP_OK;
    if (!g.stage.stream) {
        rc = g.stage.init();
        if (rc) return rc;
    }
    const size_t nb = 4 * n, bal = (nb + 255) & ~(size_t)255;
    rc = g.stage.reserve(nb, 2 * bal);
    if (rc) return rc;
    hipStream_t s = g.stage.stream;
    char *d_i = (char *)g.stage.d_buf, *d_o = d_i + bal;
    host_copy(g.stage.h_buf, in, nb);
    SRCDSP_HIP_TRY(hipMemcpyAsync(d_i, g.stage.h_buf, nb, hipMemcpyHostToDevice, s));
    rc = stagger_launch(&h, 1, d_i, 0, d_o, 0, n, s);
    if (rc) return rc;
    SRCDSP_HIP_TRY(hipMemcpyAsync(g.stage.h_buf, d_o, nb, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    host_copy(out, g.stage.h_buf, nb);
    return SRCDSP_OK;
}

}  // extern "C"
