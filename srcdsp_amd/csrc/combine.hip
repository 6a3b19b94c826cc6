// combine.hip -- the carrier combiner on gfx950: srcdsp_combine_step and its
// host-buffer form.  An extension with no reference call: `rows` rows of
// complex<int16_t> summed sample by sample in int32 and put back on int16
// through the reference's limitScale (dsp_complex.h:83-108).  Stateless, like
// srcdsp_fill_synthetic: no handle.
//
// A persistent streaming kernel: kCombineWgPerCu workgroups per compute unit
// stride over tiles of 1024 samples.  A lane owns 4 consecutive samples: one
// 16-byte load per row (non-temporal: every input byte is read once; four rows'
// loads issued together, or one for a few long rows), 8 int32 sums in
// registers, one non-temporal 16-byte store.  (rows + 1) * 4 bytes move
// per sample and nothing is read twice.  Rows whose base or stride is off 16
// bytes, and the last n % 4 samples, take the scalar path.  A lane reads every
// row's samples before it stores its own, and no other lane touches them, so
// the output may be row 0 itself.  The arithmetic is combine_kernels.h, shared
// with the host.
#include <algorithm>
#include <atomic>

#include "ops.h"
#include "combine_kernels.h"

namespace srcdsp {
namespace {

typedef uint32_t c4v_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void combine_add4(int32_t (&re)[4], int32_t (&im)[4], const c4v_t v) {
#pragma unroll
    for (int u = 0; u < kCombineLaneWords; ++u) combine_add(re[u], im[u], v[u]);
}

// vec: the row bases and the stride are 16-byte aligned; U: rows in flight
template <int U>
__global__ __launch_bounds__(kCombineBlock) void combine_rows(const uint32_t *in, long stride, long rows, long n,
                                                              unsigned shift, int vec, uint32_t *out) {
    const long ntiles = (n + kCombineTileWords - 1) / kCombineTileWords;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long i0 = tile * kCombineTileWords + (long)threadIdx.x * kCombineLaneWords;
        if (i0 >= n) continue;
        if (vec && i0 + kCombineLaneWords <= n) {
            int32_t re[4] = {0, 0, 0, 0}, im[4] = {0, 0, 0, 0};
            const uint32_t *p = in + i0;
            long c = 0;
            if constexpr (U > 1) {
                for (; c + U <= rows; c += U) {
                    c4v_t v[U];
#pragma unroll
                    for (int k = 0; k < U; ++k) v[k] = __builtin_nontemporal_load((const c4v_t *)(p + (c + k) * stride));
#pragma unroll
                    for (int k = 0; k < U; ++k) combine_add4(re, im, v[k]);
                }
            }
            for (; c < rows; ++c) combine_add4(re, im, __builtin_nontemporal_load((const c4v_t *)(p + c * stride)));
            c4v_t w;
#pragma unroll
            for (int u = 0; u < kCombineLaneWords; ++u) w[u] = combine_word(re[u], im[u], shift);
            __builtin_nontemporal_store(w, (c4v_t *)(out + i0));
            continue;
        }
        for (long i = i0; i < i0 + kCombineLaneWords && i < n; ++i) out[i] = combine_sample(in, stride, rows, i, shift);
    }
}

// persistent workgroups of a launch on the current device, asked once per device
constexpr int kCombineDevices = 64;
std::atomic<int> g_combine_wgs[kCombineDevices];

int combine_workgroups(int *out) {
    int dev = 0, cus = 0;
    SRCDSP_HIP_TRY(hipGetDevice(&dev));
    const bool slot = dev >= 0 && dev < kCombineDevices;
    int w = slot ? g_combine_wgs[dev].load(std::memory_order_relaxed) : 0;
    if (!w) {
        SRCDSP_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        w = kCombineWgPerCu * (cus > 0 ? cus : 1);
        if (slot) g_combine_wgs[dev].store(w, std::memory_order_relaxed);
    }
    *out = w;
    return SRCDSP_OK;
}

int combine_check(const void *in, size_t rows, unsigned shift, const void *out, size_t n, const char *who) {
    SRCDSP_ARG_CHECK(rows >= 1 && rows <= (size_t)kCombineMaxRows, std::string(who) + ": rows is 1..65535");
    SRCDSP_ARG_CHECK(shift <= kCombineMaxShift, std::string(who) + ": shift is 0..15");
    SRCDSP_ARG_CHECK(n == 0 || (in != nullptr && out != nullptr), std::string(who) + ": null buffer");
    return SRCDSP_OK;
}

// the checked call, n > 0
int combine_launch(const void *d_in, size_t in_stride, size_t rows, void *d_out, size_t n, unsigned shift,
                   hipStream_t s) {
    int wgs = 0;
    int rc = combine_workgroups(&wgs);
    if (rc) return rc;
    const size_t ntiles = (n + kCombineTileWords - 1) / kCombineTileWords;
    const int vec = aligned16(d_in) && aligned16(d_out) && (rows == 1 || (in_stride * 4) % 16 == 0);
    const dim3 grid((unsigned)std::min<size_t>(ntiles, (size_t)wgs));
#ifdef SRCDSP_COMBINE_FORCE_ROWS_IN_FLIGHT  // a tuning build: one U for every shape (scripts/combine_ab.py)
    hipLaunchKernelGGL(combine_rows<SRCDSP_COMBINE_FORCE_ROWS_IN_FLIGHT>, grid, dim3(kCombineBlock), 0, s,
                       (const uint32_t *)d_in, (long)in_stride, (long)rows, (long)n, shift, vec, (uint32_t *)d_out);
#else
    if (rows <= (size_t)kCombineFewRows && n >= (size_t)kCombineLongRow) {
        hipLaunchKernelGGL(combine_rows<1>, grid, dim3(kCombineBlock), 0, s, (const uint32_t *)d_in, (long)in_stride,
                           (long)rows, (long)n, shift, vec, (uint32_t *)d_out);
    } else {
        hipLaunchKernelGGL(combine_rows<kCombineRowsInFlight>, grid, dim3(kCombineBlock), 0, s, (const uint32_t *)d_in,
                           (long)in_stride, (long)rows, (long)n, shift, vec, (uint32_t *)d_out);
    }
#endif
    SRCDSP_HIP_TRY(hipGetLastError());
    return SRCDSP_OK;
}

}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_combine_step(const void *d_in, size_t in_stride, size_t rows, void *d_out, size_t n,
                                   unsigned shift, void *stream) {
    int rc = combine_check(d_in, rows, shift, d_out, n, "combine_step");
    if (rc || n == 0) return rc;
    return combine_launch(d_in, in_stride, rows, d_out, n, shift, (hipStream_t)stream);
}

// no HIP call: the kernel's arithmetic on the host
SRCDSP_API int srcdsp_combine_step_host(const void *in, size_t in_stride, size_t rows, void *out, size_t n,
                                        unsigned shift) {
    int rc = combine_check(in, rows, shift, out, n, "combine_step_host");
    if (rc || n == 0) return rc;
    combine_host_run((const uint32_t *)in, in_stride, rows, n, shift, (uint32_t *)out);
    return SRCDSP_OK;
}

}  // extern "C"
