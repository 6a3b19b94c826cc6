// freqest.hip -- estimateFreq<int16_t, L> (dsptl_miscellaneous.h:43-58) on
// gfx950: srcdsp_freqest_run, its bank srcdsp_freqest_run_batched and the
// host-buffer form, one kernel for all three (freqest_kernels.h; the single
// row is the bank at one row).
//
// A handle holds L and the scratch of its calls; it has no signal state.  A
// call launches freqest_rows (and freqest_finish when a row was given more than
// one workgroup), takes one pinned row of 4 words per channel back in one copy
// and synchronises once, whatever the number of rows; the atan2 is the host's.
#include <algorithm>
#include <vector>

#include "ops.h"
#include "freqest_kernels.h"

namespace srcdsp {

struct FreqEst {
    int L = 1;
    int max_wg = 0;  // persistent workgroups of a launch: kFreqWgPerCu per compute unit, asked once
    // scratch: slabs on the device, result rows there and their pinned mirror,
    // the row offsets (pinned, and their device copy)
    GrowBuf slab{GrowBuf::kDevice}, res, off;
    HostStage stage;  // srcdsp_freqest_run_host
};

namespace {

int freqest_workgroups(int *out) {
    int dev = 0, cus = 0;
    SRCDSP_HIP_TRY(hipGetDevice(&dev));
    SRCDSP_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    *out = kFreqWgPerCu * (cus > 0 ? cus : 1);
    return SRCDSP_OK;
}

// the results of one row from its 4 words
void freqest_result(const long long *row, size_t pairs, int L, float *freq, int64_t *sums, int *exact) {
    *freq = static_cast<float>(std::atan2((double)row[1], (double)row[0]) / L);
    if (sums) {
        sums[0] = row[0];
        sums[1] = row[1];
    }
    if (exact) *exact = freqest_exact(pairs, freqest_bound(row[2], row[3]));
}

// the checked call, n > L: launch, rows back, one synchronisation
int freqest_launch(FreqEst &f, int channels, const uint32_t *d_in, size_t in_stride, const size_t *in_offset, size_t n,
                   float *freq, int64_t *sums, int *exact, hipStream_t s) {
    if (!f.max_wg) {
        int rc = freqest_workgroups(&f.max_wg);
        if (rc) return rc;
    }
    const size_t C = (size_t)channels, pairs = n - (size_t)f.L;
    const size_t ntiles = (pairs + kFreqTile - 1) / kFreqTile;
    size_t bpr = std::max<size_t>(1, (size_t)f.max_wg / C);
    bpr = std::min(bpr, ntiles);
    const size_t tiles_per_wg = (ntiles + bpr - 1) / bpr;
    bpr = (ntiles + tiles_per_wg - 1) / tiles_per_wg;  // no workgroup without a tile
    if (C * bpr > 0x7fffffffUL) {
        set_error("freqest: more workgroups than a launch takes");
        return SRCDSP_ERR_SIZE;
    }
    int rc = f.slab.reserve(bpr > 1 ? 8 * kFreqWords * C * bpr : 0);
    if (!rc) rc = f.res.reserve(8 * kFreqWords * C);
    if (!rc) rc = f.off.reserve(in_offset ? 8 * C : 0);
    if (rc) return rc;
    long long *d_slab = f.slab.dev<long long>(), *d_res = f.res.dev<long long>(), *h_res = f.res.host<long long>();
    if (in_offset) {
        long *h_off = f.off.host<long>();
        for (size_t c = 0; c < C; ++c) h_off[c] = (long)in_offset[c];
        SRCDSP_HIP_TRY(hipMemcpyAsync(f.off.d, h_off, 8 * C, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(freqest_rows, dim3((unsigned)(C * bpr)), dim3(kFreqLanes), 0, s, d_in, (long)in_stride,
                       in_offset ? f.off.dev<const long>() : nullptr, (long)n, (long)f.L, (int)bpr, (long)tiles_per_wg,
                       d_slab, d_res);
    SRCDSP_HIP_TRY(hipGetLastError());
    if (bpr > 1) {
        hipLaunchKernelGGL(freqest_finish, dim3((unsigned)C), dim3(64), 0, s, (const long long *)d_slab, (int)bpr,
                           d_res);
        SRCDSP_HIP_TRY(hipGetLastError());
    }
    SRCDSP_HIP_TRY(hipMemcpyAsync(h_res, d_res, 8 * kFreqWords * C, hipMemcpyDeviceToHost, s));
    SRCDSP_HIP_TRY(hipStreamSynchronize(s));
    for (size_t c = 0; c < C; ++c)
        freqest_result(h_res + kFreqWords * c, pairs, f.L, freq + c, sums ? sums + 2 * c : nullptr,
                       exact ? exact + c : nullptr);
    return SRCDSP_OK;
}

// n <= L: the reference's loop is empty, atan2(0, 0) / L = +0
void freqest_zeros(int channels, float *freq, int64_t *sums, int *exact) {
    for (int c = 0; c < channels; ++c) {
        freq[c] = 0.0f;
        if (sums) sums[2 * c] = sums[2 * c + 1] = 0;
        if (exact) exact[c] = 1;
    }
}

}  // namespace
}  // namespace srcdsp

struct srcdsp_freqest { srcdsp::FreqEst f; };

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_freqest_create(srcdsp_freqest_t *out, int L) {
    SRCDSP_ARG_CHECK(out != nullptr, "freqest_create: null out");
    SRCDSP_ARG_CHECK(L >= 1, "freqest_create: L is at least 1");
    *out = new srcdsp_freqest();
    (*out)->f.L = L;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_freqest_destroy(srcdsp_freqest_t h) {
    if (!h) return SRCDSP_OK;
    FreqEst &f = h->f;
    f.slab.destroy();
    f.res.destroy();
    f.off.destroy();
    if (f.stage.stream) f.stage.destroy();
    delete h;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_freqest_geometry(srcdsp_freqest_t h, int *L, int *tile, int *vec, int *workgroups) {
    SRCDSP_ARG_CHECK(h != nullptr, "freqest_geometry: null handle");
    if (L) *L = h->f.L;
    if (tile) *tile = kFreqTile;
    if (vec) *vec = kFreqVec;
    if (workgroups) {
        if (!h->f.max_wg) {
            int rc = freqest_workgroups(&h->f.max_wg);
            if (rc) return rc;
        }
        *workgroups = h->f.max_wg;
    }
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_freqest_run_batched(srcdsp_freqest_t h, int channels, const void *d_in, size_t in_stride,
                                          const size_t *in_offset, size_t n, float *freq, int64_t *sums, int *exact,
                                          void *stream) {
    SRCDSP_ARG_CHECK(h != nullptr && freq != nullptr, "freqest_run_batched: null handle or result array");
    SRCDSP_ARG_CHECK(channels >= 1, "freqest_run_batched: channels is at least 1");
    if (n > 0x7fffffffUL) {
        set_error("freqest_run_batched: input longer than INT_MAX samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n <= (size_t)h->f.L) {
        freqest_zeros(channels, freq, sums, exact);
        return SRCDSP_OK;
    }
    SRCDSP_ARG_CHECK(d_in != nullptr, "freqest_run_batched: null buffer");
    return freqest_launch(h->f, channels, (const uint32_t *)d_in, in_stride, in_offset, n, freq, sums, exact,
                          (hipStream_t)stream);
}

SRCDSP_API int srcdsp_freqest_run(srcdsp_freqest_t h, const void *d_in, size_t n, float *freq, int64_t sums[2],
                                  int *exact, void *stream) {
    return srcdsp_freqest_run_batched(h, 1, d_in, 0, nullptr, n, freq, sums, exact, stream);
}

SRCDSP_API int srcdsp_freqest_run_host(srcdsp_freqest_t h, const void *in, size_t n, float *freq, int64_t sums[2],
                                       int *exact) {
    SRCDSP_ARG_CHECK(h != nullptr && freq != nullptr, "freqest_run_host: null handle or result");
    if (n > 0x7fffffffUL) {
        set_error("freqest_run_host: input longer than INT_MAX samples");
        return SRCDSP_ERR_SIZE;
    }
    FreqEst &f = h->f;
    if (n <= (size_t)f.L) {
        freqest_zeros(1, freq, sums, exact);
        return SRCDSP_OK;
    }
    SRCDSP_ARG_CHECK(in != nullptr, "freqest_run_host: null buffer");
    int rc = SRCDSP_OK;
    if (!f.stage.stream) {
        rc = f.stage.init();
        if (rc) return rc;
    }
    rc = f.stage.reserve(4 * n, 4 * n);
    if (rc) return rc;
    host_copy(f.stage.h_buf, in, 4 * n);
    SRCDSP_HIP_TRY(hipMemcpyAsync(f.stage.d_buf, f.stage.h_buf, 4 * n, hipMemcpyHostToDevice, f.stage.stream));
    return freqest_launch(f, 1, (const uint32_t *)f.stage.d_buf, 0, nullptr, n, freq, sums, exact, f.stage.stream);
}

}  // extern "C"
