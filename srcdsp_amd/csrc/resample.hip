// resample.hip -- FilterUpsamplingFir -> FilterDnsamplingFir in one call: the
// rational L/M rate change (interpolate by L, upsampling_filters.h:149-233,
// then decimate by M, dnsampling_filters.h:129-172), single
// (srcdsp_resample_step) and as a bank of C chains in one launch
// (srcdsp_resample_step_batched).
//
// Every output is limitScale16(sum_k c_d[k] * mid[i M - k], coeffScaling -
// leftShift) over mid = limitScale<complex<int16_t>>(interpolator sums, 15 -
// round(log2 L)): the interpolator's asymmetric int16 clamp first
// (dsp_complex.h:83-108), the intermediate rounded to int16, then the
// decimator's taps and its symmetric clamp (dsp_complex.cpp:63-73).  Both
// handles end as the two calls leave them: the interpolator's history as
// srcdsp_up_step writes it, the decimator's as the last N_d - 1 interpolated
// samples of history ++ call.
//
// Two routes.  The fused kernel resample_tile_dot2 (resample_kernels.h) takes
// interpolator variant 0 with int16-range taps, L = 2..8, up to kUpMaxTaps
// taps; decimator variant 1 with int16-range taps, M = 1..8, up to
// kRsMaxDecimTaps taps; 16-byte aligned input and output (the bank: row
// strides of whole 16 bytes too).  Of these it serves the calls rs_route()
// names, which is decided by measurement: L/M = 4/3 and 2/3 from
// 2048 tiles on.  Every other legal call runs srcdsp_up_step into a grow-only
// scratch on the interpolator handle and srcdsp_decim_step from it, inside the
// call; the bank then loops over its channels.  The caller never sees the
// intermediate.
#include <algorithm>
#include <atomic>

#include "ops.h"

#include "resample_kernels.h"

namespace srcdsp {
namespace {
PathCounter g_fused_calls, g_pair_calls, g_bank_calls, g_loop_calls;

// > 0: set by srcdsp_resample_set_min_tiles, for every shape the kernel takes
std::atomic<long> g_min_tiles{0};

// The fewest tiles of a call (rows x tiles per row) from which the fused kernel
// serves a shape it takes; 0: never.  Measured (DESIGN 5.4c,
// profiles/resample_time.json), against the faster of two timings of the
// sequence srcdsp_up_step; srcdsp_decim_step: at M = 3 the kernel is 17 %
// faster at L = 4 and 10 % at L = 2 on 2^26 inputs, and at L = 4 the bank of
// 64 rows x 32 tiles is 2.1 x faster than the loop of 64 sequences; 2048 tiles
// is the smallest call measured.  At L/M = 8/5 it is 7 % slower and at 4/4,
// where the decimator has its own v_dot2 kernel, 41 % slower: those and every
// shape not measured run the pair.
constexpr long kRsMinTiles = 2048;
long rs_route(unsigned L, unsigned M) {
    const long forced = g_min_tiles.load(std::memory_order_relaxed);
    if (forced > 0) return forced;
    return M == 3 && (L == 2 || L == 4) ? kRsMinTiles : 0;
}

// the shapes the fused kernel takes, the routing aside
bool fused_takes(const srcdsp_up_state &u, const FirCore &f, const void *d_in, const void *d_out) {
    return u.variant == UV_CI16_I32 && u.coef_i16 && u.L >= 2 && u.L <= 8 && u.ntaps <= kUpMaxTaps &&
           f.kv == KV_CI16_I32 && f.coef_fits_i16 && f.M >= 1 && f.M <= 8 && f.ntaps <= kRsMaxDecimTaps &&
           aligned16(d_in) && aligned16(d_out);
}

bool fused_serves(const srcdsp_up_state &u, const FirCore &f, const void *d_in, const void *d_out, long n_total,
                  int channels) {
    if (!fused_takes(u, f, d_in, d_out)) return false;
    const long min_tiles = rs_route(u.L, f.M);
    return min_tiles > 0 && up_tiles(n_total) * channels >= min_tiles;
}

// nc <= kMaxBatch chains in one launch; the shape is one fused_takes accepts
int fused_launch(const srcdsp_up_t *ups, const srcdsp_decim_t *decims, int nc, const void *d_in, size_t in_stride,
                 void *d_out, size_t out_stride, size_t n_in, long n_total, long n_out, hipStream_t s) {
    srcdsp_up_state &u0 = ups[0]->u;
    FirCore &f0 = decims[0]->core;
    ResampleLaunch P{};
    P.in = (const uint32_t *)d_in;
    P.out = (uint32_t *)d_out;
    P.pairs = u0.d_pair;
    P.cpair = f0.d_cpair;
    P.n_in = (long)n_in;
    P.n_total = n_total;
    P.n_out = n_out;
    P.in_stride = (long)in_stride;
    P.out_stride = (long)out_stride;
    P.H = u0.H;
    P.Nd = f0.ntaps;
    P.M = (int)f0.M;
    P.shift_up = (unsigned)(15 - u0.left_shift_factor);
    P.shift_dn = f0.shift();
    const int PP = (u0.H + 1) / 2;
    P.HP = rs_halo_words(f0.ntaps);
    P.HG = rs_halo_granules(PP, (int)u0.L, P.HP);
    P.mid_off = (unsigned)rs_planes_bytes(P.HG);
    const size_t smem = rs_smem(u0.H, (int)u0.L, f0.ntaps);
    for (int c = 0; c < nc; ++c) {
        int rc = chan_begin(ups[c]->u, s, P.uhist_in[c], P.uhist_out[c]);
        if (!rc) rc = chan_begin(decims[c]->core, s, P.dhist_in[c], P.dhist_out[c]);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)up_tiles(n_total), (unsigned)nc);
    int rc = SRCDSP_OK;
    const bool served = up_dot2_dispatch<UpDot2Resampler>(u0.L, PP, [&](auto lr, auto ppc) {
        constexpr int LR = decltype(lr)::value;
        auto kern = resample_tile_dot2<LR, decltype(ppc)::value>;
        // beyond the default limit of dynamic LDS: the kernel's largest launch, so once per kernel
        rc = raise_lds_limit((const void *)kern, rs_smem(kUpMaxTaps / LR, LR, kRsMaxDecimTaps));
        if (!rc) hipLaunchKernelGGL(kern, grid, dim3(kUpBlockD), smem, s, P);
    });
    if (!rc) rc = up_dot2_launched(served);
    if (rc) return rc;
    for (int c = 0; c < nc; ++c) {
        rc = chan_commit(ups[c]->u, s);
        if (!rc) rc = chan_commit(decims[c]->core, s);
        if (rc) return rc;
    }
    return SRCDSP_OK;
}

// The two reference calls as two launches through the interpolator handle's
// grow-only scratch.  The interpolator's ordering event is recorded again after
// the DECIMATOR launch (the scratch's reader), so the next write into the
// scratch -- from whichever decimator and stream the interpolator feeds next --
// waits for the last read of it.
int pair_launch(srcdsp_up_t up, srcdsp_decim_t decim, const void *d_in, size_t n_in, void *d_out, size_t n_out,
                size_t n_mid, bool flush, hipStream_t s) {
    srcdsp_up_state &u = up->u;
    if (u.mid.cap < 4 * n_mid) {  // grow: only after every earlier use is done
        int rc = u.order.sync();
        if (!rc) rc = decim->core.order.sync();
        if (rc) return rc;
        SRCDSP_HIP_TRY(hipStreamSynchronize(s));
        rc = u.mid.reserve(4 * n_mid);
        if (rc) return rc;
    }
    int rc = srcdsp_up_step(up, d_in, n_in, u.mid.d, n_mid, flush, 0, s);
    if (rc == SRCDSP_OK) rc = srcdsp_decim_step(decim, u.mid.d, n_mid, d_out, n_out, s);
    if (rc == SRCDSP_OK) rc = u.order.after(s);  // scratch released after its reader
    return rc;
}

// variants that chain: complex<int16_t> out of the interpolator, into the decimator
int check_types(const srcdsp_up_state &u, const FirCore &f, const char *who) {
    if (u.variant == UV_I16_I32) {
        set_error(std::string(who) + ": a real int16_t interpolator cannot feed the decimator (complex<int16_t> input)");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    if (f.kv != KV_CI16_I32 && f.kv != KV_CI16_I16) {
        set_error(std::string(who) + ": the decimator must take complex<int16_t> input (variant 1 or 2)");
        return SRCDSP_ERR_UNSUPPORTED;
    }
    return SRCDSP_OK;
}

// n_mid = L (n_in + length/L when flushing) must be a whole number of outputs
int check_sizes(const srcdsp_up_state &u, const FirCore &f, size_t n_in, bool flush, size_t *n_mid, size_t *n_out,
                const char *who) {
    const size_t extra = flush ? u.length / u.L : 0;
    *n_mid = (size_t)u.L * (n_in + extra);
    if (*n_mid % f.M) {
        set_error(std::string(who) + ": L*(n_in + length/L when flushing) must be a multiple of M "
                                     "(dnsampling_filters.h:133)");
        return SRCDSP_ERR_SIZE;
    }
    *n_out = *n_mid / f.M;
    return SRCDSP_OK;
}

// one checked chain; *fused tells which route served it
int resample_one(srcdsp_up_t up, srcdsp_decim_t decim, const void *d_in, size_t n_in, void *d_out, size_t n_out,
                 size_t n_mid, bool flush, hipStream_t s, bool *fused) {
    const long n_total = (long)(n_mid / up->u.L);
    *fused = fused_serves(up->u, decim->core, d_in, d_out, n_total, 1);
    if (*fused) return fused_launch(&up, &decim, 1, d_in, 0, d_out, 0, n_in, n_total, (long)n_out, s);
    return pair_launch(up, decim, d_in, n_in, d_out, n_out, n_mid, flush, s);
}
}  // namespace
}  // namespace srcdsp

using namespace srcdsp;

extern "C" {

SRCDSP_API int srcdsp_resample_step(srcdsp_up_t up, srcdsp_decim_t decim, const void *d_in, size_t n_in, void *d_out,
                                    size_t n_out, int flush, void *stream) {
    const char *who = "resample_step";
    SRCDSP_ARG_CHECK(up != nullptr && decim != nullptr, "resample_step: null handle");
    int rc = check_types(up->u, decim->core, who);
    if (rc) return rc;
    size_t n_mid = 0, want = 0;
    rc = check_sizes(up->u, decim->core, n_in, flush != 0, &n_mid, &want, who);
    if (rc) return rc;
    if (n_out != want) {
        set_error("resample_step: output must hold exactly L*n_in/M samples (L*(n_in + length/L)/M when flushing)");
        return SRCDSP_ERR_SIZE;
    }
    if (n_mid == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_in || n_in == 0), "resample_step: null buffer");
    bool fused = false;
    rc = resample_one(up, decim, d_in, n_in, d_out, n_out, n_mid, flush != 0, (hipStream_t)stream, &fused);
    if (rc == SRCDSP_OK) (fused ? g_fused_calls : g_pair_calls).hit();
    return rc;
}

SRCDSP_API int srcdsp_resample_step_batched(const srcdsp_up_t *ups, const srcdsp_decim_t *decims, int channels,
                                            const void *d_in, size_t in_stride, void *d_out, size_t out_stride,
                                            size_t n_in, int flush, void *stream) {
    const char *who = "resample_step_batched";
    SRCDSP_ARG_CHECK(ups != nullptr && decims != nullptr && channels >= 1, "resample_step_batched: no handles");
    int rc = check_handles(ups, channels, who);
    if (!rc) rc = check_handles(decims, channels, who);
    if (rc) return rc;
    const srcdsp_up_state &u0 = ups[0]->u;
    const FirCore &f0 = decims[0]->core;
    rc = check_types(u0, f0, who);
    if (rc) return rc;
    for (int c = 1; c < channels; ++c) {
        const srcdsp_up_state &uc = ups[c]->u;
        const FirCore &fc = decims[c]->core;
        SRCDSP_ARG_CHECK(uc.variant == u0.variant && uc.L == u0.L && uc.h_raw == u0.h_raw,
                         "resample_step_batched: interpolators must share variant, L and taps");
        SRCDSP_ARG_CHECK(fc.kv == f0.kv && fc.M == f0.M && fc.ntaps == f0.ntaps && fc.flags == f0.flags &&
                             fc.shift() == f0.shift() && fc.h_coef == f0.h_coef,
                         "resample_step_batched: decimators must share variant, M, taps, flags and shift");
    }
    size_t n_mid = 0, n_out = 0;
    rc = check_sizes(u0, f0, n_in, flush != 0, &n_mid, &n_out, who);
    if (rc) return rc;
    SRCDSP_ARG_CHECK(in_stride >= n_in, "resample_step_batched: in_stride must be >= n_in (one input row per channel)");
    if (out_stride < n_out) {
        set_error("resample_step_batched: out_stride must hold a row of L*(n_in + length/L when flushing)/M samples");
        return SRCDSP_ERR_SIZE;
    }
    if (n_mid == 0) return SRCDSP_OK;
    SRCDSP_ARG_CHECK(d_out && (d_in || n_in == 0), "resample_step_batched: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const long n_total = (long)(n_mid / u0.L);
    if (!(fused_serves(u0, f0, d_in, d_out, n_total, channels) && (in_stride * 4) % 16 == 0 && (out_stride * 4) % 16 == 0)) {
        g_loop_calls.hit();
        for (int c = 0; c < channels && !rc; ++c) {
            bool fused;
            rc = resample_one(ups[c], decims[c], chan_row(d_in, c, in_stride), n_in, chan_row(d_out, c, out_stride),
                              n_out, n_mid, flush != 0, s, &fused);
        }
        return rc;
    }
    g_bank_calls.hit();
    for (int c0 = 0; c0 < channels && !rc; c0 += kMaxBatch)
        rc = fused_launch(ups + c0, decims + c0, std::min(kMaxBatch, channels - c0), chan_row(d_in, c0, in_stride),
                          in_stride, chan_row(d_out, c0, out_stride), out_stride, n_in, n_total, (long)n_out, s);
    return rc;
}

SRCDSP_API int srcdsp_resample_stats(unsigned long *fused_calls, unsigned long *pair_calls, unsigned long *bank_calls,
                                     unsigned long *loop_calls) {
    g_fused_calls.read(fused_calls);
    g_pair_calls.read(pair_calls);
    g_bank_calls.read(bank_calls);
    g_loop_calls.read(loop_calls);
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_resample_geometry(int *tile_inputs, int *max_decim_taps) {
    if (tile_inputs) *tile_inputs = kRsTile;
    if (max_decim_taps) *max_decim_taps = kRsMaxDecimTaps;
    return SRCDSP_OK;
}

SRCDSP_API int srcdsp_resample_set_min_tiles(long min_tiles) {
    SRCDSP_ARG_CHECK(min_tiles >= 0, "resample_set_min_tiles: min_tiles is >= 1, or 0 for the measured routing");
    g_min_tiles.store(min_tiles, std::memory_order_relaxed);
    return SRCDSP_OK;
}

}  // extern "C"
