/*
 * srcdsp_hip.h -- C ABI of libsrcdsp_hip.so, the MI355X (gfx950) implementation
 * of SrcDsp's sample-buffer hot path.
 *
 * Every entry point replaces one member function of a SrcDsp operator class;
 * the reference interface is cited next to each declaration as
 * <file>:<line> of the upstream tree (dogjin/SrcDsp).  Plain pointers and sizes
 * only: no C++ or framework types cross this boundary.  A `stream` argument is a
 * hipStream_t passed as void* (NULL = the default stream).
 *
 * Conventions shared by all operators
 *  - Handles own the operator state on the device (coefficients, history ring,
 *    NCO phase, correlator registers) exactly as the reference objects own it
 *    in member vectors; the caller owns input/output buffers.
 *  - `*_step` takes DEVICE pointers and is asynchronous on `stream`; successive
 *    calls on one handle are ordered even across streams (the handle keeps an
 *    event of its last step).  `*_step_host` takes HOST pointers, stages through
 *    pinned memory and returns when the result is in `out` (PCIe-bound;
 *    drop-in convenience).
 *  - Sizes are in samples (one complex sample = one element).  Where the
 *    reference asserts (e.g. dnsampling_filters.h:133 out.size()*M==in.size())
 *    the C ABI returns SRCDSP_ERR_SIZE instead of aborting.
 *  - Sample layouts are those of std::complex<T> (interleaved re, im).
 */
#ifndef SRCDSP_HIP_H
#define SRCDSP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SRCDSP_API __attribute__((visibility("default")))
#else
#define SRCDSP_API
#endif

/* ---------------------------------------------------------------- status */
enum {
    SRCDSP_OK = 0,
    SRCDSP_ERR_ARG = -1,         /* null handle/pointer, invalid parameter           */
    SRCDSP_ERR_UNSUPPORTED = -2, /* type combination / ratio the reference cannot build */
    SRCDSP_ERR_SIZE = -3,        /* a size the reference asserts on                 */
    SRCDSP_ERR_HIP = -4,         /* HIP runtime failure (see srcdsp_last_error)     */
    SRCDSP_ERR_NOMEM = -5
};

/* ---------------------------------------------------------------- flags */
enum {
    /* Coefficient magnitude for coeffScaling (dnsampling_filters.h:92-95,
     * filters.h:92-96).  Default: the binding of a canonical TU, where
     * unqualified abs(float) resolves to ::abs(int) (coefficient truncated).
     * With this flag: fabs(), the binding seen when <math.h> precedes the
     * header. */
    SRCDSP_FLAG_ABS_FABS = 1u << 0,
    /* Floating-point accumulation contract of the complex<float> paths.
     * Default: one fused multiply-add per tap, taps in ascending order --
     * bit-exact to the reference built with -mfma, and |d| <= 1 output LSB on
     * <= 1e-4 of outputs against the -O2 x86-64 build.  With this flag:
     * separately rounded multiply then add -- bit-exact to the -O2 build. */
    SRCDSP_FLAG_FP_STRICT = 1u << 1
};

/* ============================================================================
 * FilterDnsamplingFir<In,Out,Internal,Coef,M>   (dnsampling_filters.h:49-172,
 * dsptl_dnsampling_filters.h:47-220)
 * variant: 0 <complex<float>, complex<float>, complex<float>, float>
 *          1 <complex<int16_t>, complex<int16_t>, complex<int32_t>, int32_t>
 *          2 <complex<int16_t>, complex<int16_t>, complex<int32_t>, int16_t>
 *          3 <complex<int32_t>, complex<int16_t>, complex<int32_t>, int32_t>
 * coeffs points to ntaps values of the Coef type.
 * ==========================================================================*/
typedef struct srcdsp_decim *srcdsp_decim_t;

/* ctor FilterDnsamplingFir(const vector<Coef>&)  dnsampling_filters.h:84-97 */
SRCDSP_API int srcdsp_decim_create(srcdsp_decim_t *out, int variant, unsigned M, const void *coeffs,
                                   int ntaps, unsigned flags);
SRCDSP_API int srcdsp_decim_destroy(srcdsp_decim_t h);
/* copy construction / assignment (the reference class is a value type: its
 * implicit copy ctor copies coefficients, history and shifts,
 * dnsampling_filters.h:47-79): *out = a new handle with h's coefficients,
 * coeffScaling, leftShift and CURRENT history (after h's pending steps) */
SRCDSP_API int srcdsp_decim_clone(srcdsp_decim_t h, srcdsp_decim_t *out);
/* setCoeffs  dsptl_dnsampling_filters.h:114-134 (history resized, not cleared;
 * require_multiple != 0 reproduces its assert(N % M == 0) as SRCDSP_ERR_SIZE) */
SRCDSP_API int srcdsp_decim_set_coeffs(srcdsp_decim_t h, const void *coeffs, int ntaps,
                                       int require_multiple);
/* setLeftShiftBy2  dnsampling_filters.h:63 */
SRCDSP_API int srcdsp_decim_set_left_shift(srcdsp_decim_t h, int left_shift);
/* reset  dnsampling_filters.h:56-60 */
SRCDSP_API int srcdsp_decim_reset(srcdsp_decim_t h);
/* step  dnsampling_filters.h:129-172 ; requires n_out * M == n_in */
SRCDSP_API int srcdsp_decim_step(srcdsp_decim_t h, const void *d_in, size_t n_in, void *d_out,
                                 size_t n_out, void *stream);
SRCDSP_API int srcdsp_decim_step_host(srcdsp_decim_t h, const void *in, size_t n_in, void *out,
                                      size_t n_out);
/* C channels of one configuration in one launch (grid.y = channel).  Channel c
 * reads d_in + c*in_stride samples and writes d_out + c*out_stride samples;
 * each handle keeps its own history.  All handles must share variant, M, taps;
 * every handle is non-null and listed once (SRCDSP_ERR_ARG otherwise, before
 * anything is enqueued: a refused call changes no handle). */
SRCDSP_API int srcdsp_decim_step_batched(const srcdsp_decim_t *hs, int channels, const void *d_in,
                                         size_t in_stride, void *d_out, size_t out_stride,
                                         size_t n_in, void *stream);
/* state introspection (tests, checkpointing): coeffScaling as stored by the
 * reference (unsigned), leftShift, and the N-1 history samples (host copy). */
SRCDSP_API int srcdsp_decim_get_state(srcdsp_decim_t h, unsigned *coeff_scaling, int *left_shift,
                                      void *history_host);

/* ============================================================================
 * FilterFir<In,Out,Internal,Coef>   (filters.h:42-169, global namespace)
 * variant: 0 <complex<float>, complex<float>, complex<float>, float>
 *          1 <float, complex<float>, float, float>
 *          2 <complex<int16_t>, complex<int16_t>, complex<int32_t>, int32_t>
 * ==========================================================================*/
typedef struct srcdsp_fir *srcdsp_fir_t;
/* ctor / setCoeffs  filters.h:74-97 */
SRCDSP_API int srcdsp_fir_create(srcdsp_fir_t *out, int variant, const void *coeffs, int ntaps,
                                 unsigned flags);
SRCDSP_API int srcdsp_fir_destroy(srcdsp_fir_t h);
/* implicit copy of FilterFir (filters.h:42-70): coefficients, shift, history */
SRCDSP_API int srcdsp_fir_clone(srcdsp_fir_t h, srcdsp_fir_t *out);
SRCDSP_API int srcdsp_fir_set_coeffs(srcdsp_fir_t h, const void *coeffs, int ntaps);
/* reset  filters.h:107-113 */
SRCDSP_API int srcdsp_fir_reset(srcdsp_fir_t h);
/* step  filters.h:131-169 ; requires n_in == n_out */
SRCDSP_API int srcdsp_fir_step(srcdsp_fir_t h, const void *d_in, size_t n_in, void *d_out, size_t n_out,
                               void *stream);
SRCDSP_API int srcdsp_fir_step_host(srcdsp_fir_t h, const void *in, size_t n_in, void *out,
                                    size_t n_out);

/* ============================================================================
 * FilterUpsamplingFir<In,Out,Internal,Coef,L>   (upsampling_filters.h:36-326)
 * variant: 0 <complex<int16_t>, complex<int16_t>, complex<int32_t>, int32_t>
 *          1 <complex<int16_t>, complex<int16_t>, complex<int32_t>, int16_t>
 *          2 <int16_t, int16_t, int32_t, int32_t>
 * ==========================================================================*/
typedef struct srcdsp_up *srcdsp_up_t;
/* ctor / setCoefficients  upsampling_filters.h:86-126 (ntaps % L == 0) */
SRCDSP_API int srcdsp_up_create(srcdsp_up_t *out, int variant, unsigned L, const void *coeffs, int ntaps);
SRCDSP_API int srcdsp_up_destroy(srcdsp_up_t h);
/* implicit copy of FilterUpsamplingFir (upsampling_filters.h:36-87): taps,
 * length, shift and the current history ring */
SRCDSP_API int srcdsp_up_clone(srcdsp_up_t h, srcdsp_up_t *out);
SRCDSP_API int srcdsp_up_set_coeffs(srcdsp_up_t h, const void *coeffs, int ntaps);
/* reset  upsampling_filters.h:50-55 */
SRCDSP_API int srcdsp_up_reset(srcdsp_up_t h);
/* getLength / getImpLength / getUpsamplingRatio  upsampling_filters.h:57-67 */
SRCDSP_API int srcdsp_up_get_length(srcdsp_up_t h, int *length, int *imp_length, int *ratio);
/* step(vector, flush)  upsampling_filters.h:149-233 (iterator=0) and
 * step(iterator, flush)  :240-323 (iterator=1: output shift 0).
 * n_out must be L*n_in, or L*(n_in + length/L) when flush. */
SRCDSP_API int srcdsp_up_step(srcdsp_up_t h, const void *d_in, size_t n_in, void *d_out, size_t n_out,
                              int flush, int iterator, void *stream);
SRCDSP_API int srcdsp_up_step_host(srcdsp_up_t h, const void *in, size_t n_in, void *out, size_t n_out,
                                   int flush, int iterator);

/* ============================================================================
 * Mixer<complex<int16_t>, complex<int16_t>, int16_t, N>   (mixers.h:27-188)
 * ==========================================================================*/
typedef struct srcdsp_mixer *srcdsp_mixer_t;
/* ctor  mixers.h:149-159 (LUT of N points), _Mixer() phi = freq = 0 */
SRCDSP_API int srcdsp_mixer_create(srcdsp_mixer_t *out, unsigned N);
SRCDSP_API int srcdsp_mixer_destroy(srcdsp_mixer_t h);
/* implicit copy of Mixer (mixers.h:27-48, 134-160): table, phi, freq, nominal */
SRCDSP_API int srcdsp_mixer_clone(srcdsp_mixer_t h, srcdsp_mixer_t *out);
/* setFrequency / reset / adjustFrequency  mixers.h:51-98 */
SRCDSP_API int srcdsp_mixer_set_frequency(srcdsp_mixer_t h, float lo_freq);
SRCDSP_API int srcdsp_mixer_reset(srcdsp_mixer_t h, float lo_freq);
SRCDSP_API int srcdsp_mixer_adjust_frequency(srcdsp_mixer_t h, float adjust);
/* phase, frequency word, nominal frequency; and the N-entry LUT (host copy) */
SRCDSP_API int srcdsp_mixer_get_state(srcdsp_mixer_t h, int *phi, int *freq, float *nominal);
SRCDSP_API int srcdsp_mixer_get_table(srcdsp_mixer_t h, int16_t *table_host);
/* Extension (no reference call; SURVEY 8e time sharding): set the phase
 * accumulator phi (0 <= phi < N), the closed form (phi0 + k*freq) mod N of
 * mixers.h:177 at sample k, so a buffer segment starting at sample k mixes
 * exactly as the unsplit buffer. */
SRCDSP_API int srcdsp_mixer_set_phase(srcdsp_mixer_t h, int phi);
/* step  mixers.h:169-188 ; n_out == n_in */
SRCDSP_API int srcdsp_mixer_step(srcdsp_mixer_t h, const void *d_in, size_t n, void *d_out, void *stream);
SRCDSP_API int srcdsp_mixer_step_host(srcdsp_mixer_t h, const void *in, size_t n, void *out);

/* Mixer -> FilterDnsamplingFir (variant 1) fused: the two reference calls
 * mixer.step(in, tmp); decim.step(tmp, out) in one pass with no intermediate
 * buffer.  Both objects' state advances exactly as in the two calls. */
SRCDSP_API int srcdsp_mixdecim_step(srcdsp_mixer_t mixer, srcdsp_decim_t decim, const void *d_in,
                                    size_t n_in, void *d_out, size_t n_out, void *stream);
/* Extension (no reference call).  C mixer -> decimator chains in one call: for
 * every channel c exactly the two reference calls mixers[c].step(in_c, tmp);
 * decims[c].step(tmp, out_c) (mixers.h:169-188, dnsampling_filters.h:129-172),
 * in_c = d_in + c*in_stride samples, out_c = d_out + c*out_stride samples.
 * in_stride == 0: every channel reads the SAME n_in samples (one wideband
 * input, C local oscillators): the input is read once.
 * Every handle's state advances as in the per-channel calls.
 * The decimators must share variant, M, taps, flags and shift, the mixers N;
 * every handle is listed once; n_in % M == 0 (SRCDSP_ERR_ARG otherwise).
 * One kernel (the DDC bank kernel) serves variant 1 with int16-range taps,
 * M = 4, 1..1024 taps, N a power of two <= 4096, a 16-byte aligned input and
 * input row stride, n_in x taps <= 2^31 (longer calls measured faster through
 * the single-channel kernel: 8 x 2^26 samples x 127 taps 1.04 ms against
 * 0.83 ms); every other shape runs srcdsp_mixdecim_step per channel. */
SRCDSP_API int srcdsp_mixdecim_step_batched(const srcdsp_mixer_t *mixers, const srcdsp_decim_t *decims,
                                            int channels, const void *d_in, size_t in_stride,
                                            void *d_out, size_t out_stride, size_t n_in, void *stream);
/* process-wide counters: calls served by the bank kernel, calls served by the per-channel loop */
SRCDSP_API int srcdsp_mixdecim_batched_stats(unsigned long *bank_calls, unsigned long *loop_calls);

/* Extension (test and measurement hook of the persistent streaming kernels
 * behind srcdsp_decim_step, srcdsp_fir_step, srcdsp_mixdecim_step and their
 * batched forms: dnsampling_filters.h:129-172, filters.h:131-169,
 * mixers.h:169-188).  Those kernels run on min(tiles of the call, a measured
 * product grid) workgroups, each walking its share of the tiles.  cap >= 1
 * makes every such launch use min(its product grid, cap) workgroups in x, so
 * that a short call gives every workgroup several tiles; 0 puts the product
 * grids back; negative is SRCDSP_ERR_ARG.  Process-wide.  Results do not
 * depend on it; speed does. */
SRCDSP_API int srcdsp_stream_set_grid_cap(long cap);
/* Extension: the cap as last set (0: the product grids) */
SRCDSP_API long srcdsp_stream_get_grid_cap(void);
/* Extension.  Process-wide counters: launches of the persistent streaming
 * kernels, and those among them with more tiles than workgroups (some
 * workgroup walked more than one tile).  Null pointers are skipped. */
SRCDSP_API int srcdsp_stream_grid_stats(unsigned long *launches, unsigned long *looping);

/* FilterUpsamplingFir (variant 0 or 1) -> Mixer fused, the transmit chain: the
 * two reference calls up.step(in, tmp, flush) (upsampling_filters.h:149-233;
 * iterator=1: the iterator overload's shift 0, :240-323); mixer.step(tmp, out)
 * (mixers.h:169-188) in one pass with no intermediate buffer.  Every output is
 * limitScale16(limitScale<complex<int16_t>>(y, shift) * lo, 14): the
 * interpolator's asymmetric clamp to int16 (dsp_complex.h:83-108), then the
 * mixer's product and symmetric clamp (dsp_complex.cpp:31-37, 63-73).
 * n_out must be exactly L*n_in, or L*(n_in + length/L) when flush
 * (SRCDSP_ERR_SIZE otherwise; unlike srcdsp_up_step no larger buffer when
 * flushing: the mixer would step over the slack).  The mixer advances by n_out
 * samples, flushed ones included, the interpolator's history as in
 * srcdsp_up_step; a later single-operator call on either handle continues bit
 * for bit.  Variant 2 (real int16_t) cannot feed the mixer:
 * SRCDSP_ERR_UNSUPPORTED.  A refused call changes no handle.
 * One kernel serves variant 0 with int16-range taps, L = 2..8, <= 4096 taps,
 * 16-byte aligned d_in and d_out and a mixer of N <= 4096; every other shape
 * runs srcdsp_up_step into d_out and srcdsp_mixer_step in place on it. */
SRCDSP_API int srcdsp_upmix_step(srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_in, size_t n_in,
                                 void *d_out, size_t n_out, int flush, int iterator, void *stream);
/* Extension (no reference call).  C such chains in one call (vector overload):
 * channel c reads d_in + c*in_stride samples and writes the row d_out +
 * c*out_stride samples exactly as srcdsp_upmix_step(ups[c], mixers[c], ...)
 * would.  in_stride == 0: every channel reads the SAME n_in samples (one
 * baseband stream onto C carriers); otherwise in_stride >= n_in.  out_stride >=
 * L*(n_in + length/L when flush) (SRCDSP_ERR_SIZE otherwise); samples of a row
 * past that are not written.  The interpolators must share variant, L and
 * taps, the mixers N; every handle is listed once; channels >= 1
 * (SRCDSP_ERR_ARG otherwise).  One launch (grid.y = channel) serves the shapes
 * the single call's kernel serves when the row strides are multiples of 16
 * bytes too; every other shape runs the single call per channel. */
SRCDSP_API int srcdsp_upmix_step_batched(const srcdsp_up_t *ups, const srcdsp_mixer_t *mixers, int channels,
                                         const void *d_in, size_t in_stride, void *d_out, size_t out_stride,
                                         size_t n_in, int flush, void *stream);
/* process-wide counters: single calls served by the fused kernel / by the pair
 * of operators, batched calls served by one launch / by the per-channel loop */
SRCDSP_API int srcdsp_upmix_stats(unsigned long *fused_calls, unsigned long *pair_calls,
                                  unsigned long *bank_calls, unsigned long *loop_calls);

/* FilterUpsamplingFir (variant 0 or 1) -> FilterDnsamplingFir (variant 1 or 2),
 * the rational L/M rate change: the two reference calls up.step(in, tmp,
 * flush) (the vector overload, upsampling_filters.h:149-233: shift 15 -
 * round(log2 L), asymmetric clamp to int16, dsp_complex.h:83-108) and
 * decim.step(tmp, out) (dnsampling_filters.h:129-172: shift coeffScaling -
 * leftShift masked & 31, symmetric +-32767 clamp, dsp_complex.cpp:63-73) in one
 * call; the caller never allocates tmp.  With n_mid = L*(n_in + (flush ?
 * length/L : 0)): n_mid % M == 0 and n_out == n_mid / M, else SRCDSP_ERR_SIZE;
 * n_in == 0 without flush is SRCDSP_OK and changes nothing.  Both handles end
 * as the two calls leave them (the interpolator's history as srcdsp_up_step
 * writes it, the decimator's the last N_d - 1 interpolated samples of history
 * ++ call; coeffScaling and leftShift untouched), so any later
 * single-operator or fused call on either handle continues bit for bit.
 * Interpolator variant 2 (real int16_t) and decimator variants 0 and 3 cannot
 * be chained: SRCDSP_ERR_UNSUPPORTED.  Null handle: SRCDSP_ERR_ARG.  A refused
 * call changes no handle.  The iterator overload (shift 0) is not offered.
 * One kernel (resample_tile_dot2) takes interpolator variant 0 with int16-range
 * taps, L = 2..8, <= 4096 taps, decimator variant 1 with int16-range taps, M =
 * 1..8, <= 1024 taps, and 16-byte aligned d_in and d_out; of those it serves
 * the shape classes where it measured faster than the two calls (DESIGN 5.4c:
 * L/M = 4/3 and 2/3 in calls of at least 2048 tiles of 2048 inputs, rows x
 * tiles per row).
 * Every other call runs srcdsp_up_step into a grow-only scratch owned by the
 * interpolator handle and srcdsp_decim_step from it. */
SRCDSP_API int srcdsp_resample_step(srcdsp_up_t up, srcdsp_decim_t decim, const void *d_in, size_t n_in,
                                    void *d_out, size_t n_out, int flush, void *stream);
/* Extension (no reference call).  C such chains in one call: channel c reads
 * d_in + c*in_stride samples and writes the row d_out + c*out_stride samples
 * exactly as srcdsp_resample_step(ups[c], decims[c], ...) would.  in_stride >=
 * n_in (there is no shared-input form: equal filters on one input give equal
 * rows); out_stride >= n_out (SRCDSP_ERR_SIZE otherwise).  The interpolators
 * must share variant, L and taps, the decimators variant, M, taps, flags and
 * shift; every handle is listed once; channels >= 1 (SRCDSP_ERR_ARG otherwise,
 * before anything is enqueued).  One launch (grid.y = channel, 64 per launch)
 * where the single call's kernel serves and both row strides are multiples of
 * 16 bytes; otherwise the call loops the single call. */
SRCDSP_API int srcdsp_resample_step_batched(const srcdsp_up_t *ups, const srcdsp_decim_t *decims, int channels,
                                            const void *d_in, size_t in_stride, void *d_out, size_t out_stride,
                                            size_t n_in, int flush, void *stream);
/* process-wide counters: single calls served by the fused kernel / by the pair
 * of operators, batched calls served by one launch / by the per-channel loop */
SRCDSP_API int srcdsp_resample_stats(unsigned long *fused_calls, unsigned long *pair_calls,
                                     unsigned long *bank_calls, unsigned long *loop_calls);
/* the fused kernel's tile (input samples) and its decimator tap limit */
SRCDSP_API int srcdsp_resample_geometry(int *tile_inputs, int *max_decim_taps);
/* Test and measurement hook: min_tiles >= 1 sends every call the fused kernel
 * takes with at least that many tiles to it, whatever was measured; 0 restores
 * the measured routing.  Process-wide. */
SRCDSP_API int srcdsp_resample_set_min_tiles(long min_tiles);

/* ============================================================================
 * SymbolMapperSdpsk<int16_t> (modulators.h:82-131) and
 * SymbolMapperQpsk<int16_t>  (modulators.h:147-198)
 * A bit is a uint8_t and a one whenever it is non-zero (`bits[i] > 0`, :110,
 * :177).  A symbol is complex<int16_t> of amplitude 8192 (:34-39).
 * ==========================================================================*/
typedef struct srcdsp_mapper *srcdsp_mapper_t;
#define SRCDSP_MAPPER_SDPSK 0
#define SRCDSP_MAPPER_QPSK 1

/* the constructors (modulators.h:87-99, :152-165); state 0.  No device call: a
 * handle is a host object until it steps on device buffers. */
SRCDSP_API int srcdsp_mapper_create(srcdsp_mapper_t *out, int kind);
SRCDSP_API int srcdsp_mapper_destroy(srcdsp_mapper_t h);
/* the implicit copy constructor: kind and state (waits for the last step) */
SRCDSP_API int srcdsp_mapper_clone(srcdsp_mapper_t h, srcdsp_mapper_t *out);
/* reset() (modulators.h:120-123, :187-190): state 0 */
SRCDSP_API int srcdsp_mapper_reset(srcdsp_mapper_t h);
/* the private `state` member (modulators.h:127, :194); waits for the handle's
 * last step */
SRCDSP_API int srcdsp_mapper_get_state(srcdsp_mapper_t h, int *kind, int *state);
/* Extension (no reference call): set the state, 0..3, so that a bit stream can
 * be split in time (as srcdsp_mixer_set_phase does for the mixer). */
SRCDSP_API int srcdsp_mapper_set_state(srcdsp_mapper_t h, int state);
/* the bits one workgroup tile of the kernels covers */
SRCDSP_API int srcdsp_mapper_geometry(int *tile_bits);
/* step() (modulators.h:103-117 SDPSK: state = (state + (bit ? 1 : 3)) % 4 per
 * bit, out[i] = map[state], n_out == n_bits; :169-184 QPSK: state = first bit
 * << 1 | second bit per pair, n_bits == 2 n_out) on device buffers: d_bits
 * uint8_t[n_bits], d_out complex<int16_t>[n_out].  The reference's asserts on
 * the sizes (:106, :171) are SRCDSP_ERR_SIZE; n_bits == 0 changes nothing. */
SRCDSP_API int srcdsp_mapper_step(srcdsp_mapper_t h, const void *d_bits, size_t n_bits, void *d_out, size_t n_out,
                                  void *stream);
SRCDSP_API int srcdsp_mapper_step_host(srcdsp_mapper_t h, const void *bits, size_t n_bits, void *out, size_t n_out);
/* Extension (no reference call).  C mappers in one call: row c reads d_bits +
 * c*bits_stride bytes and writes d_out + c*out_stride samples exactly as
 * srcdsp_mapper_step(hs[c], ...) (modulators.h:103-117, :169-184) would.
 * bits_stride == 0: every row reads the SAME bits; otherwise bits_stride >=
 * n_bits.  out_stride >= the row's symbols (SRCDSP_ERR_SIZE otherwise, as an
 * odd QPSK n_bits).  The mappers share a kind (their states may differ), every
 * handle is listed once, channels >= 1 (SRCDSP_ERR_ARG otherwise).  A refused
 * call changes no handle. */
SRCDSP_API int srcdsp_mapper_step_batched(const srcdsp_mapper_t *hs, int channels, const void *d_bits,
                                          size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits,
                                          void *stream);

/* Mapper -> FilterUpsamplingFir (variant 0 or 1) -> Mixer, the transmit chain
 * from bits: the three reference calls mapper.step(bits, sym)
 * (modulators.h:103-117 / :169-184); up.step(sym, tmp, flush)
 * (upsampling_filters.h:149-233; iterator=1: :240-323); mixer.step(tmp, out)
 * (mixers.h:169-188) in one call.  n_out follows srcdsp_upmix_step with n_in
 * the symbol count (n_bits, or n_bits / 2 for QPSK; an odd QPSK n_bits is
 * SRCDSP_ERR_SIZE).  All three handles advance as in the three calls: the
 * interpolator's history ends holding the last symbols, the mixer advances by
 * n_out, the mapper reaches its end state; a later single-operator call on any
 * of them continues bit for bit.  A real int16_t interpolator is
 * SRCDSP_ERR_UNSUPPORTED.  A refused call changes no handle.
 * One kernel (the interpolator's tile fed from bits, the mixer in its
 * epilogue) serves what srcdsp_upmix_step's kernel serves when d_bits is
 * 16-byte aligned too; every other shape runs srcdsp_mapper_step into scratch
 * and srcdsp_upmix_step inside the call. */
SRCDSP_API int srcdsp_modulate_step(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_mixer_t mixer, const void *d_bits,
                                    size_t n_bits, void *d_out, size_t n_out, int flush, int iterator, void *stream);
/* Extension (no reference call).  C such chains in one call: row c is
 * srcdsp_modulate_step(mappers[c], ups[c], mixers[c], d_bits + c*bits_stride
 * bytes, ..., d_out + c*out_stride samples, ...) (modulators.h:103-117 /
 * :169-184, upsampling_filters.h:149-233, mixers.h:169-188).  bits_stride == 0:
 * shared bits; otherwise >= n_bits.  out_stride as srcdsp_upmix_step_batched.
 * The mappers share a kind, the interpolators variant, L and taps, the mixers
 * N; every handle is listed once (SRCDSP_ERR_ARG otherwise).  One launch
 * serves the single call's kernel shapes when the row strides are multiples
 * of 16 bytes; every other shape loops over the channels. */
SRCDSP_API int srcdsp_modulate_step_batched(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                            const srcdsp_mixer_t *mixers, int channels, const void *d_bits,
                                            size_t bits_stride, void *d_out, size_t out_stride, size_t n_bits,
                                            int flush, void *stream);
/* process-wide counters (the paths of modulators.h:103-184 ->
 * upsampling_filters.h:149-233 -> mixers.h:169-188): single calls served by
 * the fused kernel / by the mapper then srcdsp_upmix_step, batched calls
 * served by one launch / by the per-channel loop */
SRCDSP_API int srcdsp_modulate_stats(unsigned long *fused_calls, unsigned long *chain_calls,
                                     unsigned long *bank_calls, unsigned long *loop_calls);

/* ============================================================================
 * The OQPSK Q-rail stagger: an extension with no reference class.
 * SymbolMapperQpsk is "for QPSK or OQPSK modulations" (modulators.h:147-198);
 * the offset is the application's there: a delay line of half a symbol (L/2
 * output samples) on the imaginary rail between FilterUpsamplingFir::step
 * (upsampling_filters.h:149-233) and Mixer::step (mixers.h:169-188).  This is
 * that delay line.  With v = carry ++ im(in[0..n)):
 *   out[i] = (re(in[i]), v[i])     i.e. im(in[i-D]), or carry[i] for i < D
 *   carry' = v[n .. n+D)           the last D imaginary halves, also for n < D
 * ==========================================================================*/
typedef struct srcdsp_stagger *srcdsp_stagger_t;
/* Extension (between upsampling_filters.h:149-233 and mixers.h:169-188): a
 * delay of D samples, 1 <= D <= 64 (SRCDSP_ERR_ARG otherwise), carry 0.  No
 * device call: a handle is a host object until it steps on device buffers. */
SRCDSP_API int srcdsp_stagger_create(srcdsp_stagger_t *out, unsigned D);
SRCDSP_API int srcdsp_stagger_destroy(srcdsp_stagger_t h);
/* Extension: a value copy, D and the carry (waits for the last step) */
SRCDSP_API int srcdsp_stagger_clone(srcdsp_stagger_t h, srcdsp_stagger_t *out);
/* Extension: carry = 0, as a new handle */
SRCDSP_API int srcdsp_stagger_reset(srcdsp_stagger_t h);
/* Extension: D and the carry (D int16_t, carry[i] is the imaginary half of the
 * next step's out[i]); waits for the handle's last step.  Null pointers are
 * skipped. */
SRCDSP_API int srcdsp_stagger_get_state(srcdsp_stagger_t h, unsigned *D, int16_t *carry);
/* Extension: the samples one workgroup of the kernel covers, the largest D */
SRCDSP_API int srcdsp_stagger_geometry(int *tile_samples, unsigned *max_delay);
/* Extension (the delay between up.step, upsampling_filters.h:149-233, and
 * mixer.step, mixers.h:169-188): one step on device buffers of n
 * complex<int16_t> each.  d_in and d_out may not overlap (SRCDSP_ERR_ARG): a
 * sample is read again D samples later.  n == 0 changes nothing.  A refused
 * call changes no handle. */
SRCDSP_API int srcdsp_stagger_step(srcdsp_stagger_t h, const void *d_in, size_t n, void *d_out, void *stream);
SRCDSP_API int srcdsp_stagger_step_host(srcdsp_stagger_t h, const void *in, size_t n, void *out);
/* Extension.  C staggers in one call: row c reads d_in + c*in_stride samples
 * and writes d_out + c*out_stride samples exactly as srcdsp_stagger_step(hs[c],
 * ...) would.  in_stride == 0: every row reads the SAME samples; otherwise
 * in_stride >= n.  out_stride >= n (SRCDSP_ERR_SIZE otherwise).  The staggers
 * share D (their carries may differ), every handle is listed once, channels >=
 * 1, and the two arrays do not overlap (SRCDSP_ERR_ARG otherwise). */
SRCDSP_API int srcdsp_stagger_step_batched(const srcdsp_stagger_t *hs, int channels, const void *d_in,
                                           size_t in_stride, void *d_out, size_t out_stride, size_t n, void *stream);

/* Extension.  Mapper -> FilterUpsamplingFir -> stagger -> Mixer, the offset-QPSK
 * transmit chain from bits: mapper.step(bits, sym) (modulators.h:103-117 /
 * :169-184); up.step(sym, tmp, flush) (upsampling_filters.h:149-233;
 * iterator=1: :240-323); srcdsp_stagger_step(tmp, tmp2); mixer.step(tmp2, out)
 * (mixers.h:169-188) in one call.  Sizes and refusals as srcdsp_modulate_step;
 * any mapper kind.  All four handles end as the four calls leave them, bit for
 * bit: the carry holds the last D imaginary outputs after the interpolator's
 * clamp and before the mixer.
 * One kernel (srcdsp_modulate_step's, the delay between the interpolator's
 * clamp and the mixer epilogue) serves what that call's kernel serves with
 * D <= L; every other shape runs the four operators inside the call. */
SRCDSP_API int srcdsp_modulate_offset_step(srcdsp_mapper_t mapper, srcdsp_up_t up, srcdsp_stagger_t stagger,
                                           srcdsp_mixer_t mixer, const void *d_bits, size_t n_bits, void *d_out,
                                           size_t n_out, int flush, int iterator, void *stream);
/* Extension.  C such chains in one call: row c is
 * srcdsp_modulate_offset_step(mappers[c], ups[c], staggers[c], mixers[c], ...)
 * (modulators.h:103-117 / :169-184, upsampling_filters.h:149-233,
 * mixers.h:169-188), rows and strides as srcdsp_modulate_step_batched.  The
 * staggers share D as the mappers share a kind; every handle is listed once
 * (SRCDSP_ERR_ARG otherwise).  One launch (grid.y = channel) serves the single
 * call's kernel shapes when the row strides are multiples of 16 bytes; every
 * other shape loops over the channels. */
SRCDSP_API int srcdsp_modulate_offset_step_batched(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                                   const srcdsp_stagger_t *staggers, const srcdsp_mixer_t *mixers,
                                                   int channels, const void *d_bits, size_t bits_stride, void *d_out,
                                                   size_t out_stride, size_t n_bits, int flush, void *stream);
/* Extension.  Process-wide counters (the paths of modulators.h:103-184 ->
 * upsampling_filters.h:149-233 -> stagger -> mixers.h:169-188): single calls
 * served by the fused kernel / by the four operators, batched calls served by
 * one launch / by the per-channel loop */
SRCDSP_API int srcdsp_modulate_offset_stats(unsigned long *fused_calls, unsigned long *chain_calls,
                                            unsigned long *bank_calls, unsigned long *loop_calls);

/* ============================================================================
 * The carrier combiner: an extension with no reference call.  C carriers, each
 * a row of complex<int16_t> as Mixer::step leaves it (mixers.h:169-188), onto
 * one wire:
 *   out[i] = limitScale<complex<int16_t>, complex<int32_t>>(
 *                sum_{c < rows} in_c[i], shift)            (dsp_complex.h:83-108)
 *   in_c = d_in + c*in_stride samples,  i < n
 * The sum is exact in int32, then the arithmetic shift right by `shift` and the
 * clamp to [-32768, 32767], each per component.  rows == 1 is limitScale(x,
 * shift).
 * ==========================================================================*/
/* Extension (dsp_complex.h:83-108 over a sum of rows).  Stateless: no handle.
 * rows is 1..65535 (rows * 32768 fits int32), shift 0..15, and neither buffer
 * is null unless n == 0 (SRCDSP_ERR_ARG otherwise, before any HIP call).  n ==
 * 0 does nothing.  in_stride == 0 sums the same row `rows` times.  Offsets are
 * 64-bit: no INT_MAX limit on n or in_stride.  d_out may be row 0 itself (as
 * the mixer runs in place); any other overlap of d_out with the rows is the
 * caller's error and is not detected.  Rows whose base and stride are
 * multiples of 16 bytes are read 16 bytes per lane; others sample by sample. */
SRCDSP_API int srcdsp_combine_step(const void *d_in, size_t in_stride, size_t rows, void *d_out, size_t n,
                                   unsigned shift, void *stream);
/* Extension: the same on host buffers, with the kernel's own arithmetic on the
 * host; no HIP call. */
SRCDSP_API int srcdsp_combine_step_host(const void *in, size_t in_stride, size_t rows, void *out, size_t n,
                                        unsigned shift);

/* Extension.  C transmit chains from bits summed onto ONE wire in one call.
 * d_out is one row of n_out complex<int16_t> and holds exactly what
 *   srcdsp_modulate_offset_step_batched(mappers, ups, staggers, mixers, ...)
 *     into C private rows (modulators.h:103-117 / :169-184,
 *     upsampling_filters.h:149-233, the stagger, mixers.h:169-188; staggers ==
 *     NULL: srcdsp_modulate_step_batched, the chains without a stagger), then
 *   srcdsp_combine_step(rows, stride, channels, d_out, n_out, shift, stream)
 *     (dsp_complex.h:83-108)
 * would leave, without the [C, n_out] rows.  Every handle (mapper state,
 * interpolator history, stagger carry, mixer phase) ends as the bank call
 * leaves it, bit for bit.
 * The bank's size and sharing rules apply (shared kind, variant, L, taps, D and
 * N; every handle listed once; bits_stride 0 or >= n_bits; an odd QPSK n_bits
 * is SRCDSP_ERR_SIZE).  n_out equals the bank's row length, L*(symbols +
 * length/L when flushing), exactly (SRCDSP_ERR_SIZE otherwise); shift is 0..15
 * and channels >= 1 (SRCDSP_ERR_ARG otherwise).  A refused call changes no
 * handle; n_out == 0 does nothing.
 * One kernel, a workgroup per tile of 2048 symbols looping over the chains with
 * the sums in registers, exists for L = 2, 4 and 8 where the bank's one launch
 * would serve the chains (variant 0 with int16-range taps, N <= 4096, D <= L,
 * at L = 8 D = 4, d_bits 16-byte aligned, bits_stride a multiple of 16 bytes),
 * with at most 64 chains and d_out 16-byte aligned.  It is routed by
 * measurement (srcdsp_modulate_sum_geometry): as measured it serves L = 2 from
 * 2048 tiles on with at most 8 chains, and no call at L = 4 or L = 8, where it
 * did not beat the bank and the combiner at any length.  Every other call
 * (those, L = 3, 5, 6 and 7, which have no kernel, more than 64 chains, D > L,
 * int16-tap interpolators, unaligned bits, short rows) runs the bank into
 * grow-only rows on the lead mapper and the combiner inside the call. */
SRCDSP_API int srcdsp_modulate_sum_step(const srcdsp_mapper_t *mappers, const srcdsp_up_t *ups,
                                        const srcdsp_stagger_t *staggers, const srcdsp_mixer_t *mixers, int channels,
                                        const void *d_bits, size_t bits_stride, void *d_out, size_t n_out,
                                        size_t n_bits, int flush, unsigned shift, void *stream);
/* Extension.  Process-wide counters (the paths of modulators.h:103-184 ->
 * upsampling_filters.h:149-233 -> stagger -> mixers.h:169-188 ->
 * dsp_complex.h:83-108): calls served by the fused kernel / by the bank and the
 * combiner */
SRCDSP_API int srcdsp_modulate_sum_stats(unsigned long *fused_calls, unsigned long *bank_calls);
/* Extension (routing of the sum behind mixers.h:169-188): the symbols one
 * workgroup of the fused kernel covers, and the calls it serves of those it
 * takes at interpolation by L: at least min_tiles tiles (0: none) and at most
 * max_channels chains.  Null pointers are skipped. */
SRCDSP_API int srcdsp_modulate_sum_geometry(unsigned L, int *tile_symbols, long *min_tiles, int *max_channels);
/* Extension (routing of the sum behind mixers.h:169-188): min_tiles >= 1 routes
 * every call the fused kernel takes (L = 2, 4 and 8, up to 64 chains) to it from
 * that many tiles on, process-wide (tests, measurements); 0 puts the measured
 * routing back; negative is SRCDSP_ERR_ARG.  Results do not depend on it. */
SRCDSP_API int srcdsp_modulate_sum_set_min_tiles(long min_tiles);

/* ============================================================================
 * FixedPatternCorrelator<int16_t, int32_t, N, S>   (correlators.h:54-316)
 * ==========================================================================*/
typedef struct srcdsp_corr *srcdsp_corr_t;
/* ctor  correlators.h:119-132 */
SRCDSP_API int srcdsp_corr_create(srcdsp_corr_t *out, unsigned N, unsigned S);
SRCDSP_API int srcdsp_corr_destroy(srcdsp_corr_t h);
/* implicit copy of FixedPatternCorrelator (correlators.h:54-118): pattern,
 * thresholds, history ring, the three corr/energy registers, bitSamples */
SRCDSP_API int srcdsp_corr_clone(srcdsp_corr_t h, srcdsp_corr_t *out);
/* setPattern(array<complex<int32_t>,N>, thresholdCoeff)  correlators.h:167-194;
 * pattern = N complex<int32_t> (2N int32).  The reference's
 * assert(energy <= 1073217600) is returned as SRCDSP_ERR_ARG. */
SRCDSP_API int srcdsp_corr_set_pattern(srcdsp_corr_t h, const int32_t *pattern, double threshold_coeff);
/* reset  correlators.h:146-159 */
SRCDSP_API int srcdsp_corr_reset(srcdsp_corr_t h);
/* step(in, corrIndex) -> bool  correlators.h:209-303.  *found = 0/1,
 * *corr_index written only when found (as the reference).  Synchronous: the
 * answer is needed on the host. */
SRCDSP_API int srcdsp_corr_step(srcdsp_corr_t h, const void *d_in, size_t n, int *found, int *corr_index,
                                void *stream);
SRCDSP_API int srcdsp_corr_step_host(srcdsp_corr_t h, const void *in, size_t n, int *found,
                                     int *corr_index);
/* Extension (no reference call; SURVEY 8e time sharding): the state step()
 * leaves after streaming these n samples with NO detection test
 * (correlators.h:221-250 without :262-291): history ring and the
 * energy/correlation registers.  Seeds a time segment with its halo. */
SRCDSP_API int srcdsp_corr_prime(srcdsp_corr_t h, const void *d_in, size_t n, void *stream);
/* Extension (no reference call).  C correlators stepped in one call: for every
 * channel c exactly hs[c].step(in_c, corrIndex_c) (correlators.h:209-303),
 * in_c = d_in + c*in_stride samples of complex<int16_t>, n samples each.
 * in_stride == 0: every channel scans the SAME n samples (several sync words
 * searched in one stream).  found[c] = 0/1 and corr_index[c] (written only
 * when found) are host arrays of `channels` entries.  Channels are
 * independent: each scans up to its own first detection.  Every handle is left
 * as srcdsp_corr_step leaves it (registers, history, bitSamples, stream
 * ordering).  Synchronous, with at most two host synchronisations per call
 * whatever `channels` is.
 * The handles must share N and S (patterns and scalings may differ) and be
 * listed once each; channels >= 1 (SRCDSP_ERR_ARG otherwise).  n == 0 is OK
 * with every found[c] = 0; n > INT_MAX is SRCDSP_ERR_SIZE.  A refused call
 * changes no handle.
 * One bank kernel serves S == 1 with int16-range patterns and N <= 8192 (the
 * shapes of the fused single-channel scan); every other shape runs
 * srcdsp_corr_step per channel inside the call. */
SRCDSP_API int srcdsp_corr_step_batched(const srcdsp_corr_t *hs, int channels, const void *d_in, size_t in_stride,
                                        size_t n, int *found, int *corr_index, void *stream);
/* process-wide counters: calls served by the bank kernel, calls served by the per-channel loop */
SRCDSP_API int srcdsp_corr_batched_stats(unsigned long *bank_calls, unsigned long *loop_calls);
/* Extension (no reference call).  Every detection of a stream in one call:
 * per channel exactly the application's loop of step() on the remainders
 * (correlators.h:209-303 called again after each `break`, :291),
 *
 *     off = 0; k = 0
 *     while off < n and k < max_hits:
 *         found, ci = h.step(in[off:n])
 *         if not found: off = n; break
 *         corr_index[k] = off + ci; bits[k] = h.getRefBitSamples()   (:311-316)
 *         k += 1; off += ci + 2
 *     n_hits = k; consumed = off
 *
 * and nothing else.  corr_index is relative to this call's input; it can be
 * off - 1, and -1 when the peak was the previous call's last sample.  step
 * breaks before `top` advances (:291-296), so the detected sample is
 * overwritten by the next one: the loop scans the stream with every detected
 * sample removed, and so does this call.  bits_host, [max_hits][N]
 * complex<int16_t>, receives the bitSamples of each detection and may be NULL.
 * The handle is left exactly as the loop leaves it: registers, history,
 * bitSamples of the last detection, stream ordering.  consumed < n only when
 * max_hits was reached; calling again on d_in + consumed continues the loop.
 * Synchronous, with at most two host synchronisations per call whatever
 * `channels` and the number of detections are (the loop path below makes those
 * of its srcdsp_corr_step calls).  Scratch, owned by hs[0], grows with
 * channels * min(max_hits, n / 2 + 1) * N samples.
 * The batched form follows srcdsp_corr_step_batched: handles sharing N and S,
 * listed once each, any number of them; in_stride == 0 is one shared input;
 * n_hits[C], consumed[C], corr_index[C][max_hits] and bits_host[C][max_hits][N]
 * are host arrays.  n == 0 is OK with every n_hits[c] = 0; n > INT_MAX is
 * SRCDSP_ERR_SIZE; max_hits < 1, channels < 1 or a null result array is
 * SRCDSP_ERR_ARG.  A refused call changes no handle.
 * Kernels serve S == 1 with int16-range patterns and N <= 8192 (the shapes of
 * the fused scan): a candidate pass over the undisturbed stream and a resolve
 * pass that recomputes the stretch after each accepted detection on the stream
 * with the detected samples removed.  Every other shape runs the loop above
 * with srcdsp_corr_step inside the call. */
SRCDSP_API int srcdsp_corr_step_all(srcdsp_corr_t h, const void *d_in, size_t n, int max_hits, int *n_hits,
                                    int *corr_index, int16_t *bits_host, size_t *consumed, void *stream);
/* the same on a host buffer, staged through the handle's pinned buffer */
SRCDSP_API int srcdsp_corr_step_all_host(srcdsp_corr_t h, const void *in, size_t n, int max_hits, int *n_hits,
                                         int *corr_index, int16_t *bits_host, size_t *consumed);
SRCDSP_API int srcdsp_corr_step_all_batched(const srcdsp_corr_t *hs, int channels, const void *d_in, size_t in_stride,
                                            size_t n, int max_hits, int *n_hits, int *corr_index, int16_t *bits_host,
                                            size_t *consumed, void *stream);
/* process-wide counters: calls served by the kernels, calls served by the loop of srcdsp_corr_step */
SRCDSP_API int srcdsp_corr_all_stats(unsigned long *kernel_calls, unsigned long *loop_calls);
/* step() as built with CREATE_DEBUG_FILES (correlators.h:107-132, 253-257):
 * also returns, for every sample the call processed, the registers the
 * reference writes to its debug files -- corr_out[k] = corrValue[0] and
 * energy_out[k] = energyValue[0] after input sample k (host arrays of n
 * entries; *count = corrIndex + 2 on a detection, else n).  Runs the
 * segmented kernels (they keep per-sample values); same results as step(). */
SRCDSP_API int srcdsp_corr_step_trace(srcdsp_corr_t h, const void *d_in, size_t n, int *found, int *corr_index,
                                      uint32_t *corr_out, uint32_t *energy_out, size_t *count, void *stream);
SRCDSP_API int srcdsp_corr_step_host_trace(srcdsp_corr_t h, const void *in, size_t n, int *found, int *corr_index,
                                           uint32_t *corr_out, uint32_t *energy_out, size_t *count);
/* getRefBitSamples  correlators.h:311-316 (N complex<int16_t>, host copy) */
SRCDSP_API int srcdsp_corr_get_bit_samples(srcdsp_corr_t h, int16_t *bits_host);
/* getStatus  correlators.h:90 (CorrState fields) */
SRCDSP_API int srcdsp_corr_get_status(srcdsp_corr_t h, uint32_t *energy3, uint32_t *corr3,
                                      uint32_t *coeffs_energy, int *coeff_scaling,
                                      double *threshold_factor);

/* ============================================================================
 * DemodulatorOqpsk<int16_t>   (demodulators.h:53-130, demodulators.cpp:34-308)
 * One sample per bit in, soft bits (int8) out.  The PLL makes one burst a
 * sequential recurrence; the kernel runs one burst per lane, so the single
 * step is provided for parity and state continuity (slower than a host core)
 * and the bank, srcdsp_demod_step_batched, is the form to call.
 * A handle is a host object (configuration and the 7 words of StateVar): each
 * step uploads them with the reference samples its preamble reads and takes
 * the new state back, so the set/get/reset/clone calls make no device call.
 * A step returns with `stream` synchronised (the error is needed on the host),
 * which also orders the steps of a handle across streams.
 * ==========================================================================*/
typedef struct srcdsp_demod *srcdsp_demod_t;
/* ctor  demodulators.cpp:34-58 (the two lookup tables are process-wide) */
SRCDSP_API int srcdsp_demod_create(srcdsp_demod_t *out);
SRCDSP_API int srcdsp_demod_destroy(srcdsp_demod_t h);
/* implicit copy (demodulators.h:53-130 is a value type): configuration and state */
SRCDSP_API int srcdsp_demod_clone(srcdsp_demod_t h, srcdsp_demod_t *out);
/* setSyncPattern  demodulators.h:60.  nbits = 0: no pattern; nbits = 1 is
 * refused (reset() asserts, demodulators.cpp:302), as are bits other than 0 / 1
 * (demodulators.h:94) */
SRCDSP_API int srcdsp_demod_set_sync_pattern(srcdsp_demod_t h, const int8_t *bits, int nbits);
/* setReference  demodulators.cpp:126-139 (n complex<int16_t>, host) */
SRCDSP_API int srcdsp_demod_set_reference(srcdsp_demod_t h, const int16_t *ref_host, int n);
/* setReference(corr.getRefBitSamples())  correlators.h:311-316,
 * demodulators.h:67-68: the join with the correlator, without the caller's
 * vector.  Takes the N bit samples the correlator's last detection left in its
 * handle (its step is synchronous). */
SRCDSP_API int srcdsp_demod_set_reference_corr(srcdsp_demod_t h, srcdsp_corr_t corr, void *stream);
/* setInitialFrequency  demodulators.h:64.  A word outside +-4096 (the
 * reference's phase goes negative and phaseShift asserts, :109): SRCDSP_ERR_ARG */
SRCDSP_API int srcdsp_demod_set_initial_frequency(srcdsp_demod_t h, float f);
/* setInitialPhase  demodulators.h:66 (stored only, as in the reference) */
SRCDSP_API int srcdsp_demod_set_initial_phase(srcdsp_demod_t h, float p);
/* setInputShift  demodulators.h:70; 0..15 */
SRCDSP_API int srcdsp_demod_set_input_shift(srcdsp_demod_t h, int shift);
/* reset  demodulators.cpp:293-308: StateVar cleared, the shift back to 0,
 * bit1 / bit2 from the last two sync bits */
SRCDSP_API int srcdsp_demod_reset(srcdsp_demod_t h);
/* getMeasuredFrequency  demodulators.h:72 (0 before the first step) */
SRCDSP_API int srcdsp_demod_get_measured_frequency(srcdsp_demod_t h, float *f);
/* StateVar demodulators.h:76-88, then intialFreqEst, accumulatedFrequency, rightShift */
SRCDSP_API int srcdsp_demod_get_state(srcdsp_demod_t h, unsigned *bit_cnt, int *mod2_cnt, int *phase, int *bit1,
                                      int *bit2, int *i_prev, int *q_prev, int *freq_word, int *acc_freq, int *shift);
/* sineLUT[8192] and phaseLUT[128 * 128] as the constructor builds them
 * (demodulators.cpp:39-55); host arrays, no device call */
SRCDSP_API int srcdsp_demod_get_tables(int16_t *sine8192_host, int16_t *phase16384_host);
/* step  demodulators.cpp:150-284.  d_soft has room for cap int8; *n_soft =
 * the size of the vector the reference returns (n, or n - P on the first call
 * after reset with a pattern of P bits); cap < that -> SRCDSP_ERR_SIZE.  A first
 * call with n <= P (:171 asserts) and a preamble longer than the reference
 * vector (:196 reads past Iref) -> SRCDSP_ERR_SIZE; n > INT_MAX likewise.
 * n = 0: SRCDSP_OK, nothing changes.  Synchronous like srcdsp_corr_step. */
SRCDSP_API int srcdsp_demod_step(srcdsp_demod_t h, const void *d_in, size_t n, int8_t *d_soft, size_t cap,
                                 size_t *n_soft, int32_t *error, void *stream);
SRCDSP_API int srcdsp_demod_step_host(srcdsp_demod_t h, const void *in, size_t n, int8_t *soft, size_t cap,
                                      size_t *n_soft, int32_t *error);
/* Extension (no reference call).  C demodulators in one launch: channel c does
 * exactly hs[c].step(in_c, error[c]), in_c = d_in + c*in_stride +
 * (in_offset ? in_offset[c] : 0) samples, n samples each, soft bits to
 * d_soft + c*soft_stride.  in_stride == 0: all channels read the same buffer
 * (frequency hypotheses of one burst).  in_offset, n_soft, error: host arrays
 * of `channels` entries (in_offset may be NULL).  Patterns, references, shifts,
 * frequencies and states may differ per channel.  Every handle listed once;
 * channels >= 1 (no upper limit); soft_stride >= the largest n_soft.  One
 * upload, one launch and one host synchronisation per call whatever `channels`
 * is.  A refused call changes no handle. */
SRCDSP_API int srcdsp_demod_step_batched(const srcdsp_demod_t *hs, int channels, const void *d_in, size_t in_stride,
                                         const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride,
                                         size_t *n_soft, int32_t *error, void *stream);

/* ============================================================================
 * The differential SDPSK demodulator: an extension with no reference class,
 * the receiver of SymbolMapperSdpsk (modulators.h:82-131), which advances the
 * phase by +90 degrees for a one and by -90 degrees for a zero.  A handle has
 * a lag D (the samples per symbol), a soft shift and a carry of D samples.
 * With v = carry ++ in[0..n), a = in[i] and b = v[i] (in[i-D], or carry[i] for
 * i < D):
 *   tq      = im(a)*re(b) - re(a)*im(b)      Im(a conj(b)), exact in int32
 *   soft[i] = limitScale<int8_t, int32_t>(tq, shift)     (dsp_complex.h:45-63:
 *             an arithmetic shift, then a clamp to [-128, 127])
 *   bit[i]  = tq > 0 ? 1 : 0                 what srcdsp_mapper_step was fed
 *   carry'  = v[n .. n+D)                    the last D samples, also for n < D
 * The carry is zero after create and reset, so the first D outputs are soft 0
 * and bit 0: start a burst's window D samples early and drop D outputs.  No
 * PLL, no rotation and no frequency correction: a residual offset w tilts the
 * decision by w*D out of a 90 degree margin.
 * Every refusal below comes before any HIP call and changes no handle.
 * ==========================================================================*/
typedef struct srcdsp_sdpsk *srcdsp_sdpsk_t;
/* Extension (modulators.h:82-131 received, dsp_complex.h:45-63): 1 <= D <= 64
 * and shift 0..31 (SRCDSP_ERR_ARG otherwise), carry 0.  No device call: a
 * handle is a host object until it steps on device buffers. */
SRCDSP_API int srcdsp_sdpsk_create(srcdsp_sdpsk_t *out, unsigned D, unsigned shift);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63) */
SRCDSP_API int srcdsp_sdpsk_destroy(srcdsp_sdpsk_t h);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): a value copy, D, the
 * shift and the carry (waits for the last step) */
SRCDSP_API int srcdsp_sdpsk_clone(srcdsp_sdpsk_t h, srcdsp_sdpsk_t *out);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): carry = 0, as a new
 * handle; D and the shift stay */
SRCDSP_API int srcdsp_sdpsk_reset(srcdsp_sdpsk_t h);
/* Extension (the shift of dsp_complex.h:45-63 behind modulators.h:82-131):
 * 0..31, SRCDSP_ERR_ARG otherwise; holds from the next step on */
SRCDSP_API int srcdsp_sdpsk_set_shift(srcdsp_sdpsk_t h, unsigned shift);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): D, the shift and the
 * carry (D complex<int16_t>: 2*D int16_t, carry[i] is the next step's b for
 * in[i]); waits for the handle's last step.  Null pointers are skipped. */
SRCDSP_API int srcdsp_sdpsk_get_state(srcdsp_sdpsk_t h, unsigned *D, unsigned *shift, int16_t *carry);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): the samples one
 * workgroup of the kernel covers, the largest D, and the persistent workgroups
 * of a launch: 0, the kernel is not persistent (one workgroup per tile and
 * row).  No device call; null pointers are skipped. */
SRCDSP_API int srcdsp_sdpsk_geometry(int *tile_samples, unsigned *max_lag, int *workgroups);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): one step over n
 * complex<int16_t> in device memory; n int8 to d_soft and n uint8 to d_bits.
 * Either output may be NULL, not both (SRCDSP_ERR_ARG, as for a null d_in).
 * Asynchronous on `stream`: nothing comes back to the host.  Successive steps
 * of one handle are ordered across streams.  n == 0 changes nothing.  Offsets
 * are 64-bit: no INT_MAX limit on n.  d_in at any sample offset; an output off
 * a 4-byte boundary is stored byte by byte. */
SRCDSP_API int srcdsp_sdpsk_step(srcdsp_sdpsk_t h, const void *d_in, size_t n, int8_t *d_soft, uint8_t *d_bits,
                                 void *stream);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63): the same on host
 * buffers, with the kernel's own arithmetic on the host.  No HIP call for a
 * handle that has not stepped on device buffers; one whose carry the device
 * holds takes it back first (waits for its last step). */
SRCDSP_API int srcdsp_sdpsk_step_host(srcdsp_sdpsk_t h, const void *in, size_t n, int8_t *soft, uint8_t *bits);
/* Extension (modulators.h:82-131, dsp_complex.h:45-63).  C demodulators in one
 * call: row c is exactly srcdsp_sdpsk_step(hs[c], d_in + c*in_stride +
 * (in_offset ? in_offset[c] : 0) samples, n, d_soft + c*soft_stride, d_bits +
 * c*bits_stride, stream).  in_offset is a host array of `channels` entries or
 * NULL.  in_stride == 0: every row lies in one buffer (all the hits of one
 * stream).  The handles share D and the shift (their carries may differ) and
 * every handle is listed once (SRCDSP_ERR_ARG otherwise); channels >= 1, no
 * upper limit (65535 rows per launch).  The stride of an output that is not
 * NULL is >= n (SRCDSP_ERR_SIZE otherwise).  The row table of a call lives on
 * hs[0], in a ring of 4: a bank call waits on the host for the fourth call
 * before it that the same handle led, if that one is still running. */
SRCDSP_API int srcdsp_sdpsk_step_batched(const srcdsp_sdpsk_t *hs, int channels, const void *d_in, size_t in_stride,
                                         const size_t *in_offset, size_t n, int8_t *d_soft, size_t soft_stride,
                                         uint8_t *d_bits, size_t bits_stride, void *stream);

/* ============================================================================
 * estimateFreq<int16_t, L>   (dsptl_miscellaneous.h:43-58)
 * The frequency of n complex<int16_t> samples in rad/sample from the lag-L
 * autocorrelation sum x[i] * conj(x[i+L]), i < n - L (for e^{+jwn} it returns
 * -w, as the reference does).  Every term is an int, so the sums are taken
 * exactly in 64-bit integers, in any order:
 *   sums[0], sums[1]  the exact sums of termI, termQ.  termI at
 *                     x[i] = x[i+L] = (-32768, -32768) is the two's complement
 *                     wrap, -2^31 (undefined in the reference);
 *   *freq             (float)(atan2((double)sums[1], (double)sums[0]) / L),
 *                     the atan2 on the host;
 *   *exact            1 iff (n - L) * T < 2^53, T the largest |termI| or
 *                     |termQ| of the call (|-2^31| = 2^31; from the largest
 *                     and the smallest term, which the kernel tracks): then no
 *                     partial sum of the reference's double accumulation was
 *                     rounded and *freq is the reference's float bit for bit.
 *                     With 0 it comes from the exact sums and may differ from
 *                     the reference's in the last bits.  1 when n <= L.
 * A handle holds L and the scratch of its calls, no signal state.  The calls
 * are synchronous like srcdsp_corr_step (the answer is needed on the host):
 * one copy of 4 words per row back and one synchronisation per call.  sums
 * and exact may be NULL.  n <= L (n = 0 included): SRCDSP_OK, zeros, +0.0f,
 * no device call.  n > INT_MAX: SRCDSP_ERR_SIZE.  Only InType = int16_t: the
 * float instantiation adds rounded products to a running double in order,
 * which a parallel sum cannot reproduce.
 * ==========================================================================*/
typedef struct srcdsp_freqest *srcdsp_freqest_t;
SRCDSP_API int srcdsp_freqest_create(srcdsp_freqest_t *out, int L); /* L >= 1; no device call */
SRCDSP_API int srcdsp_freqest_destroy(srcdsp_freqest_t h);
/* L, and the kernel's geometry: pairs per tile, samples per vector load, and
 * the persistent workgroups of a launch on the current device (asks the
 * device; the others make no device call).  Any pointer may be NULL. */
SRCDSP_API int srcdsp_freqest_geometry(srcdsp_freqest_t h, int *L, int *tile, int *vec, int *workgroups);
/* one row of n samples in device memory, reduced by the whole GPU */
SRCDSP_API int srcdsp_freqest_run(srcdsp_freqest_t h, const void *d_in, size_t n, float *freq, int64_t sums[2],
                                  int *exact, void *stream);
/* host input, staged through pinned memory, the same kernel */
SRCDSP_API int srcdsp_freqest_run_host(srcdsp_freqest_t h, const void *in, size_t n, float *freq, int64_t sums[2],
                                       int *exact);
/* Extension (no reference call).  `channels` rows in one launch: row c is
 * d_in + c*in_stride + (in_offset ? in_offset[c] : 0) samples, n samples each;
 * in_stride == 0: every row lies in one buffer.  freq, exact: `channels`
 * entries; sums: 2 per channel.  No pair spans two rows and no load passes the
 * end of a row. */
SRCDSP_API int srcdsp_freqest_run_batched(srcdsp_freqest_t h, int channels, const void *d_in, size_t in_stride,
                                          const size_t *in_offset, size_t n, float *freq, int64_t *sums, int *exact,
                                          void *stream);
/* Extension: the join of the correlator bank and the demodulator bank.  For
 * every channel c taken (found == NULL, or found[c] != 0):
 *   demods[c].setReference(cors[c].getRefBitSamples()), all N samples, as
 *   srcdsp_demod_set_reference_corr; est = estimateFreq<int16_t, L> over bit
 *   samples first .. N-1; setInitialFrequency(scale * est), the product in
 *   float and the word rule of srcdsp_demod_set_initial_frequency; reset();
 *   freq[c] = est (freq may be NULL).
 * first = 0 is the literal composition estimateFreq(getRefBitSamples());
 * first = 1 leaves out slot 0, which holds the detected sample and not a
 * preamble sample (correlators.h:278-288).  scale = -1 turns the estimator's
 * sign into the demodulator's.  Channels not taken are untouched and their
 * freq[c] is not written.  All or nothing: a word outside +-4096, first
 * outside 0..N-1, L < 1, a null handle of a taken channel, or a demodulator
 * taken twice -> SRCDSP_ERR_ARG and no handle changes.  The bit samples are
 * in the correlator's host-side handle, so the join makes no launch: its
 * arithmetic is the kernel's per-pair function on the host. */
SRCDSP_API int srcdsp_demod_acquire_batched(const srcdsp_demod_t *demods, const srcdsp_corr_t *cors, int channels,
                                            const int *found, int L, int first, float scale, float *freq);

/* ============================================================================
 * FifoWithTimeTrack<T, N>  (buffers.h:58-459), the ring in HBM
 * One producer thread writes, one consumer thread reads (as the reference).
 * Element type T is opaque: elem_bytes per element.
 * ==========================================================================*/
typedef struct srcdsp_fifo *srcdsp_fifo_t;
/* ctor FifoWithTimeTrack(samplingFrequency)  buffers.h:62-66 (storage(N) zeroed) */
SRCDSP_API int srcdsp_fifo_create(srcdsp_fifo_t *out, size_t elem_bytes, size_t N, double sampling_frequency);
SRCDSP_API int srcdsp_fifo_destroy(srcdsp_fifo_t h);
/* write(in, seconds, fracSeconds)  buffers.h:140-224.  Host input, staged
 * through two pinned buffers; returns before its H2D copy completes (readers
 * are ordered after it on the device).  assert(inSize < N) -> SRCDSP_ERR_SIZE. */
SRCDSP_API int srcdsp_fifo_write(srcdsp_fifo_t h, const void *in, size_t n, unsigned seconds,
                                 double frac_seconds);
/* the same for device-resident input, copied D2D on `stream` */
SRCDSP_API int srcdsp_fifo_write_device(srcdsp_fifo_t h, const void *d_in, size_t n, unsigned seconds,
                                        double frac_seconds, void *stream);
/* read(out, start) -> bool  buffers.h:282-349.  *error = the reference's return
 * value (1: range not available); *start is raised to timeStart as the
 * reference does (with its stderr warning).  Output in device memory, copied
 * on `stream`; assert(out.size() != 0) -> SRCDSP_ERR_SIZE. */
SRCDSP_API int srcdsp_fifo_read(srcdsp_fifo_t h, void *d_out, size_t n, uint64_t *start, int *error,
                                void *stream);
SRCDSP_API int srcdsp_fifo_read_host(srcdsp_fifo_t h, void *out, size_t n, uint64_t *start, int *error);
/* count()  buffers.h:377-392 ; reset()  buffers.h:245-258 (indices only) */
SRCDSP_API int srcdsp_fifo_count(srcdsp_fifo_t h, size_t *count);
SRCDSP_API int srcdsp_fifo_reset(srcdsp_fifo_t h);
/* the fields dumpInfo() prints  buffers.h:229-240 */
SRCDSP_API int srcdsp_fifo_get_state(srcdsp_fifo_t h, size_t *write_ptr, uint64_t *time_start,
                                     uint64_t *time_end, int *rollover);
/* getAbsoluteTime(timePoint, fracTimePoint)  buffers.h:413-459 */
SRCDSP_API int srcdsp_fifo_get_absolute_time(srcdsp_fifo_t h, uint64_t time_point, double frac_time_point,
                                             unsigned *seconds, double *frac_seconds);

/* ============================================================================
 * Binary I/Q captures   (dsptl_files.h:101-109 saveBinarySamples,
 * :250-262 readBinarySamples).  Interleaved I,Q components of
 * component_bytes each.  Reading returns whole samples only and replaces the
 * output (the reference's out.empty() / trailing-sample bugs fixed).
 * ==========================================================================*/
SRCDSP_API int srcdsp_iq_save(const char *path, const void *d_samples, size_t n, size_t component_bytes,
                              int append, void *stream);
SRCDSP_API int srcdsp_iq_save_host(const char *path, const void *samples, size_t n, size_t component_bytes,
                                   int append);
/* number of whole samples in the file */
SRCDSP_API int srcdsp_iq_count(const char *path, size_t component_bytes, size_t *n);
SRCDSP_API int srcdsp_iq_load(const char *path, size_t component_bytes, void *d_out, size_t cap, size_t *n,
                              void *stream);
SRCDSP_API int srcdsp_iq_load_host(const char *path, size_t component_bytes, void *out, size_t cap, size_t *n);

/* ============================================================================
 * Multi-GPU (BASELINE configs[2]): one host process drives
 * several GPUs of one node.  The reference has no multi-device code; these
 * entries shard what its users do with one FilterDnsamplingFir object per
 * channel (dnsampling_filters.h:49-172) across devices, and bring the results
 * back with RCCL over xGMI.
 *
 * srcdsp_comm_t: one RCCL communicator per device, made together in this
 * process by ncclCommInitAll (rccl.h:236), plus one non-blocking HIP stream
 * per device on which the sharded operators run.  `rank` below = index into
 * the device list.
 * RCCL is loaded at the first srcdsp_comm_create (dlopen of librccl): without
 * it that call returns SRCDSP_ERR_UNSUPPORTED, and nothing else needs RCCL.
 * A sharded operator holds a reference to its comm: srcdsp_comm_destroy may
 * come before srcdsp_decim_sharded_destroy.
 * Verified on one GPU (contiguous and strided gathers); the N > 1 paths are
 * unverified on hardware until a multi-GPU node runs them.
 * ==========================================================================*/
typedef struct srcdsp_comm *srcdsp_comm_t;
/* devs may be NULL (devices 0..ndev-1) */
SRCDSP_API int srcdsp_comm_create(srcdsp_comm_t *out, int ndev, const int *devs);
SRCDSP_API int srcdsp_comm_destroy(srcdsp_comm_t c);
/* ndev, and the HIP device id of each rank (devs may be NULL) */
SRCDSP_API int srcdsp_comm_info(srcdsp_comm_t c, int *ndev, int *devs);
/* the hipStream_t (as void*) the sharded operators use on rank's device */
SRCDSP_API int srcdsp_comm_stream(srcdsp_comm_t c, int rank, void **stream);
/* wait for every rank's stream */
SRCDSP_API int srcdsp_comm_synchronize(srcdsp_comm_t c);
/* ORDERING RULE.  The comm streams are non-blocking: they do not wait for the
 * null stream or for any stream of the caller, and the caller's streams do
 * not wait for them.  Caller work that writes a rank's d_in, or touches its
 * d_out / the gather target d_root, must run on comm stream(rank), or after
 * srcdsp_comm_synchronize, or be ordered by these two calls (no host block):
 *   srcdsp_comm_wait_stream(c, r, s):   work queued later on rank r's comm
 *       stream (steps, gathers) waits for everything queued on `s` so far;
 *   srcdsp_comm_signal_stream(c, r, s): work queued later on `s` waits for
 *       everything queued on rank r's comm stream so far.
 * `s` is a hipStream_t (as void*) on rank r's device; NULL = its null stream. */
SRCDSP_API int srcdsp_comm_wait_stream(srcdsp_comm_t c, int rank, void *stream);
SRCDSP_API int srcdsp_comm_signal_stream(srcdsp_comm_t c, int rank, void *stream);

/* `channels` independent FilterDnsamplingFir objects of one configuration
 * (same variant/M/taps/flags as srcdsp_decim_create), block-partitioned over
 * the comm's devices: rank r owns channels [first_r, first_r + count_r), the
 * first channels % ndev ranks one more.  Each channel keeps its own history
 * on its own device; a step is one batched launch per device (no collective). */
typedef struct srcdsp_decim_sharded *srcdsp_decim_sharded_t;
SRCDSP_API int srcdsp_decim_sharded_create(srcdsp_decim_sharded_t *out, srcdsp_comm_t comm, int channels,
                                           int variant, unsigned M, const void *coeffs, int ntaps,
                                           unsigned flags);
SRCDSP_API int srcdsp_decim_sharded_destroy(srcdsp_decim_sharded_t h);
SRCDSP_API int srcdsp_decim_sharded_partition(srcdsp_decim_sharded_t h, int rank, int *first_channel,
                                              int *count);
/* the per-channel handle of global channel ch (for reset / setCoeffs /
 * setLeftShiftBy2 / get_state on its own device) */
SRCDSP_API int srcdsp_decim_sharded_channel(srcdsp_decim_sharded_t h, int ch, srcdsp_decim_t *handle);
/* one step() of every channel: d_in[r] / d_out[r] are device pointers on
 * rank r's device holding its count_r channels as rows in_stride / out_stride
 * samples apart; n_in samples per channel (n_in % M == 0).  Asynchronous on
 * the comm streams (ORDERING RULE above). */
SRCDSP_API int srcdsp_decim_sharded_step(srcdsp_decim_sharded_t h, const void *const *d_in, size_t in_stride,
                                         void *const *d_out, size_t out_stride, size_t n_in);
/* reset every channel (dnsampling_filters.h:56-60), each on its own device */
SRCDSP_API int srcdsp_decim_sharded_reset(srcdsp_decim_sharded_t h);
/* host std::vector convenience (reference-style: one vector per channel):
 * in[ch] -> out[ch] for every channel, n_in samples each; each device's
 * channels staged through pinned memory by one host thread per device;
 * returns when every output is on the host. */
SRCDSP_API int srcdsp_decim_sharded_step_host(srcdsp_decim_sharded_t h, const void *const *in, void *const *out,
                                              size_t n_in);
/* result gather to one device: channel ch's n_out outputs land at
 * d_root + ch*n_out samples (d_root on rank `root`'s device, room for
 * channels*n_out samples).  ncclGather (rccl.h:745) when every rank holds the
 * same number of contiguous rows, else grouped ncclSend/ncclRecv
 * (rccl.h:700,720) with the root's own rows copied on its device.
 * Asynchronous on the comm streams (ORDERING RULE above). */
SRCDSP_API int srcdsp_decim_sharded_gather(srcdsp_decim_sharded_t h, void *const *d_out, size_t out_stride,
                                           size_t n_out, void *d_root, int root);

/* ---------------------------------------------------------------- misc */
/* Last error text of the calling thread (HIP error string or argument check). */
SRCDSP_API const char *srcdsp_last_error(void);
/* Library version "major.minor.patch" and the offload target it was built for. */
SRCDSP_API const char *srcdsp_version(void);
/* Test switches this library was built with, read back from a kernel of this
 * library: 0 for the shipped build; SRCDSP_BUILD_CORR_ALWAYS_EXACT for the
 * test-only always-exact correlator build (tests/_build/). */
#define SRCDSP_BUILD_CORR_ALWAYS_EXACT 1u
SRCDSP_API int srcdsp_build_flags(unsigned *flags);
/* Fill d_out with the counter-based synthetic samples the benchmarks use
 * (SURVEY.md §8d): component c of sample i (global index off+i) is
 * lo + (splitmix64((seed ^ channel<<40) + 2(off+i) + c) >> 32) mod (hi-lo+1).
 * kind 0 = complex<float>, 1 = complex<int16_t>. */
SRCDSP_API int srcdsp_fill_synthetic(void *d_out, int kind, size_t n, uint64_t seed, uint64_t channel,
                                     uint64_t offset, int lo, int hi, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCDSP_HIP_H */
