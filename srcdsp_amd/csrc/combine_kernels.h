// combine_kernels.h -- the carrier combiner's arithmetic, one source for the
// kernel (combine.hip) and for the host: srcdsp_combine_step_host and the
// stand-alone host program of the tests (tests/cpp/combine_host.cpp).  Nothing
// here needs the HIP headers.
//
// An extension with no reference call, defined through the reference's
// limitScale<complex<int16_t>, complex<int32_t>> (dsp_complex.h:83-108):
//   out[i] = limitScale(sum_{c < rows} in[c * stride + i], shift)
// A sample is a packed word, lo = re, hi = im.  The sum is exact in int32
// (rows <= 65 535: 65 535 * -32 768 > INT32_MIN), the shift is arithmetic and
// the clamp is to [-32768, 32767], each per component.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SRCDSP_COMBINE_HD __host__ __device__ inline
#else
#define SRCDSP_COMBINE_HD inline
#endif

namespace srcdsp {

constexpr long kCombineMaxRows = 65535;   // rows * 32768 stays inside int32
constexpr unsigned kCombineMaxShift = 15;
constexpr int kCombineBlock = 256;        // lanes of a workgroup
constexpr int kCombineLaneWords = 4;      // one 16-byte load per row and one 16-byte store per lane
constexpr int kCombineTileWords = kCombineBlock * kCombineLaneWords;
constexpr int kCombineWgPerCu = 8;        // persistent workgroups per compute unit
// Rows whose 16-byte loads a lane issues together: four, or one for a few long
// rows (rows <= kCombineFewRows and n >= kCombineLongRow), where the ten shapes
// measured take 4.9 % less time in all with one (0.83-1.04 of four's time shape
// by shape); elsewhere neither wins across sizes and four stays
constexpr int kCombineRowsInFlight = 4;
constexpr long kCombineFewRows = 8;
constexpr long kCombineLongRow = 1L << 22;

// one more row's sample onto the running sums
SRCDSP_COMBINE_HD void combine_add(int32_t &re, int32_t &im, uint32_t w) {
    re += (int32_t)(int16_t)(uint16_t)(w & 0xffffu);
    im += (int32_t)(int16_t)(uint16_t)(w >> 16);
}
// limitScale, one component (dsp_complex.h:92-104)
SRCDSP_COMBINE_HD int32_t combine_limit(int32_t v, unsigned shift) {
    const int32_t a = v >> shift;
    return a > 32767 ? 32767 : (a < -32768 ? -32768 : a);
}
SRCDSP_COMBINE_HD uint32_t combine_word(int32_t re, int32_t im, unsigned shift) {
    return ((uint32_t)combine_limit(re, shift) & 0xffffu) | ((uint32_t)combine_limit(im, shift) << 16);
}
// out[i] of a step: every row's sample i is read before anything is returned,
// so the caller may store it over row 0's
SRCDSP_COMBINE_HD uint32_t combine_sample(const uint32_t *in, long stride, long rows, long i, unsigned shift) {
    int32_t re = 0, im = 0;
    for (long c = 0; c < rows; ++c) combine_add(re, im, in[c * stride + i]);
    return combine_word(re, im, shift);
}

// ---------------------------------------------------------------- host form
// one step on host buffers; out may be row 0
inline void combine_host_run(const uint32_t *in, size_t stride, size_t rows, size_t n, unsigned shift, uint32_t *out) {
    for (size_t i = 0; i < n; ++i) out[i] = combine_sample(in, (long)stride, (long)rows, (long)i, shift);
}

}  // namespace srcdsp
