/*
 * Drop-in for SrcDsp's dsptl_miscellaneous.h: estimateFreq<int16_t, L>
 * (reference dsptl_miscellaneous.h:43-58), executed by libsrcdsp_hip.so, and
 * the two frequency conversions dsptl::toFreqHz / dsptl::toFreqRadPerSample
 * (dsptl_miscellaneous.h:145-148), here inline.
 *
 * estimateFreq is provided for InType = int16_t only: there every term is an
 * int and the sums are order-free, so the device computes them exactly.  The
 * float instantiation adds rounded products to a running double in order,
 * which a parallel sum cannot reproduce: other InTypes are declared and not
 * defined (an incomplete type: a compile error, not another number).
 *
 * estimateShiftFactor and bits2HexStr of the reference header are host scalar
 * and string utilities with no sample buffer behind them; they stay out.
 */
#ifndef SRCDSP_DROPIN_DSPTL_MISCELLANEOUS_H
#define SRCDSP_DROPIN_DSPTL_MISCELLANEOUS_H

#include "srcdsp_dropin_common.h"

namespace dsptl {
namespace srcdsp_detail {

/// one estimator handle for the length of a call
struct FreqEstHandle {
    srcdsp_freqest_t h;
    explicit FreqEstHandle(int L) : h(nullptr) { check(srcdsp_freqest_create(&h, L), "estimateFreq"); }
    ~FreqEstHandle() { srcdsp_freqest_destroy(h); }
    FreqEstHandle(const FreqEstHandle &) = delete;
    FreqEstHandle &operator=(const FreqEstHandle &) = delete;
};

}  // namespace srcdsp_detail

/// rad/sample -> Hz
inline double toFreqHz(double freqRadPerSample, double samplingFreqHz) {
    return freqRadPerSample / 2.0 / 3.141592653589793238462643383279502884 * samplingFreqHz;
}

/// Hz -> rad/sample
inline double toFreqRadPerSample(double freqHz, double samplingFreqHz) {
    return 2.0 * 3.141592653589793238462643383279502884 * freqHz / samplingFreqHz;
}

}  // namespace dsptl

/// dsptl_miscellaneous.h:43-58 (global namespace, as in the reference)
template <class InType, int L>
float estimateFreq(std::vector<std::complex<InType>> in);

template <class InType, int L>
float estimateFreq(dsptl::DeviceSpan<const std::complex<InType>> in, void *stream = nullptr);

namespace dsptl {
namespace srcdsp_detail {

template <class InType, int L>
struct EstimateFreq;  // InType = int16_t only

template <int L>
struct EstimateFreq<int16_t, L> {
    static_assert(L >= 1, "estimateFreq: L is at least 1");
    static float host(const std::vector<std::complex<int16_t>> &in) {
        FreqEstHandle e(L);
        float f = 0.f;
        check(srcdsp_freqest_run_host(e.h, in.data(), in.size(), &f, nullptr, nullptr), "estimateFreq");
        return f;
    }
    static float device(const DeviceSpan<const std::complex<int16_t>> &in, void *stream) {
        FreqEstHandle e(L);
        float f = 0.f;
        check(srcdsp_freqest_run(e.h, in.data, in.size, &f, nullptr, nullptr, stream), "estimateFreq(device)");
        return f;
    }
};

}  // namespace srcdsp_detail
}  // namespace dsptl

template <class InType, int L>
float estimateFreq(std::vector<std::complex<InType>> in) {
    return dsptl::srcdsp_detail::EstimateFreq<InType, L>::host(in);
}

/// device input: the frequency of in.size samples in device memory
template <class InType, int L>
float estimateFreq(dsptl::DeviceSpan<const std::complex<InType>> in, void *stream) {
    return dsptl::srcdsp_detail::EstimateFreq<InType, L>::device(in, stream);
}

#endif
