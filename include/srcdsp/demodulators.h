/*
 * Drop-in for SrcDsp's demodulators.h: dsptl::DemodulatorOqpsk<int16_t>
 * (reference demodulators.h:53-130, demodulators.cpp:34-308), executed by
 * libsrcdsp_hip.so.
 *
 * One burst is a sequential recurrence (the PLL) and runs on one GPU lane, so
 * this single-object step() is slower than the reference on a host core; it
 * is here for parity and state continuity.  Many bursts are stepped at once
 * through the C ABI's srcdsp_demod_step_batched.
 *
 * Where the reference is undefined the calls fail as the other drop-ins do
 * (assert, or std::runtime_error under NDEBUG): a first step() of no more
 * samples than the sync pattern has bits, a preamble longer than the
 * reference vector, a frequency word outside +-4096.
 *
 * dsptl::DemodulatorSdpsk<int16_t> is an extension with no reference class:
 * the differential receiver of SymbolMapperSdpsk, one independent decision per
 * sample; its bank is srcdsp_sdpsk_step_batched.
 */
#ifndef SRCDSP_DROPIN_DEMODULATORS_H
#define SRCDSP_DROPIN_DEMODULATORS_H

#include "srcdsp_dropin_common.h"

namespace dsptl {

template <class InType>
class DemodulatorOqpsk;

template <class InType, class CompType, size_t N, size_t S>
class FixedPatternCorrelator;

template <>
class DemodulatorOqpsk<int16_t> {
public:
    /// demodulators.cpp:34-58
    DemodulatorOqpsk() : h_(nullptr) { srcdsp_detail::check(srcdsp_demod_create(&h_), "DemodulatorOqpsk"); }
    ~DemodulatorOqpsk() { srcdsp_demod_destroy(h_); }
    /// copies (a value type in the reference): configuration and state
    DemodulatorOqpsk(const DemodulatorOqpsk &o)
        : h_(srcdsp_detail::clone_handle(o.h_, srcdsp_demod_clone, "DemodulatorOqpsk(copy)")) {}
    DemodulatorOqpsk(DemodulatorOqpsk &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DemodulatorOqpsk &operator=(DemodulatorOqpsk o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }

    /// demodulators.cpp:150-284; the vector is sized as the reference sizes it
    std::vector<int8_t> step(const std::vector<std::complex<int16_t>> &in, int32_t &error) {
        std::vector<int8_t> soft(in.size());
        size_t ns = 0;
        int32_t e = 0;
        srcdsp_detail::check(srcdsp_demod_step_host(h_, in.data(), in.size(), soft.data(), soft.size(), &ns, &e),
                             "step");
        soft.resize(ns);
        error = e;
        return soft;
    }
    /// device input, device soft bits (room for in.size); returns their count
    size_t step(const DeviceSpan<const std::complex<int16_t>> &in, DeviceSpan<int8_t> soft, int32_t &error,
                void *stream = nullptr) {
        size_t ns = 0;
        int32_t e = 0;
        srcdsp_detail::check(srcdsp_demod_step(h_, in.data, in.size, soft.data, soft.size, &ns, &e, stream),
                             "step(device)");
        error = e;
        return ns;
    }
    /// demodulators.cpp:293-308
    void reset() { srcdsp_detail::check(srcdsp_demod_reset(h_), "reset"); }
    /// demodulators.h:60
    void setSyncPattern(std::vector<int8_t> bits) {
        srcdsp_detail::check(srcdsp_demod_set_sync_pattern(h_, bits.data(), (int)bits.size()), "setSyncPattern");
    }
    /// demodulators.h:64
    void setInitialFrequency(float f) {
        srcdsp_detail::check(srcdsp_demod_set_initial_frequency(h_, f), "setInitialFrequency");
    }
    /// demodulators.h:66
    void setInitialPhase(float p) { srcdsp_detail::check(srcdsp_demod_set_initial_phase(h_, p), "setInitialPhase"); }
    /// demodulators.cpp:126-139
    void setReference(std::vector<std::complex<int16_t>> ref) {
        srcdsp_detail::check(srcdsp_demod_set_reference(h_, reinterpret_cast<const int16_t *>(ref.data()),
                                                        (int)ref.size()),
                             "setReference");
    }
    /// setReference(corr.getRefBitSamples()) without the vector in between:
    /// the bit samples are taken from the correlator's handle
    template <size_t N, size_t S>
    void setReference(FixedPatternCorrelator<int16_t, int32_t, N, S> &corr, void *stream = nullptr) {
        srcdsp_detail::check(srcdsp_demod_set_reference_corr(h_, corr.handle(), stream), "setReference(correlator)");
    }
    /// demodulators.h:70
    void setInputShift(int shift) { srcdsp_detail::check(srcdsp_demod_set_input_shift(h_, shift), "setInputShift"); }
    /// demodulators.h:72
    float getMeasuredFrequency() {
        float f = 0.f;
        srcdsp_detail::check(srcdsp_demod_get_measured_frequency(h_, &f), "getMeasuredFrequency");
        return f;
    }
    /// the C ABI handle, for srcdsp_demod_step_batched
    srcdsp_demod_t handle() const { return h_; }

private:
    srcdsp_demod_t h_;
};

template <class InType>
class DemodulatorSdpsk;

/// Extension (no reference class): the receiver of SymbolMapperSdpsk
/// (modulators.h:82-131).  bit[i] = Im(x[i] conj(x[i - D])) > 0, soft[i] =
/// limitScale<int8_t, int32_t> of that product (dsp_complex.h:45-63), D the
/// samples per symbol (1..64), the samples before the first step zero.
template <>
class DemodulatorSdpsk<int16_t> {
public:
    explicit DemodulatorSdpsk(unsigned D = 1, unsigned shift = 0) : h_(nullptr) {
        srcdsp_detail::check(srcdsp_sdpsk_create(&h_, D, shift), "DemodulatorSdpsk");
    }
    ~DemodulatorSdpsk() { srcdsp_sdpsk_destroy(h_); }
    /// copies: D, the shift and the carry
    DemodulatorSdpsk(const DemodulatorSdpsk &o)
        : h_(srcdsp_detail::clone_handle(o.h_, srcdsp_sdpsk_clone, "DemodulatorSdpsk(copy)")) {}
    DemodulatorSdpsk(DemodulatorSdpsk &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DemodulatorSdpsk &operator=(DemodulatorSdpsk o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }

    /// soft bits, one per sample; the vector is sized to in.size()
    void step(const std::vector<std::complex<int16_t>> &in, std::vector<int8_t> &soft) {
        soft.resize(in.size());
        srcdsp_detail::check(srcdsp_sdpsk_step_host(h_, in.data(), in.size(), soft.data(), nullptr), "step");
    }
    /// hard bits (0 / 1), as SymbolMapperSdpsk::step takes them
    void step(const std::vector<std::complex<int16_t>> &in, std::vector<uint8_t> &bits) {
        bits.resize(in.size());
        srcdsp_detail::check(srcdsp_sdpsk_step_host(h_, in.data(), in.size(), nullptr, bits.data()), "step(bits)");
    }
    /// device input, device outputs of in.size each; either span may be empty
    void step(const DeviceSpan<const std::complex<int16_t>> &in, DeviceSpan<int8_t> soft, DeviceSpan<uint8_t> bits,
              void *stream = nullptr) {
        srcdsp_detail::check(srcdsp_sdpsk_step(h_, in.data, in.size, soft.data, bits.data, stream), "step(device)");
    }
    void reset() { srcdsp_detail::check(srcdsp_sdpsk_reset(h_), "reset"); }
    void setShift(unsigned shift) { srcdsp_detail::check(srcdsp_sdpsk_set_shift(h_, shift), "setShift"); }
    /// the C ABI handle, for srcdsp_sdpsk_step_batched
    srcdsp_sdpsk_t handle() const { return h_; }

private:
    srcdsp_sdpsk_t h_;
};

}  // namespace dsptl
#endif
