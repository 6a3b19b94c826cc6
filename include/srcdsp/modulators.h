/*
 * Drop-in for SrcDsp's modulators.h: dsptl::SymbolMapperSdpsk<int16_t>
 * (reference modulators.h:82-131) and dsptl::SymbolMapperQpsk<int16_t>
 * (reference modulators.h:147-198), executed by libsrcdsp_hip.so.
 *
 * Only T = int16_t (amplitude 8192, modulators.h:34-39) is defined: it is what
 * the interpolators consume.  The other T are declared and not defined, so a
 * use of one fails to compile instead of running something else.
 *
 * A std::vector step() of an object that has only ever seen host buffers maps
 * on the host with the kernels' own arithmetic; the DeviceSpan overload runs
 * the kernels.  Many bursts are stepped at once through the C ABI's
 * srcdsp_mapper_step_batched, and straight onto a carrier through
 * srcdsp_modulate_step(_batched).
 *
 * dsptl::QStagger is an extension with no reference class: the delay line on
 * the Q rail that makes the QPSK mapper's signal offset QPSK (the reference
 * leaves it to the application); srcdsp_modulate_offset_step(_batched) runs it
 * inside the transmit chain.  dsptl::combineCarriers, an extension too, puts C
 * carriers onto one wire (srcdsp_combine_step).
 *
 * Where the reference asserts (bits.size() against out.size(), :106 and :171)
 * the calls fail as the other drop-ins do (assert, or std::runtime_error
 * under NDEBUG).
 */
#ifndef SRCDSP_DROPIN_MODULATORS_H
#define SRCDSP_DROPIN_MODULATORS_H

#include <algorithm>

#include "srcdsp_dropin_common.h"

namespace dsptl {

template <class T>
class SymbolMapperSdpsk;
template <class T>
class SymbolMapperQpsk;

namespace srcdsp_detail {

/// what the two mappers share: the handle, its copies and the two step()s
template <int Kind>
class MapperBase {
public:
    MapperBase() : h_(nullptr) { check(srcdsp_mapper_create(&h_, Kind), "SymbolMapper"); }
    ~MapperBase() { srcdsp_mapper_destroy(h_); }
    /// copies (a value type in the reference): the state comes along
    MapperBase(const MapperBase &o) : h_(clone_handle(o.h_, srcdsp_mapper_clone, "SymbolMapper(copy)")) {}
    MapperBase(MapperBase &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    MapperBase &operator=(MapperBase o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }

    /// modulators.h:103-117 / :169-184
    void step(const std::vector<uint8_t> &bits, std::vector<std::complex<int16_t>> &out) {
        check(srcdsp_mapper_step_host(h_, bits.data(), bits.size(), out.data(), out.size()), "step");
    }
    /// device bits, device symbols
    void step(const DeviceSpan<const uint8_t> &bits, DeviceSpan<std::complex<int16_t>> out, void *stream = nullptr) {
        check(srcdsp_mapper_step(h_, bits.data, bits.size, out.data, out.size, stream), "step(device)");
    }
    /// modulators.h:120-123 / :187-190
    void reset() { check(srcdsp_mapper_reset(h_), "reset"); }
    /// the C ABI handle, for srcdsp_mapper_step_batched and srcdsp_modulate_step
    srcdsp_mapper_t handle() const { return h_; }

private:
    srcdsp_mapper_t h_;
};

}  // namespace srcdsp_detail

template <>
class SymbolMapperSdpsk<int16_t> : public srcdsp_detail::MapperBase<SRCDSP_MAPPER_SDPSK> {};

template <>
class SymbolMapperQpsk<int16_t> : public srcdsp_detail::MapperBase<SRCDSP_MAPPER_QPSK> {};

/// Extension (no reference class): the offset of offset-QPSK, which the
/// reference leaves to the application ("for QPSK or OQPSK modulations",
/// modulators.h:147): a delay line of D samples, 1..64, on the imaginary rail
/// between FilterUpsamplingFir::step and Mixer::step.  out[i] = (re(in[i]),
/// im(in[i - D])), the first D imaginary halves carried over from the step
/// before (zeros at first).  A value type like the mappers; in and out may not
/// overlap.  srcdsp_modulate_offset_step(_batched) takes handle().
class QStagger {
public:
    explicit QStagger(unsigned D) : h_(nullptr) { srcdsp_detail::check(srcdsp_stagger_create(&h_, D), "QStagger"); }
    ~QStagger() { srcdsp_stagger_destroy(h_); }
    QStagger(const QStagger &o) : h_(srcdsp_detail::clone_handle(o.h_, srcdsp_stagger_clone, "QStagger(copy)")) {}
    QStagger(QStagger &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    QStagger &operator=(QStagger o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }

    void step(const std::vector<std::complex<int16_t>> &in, std::vector<std::complex<int16_t>> &out) {
        srcdsp_detail::check_shape(in.size() == out.size(), "QStagger::step: in and out differ in size");
        srcdsp_detail::check(srcdsp_stagger_step_host(h_, in.data(), in.size(), out.data()), "step");
    }
    /// device samples in, device samples out
    void step(const DeviceSpan<const std::complex<int16_t>> &in, DeviceSpan<std::complex<int16_t>> out,
              void *stream = nullptr) {
        srcdsp_detail::check_shape(in.size == out.size, "QStagger::step: in and out differ in size");
        srcdsp_detail::check(srcdsp_stagger_step(h_, in.data, in.size, out.data, stream), "step(device)");
    }
    /// the carry back to zeros
    void reset() { srcdsp_detail::check(srcdsp_stagger_reset(h_), "reset"); }
    unsigned getDelay() const {
        unsigned d = 0;
        srcdsp_detail::check(srcdsp_stagger_get_state(h_, &d, nullptr), "getDelay");
        return d;
    }
    srcdsp_stagger_t handle() const { return h_; }

private:
    srcdsp_stagger_t h_;
};

/// Extension (no reference call): C carriers onto one wire.  out[i] =
/// limitScale<complex<int16_t>, complex<int32_t>>(sum_c rows[c][i], shift)
/// (dsp_complex.h:83-108): the exact int32 sum, shifted right arithmetically
/// and clamped to int16, per component.  1..65535 rows of one size, shift
/// 0..15.  On device rows: srcdsp_combine_step.
inline std::vector<std::complex<int16_t>> combineCarriers(const std::vector<std::vector<std::complex<int16_t>>> &rows,
                                                          unsigned shift) {
    srcdsp_detail::check_shape(!rows.empty(), "combineCarriers: no rows");
    const size_t n = rows[0].size();
    for (size_t c = 1; c < rows.size(); ++c)
        srcdsp_detail::check_shape(rows[c].size() == n, "combineCarriers: the rows differ in size");
    // the C ABI takes rows of one buffer
    std::vector<std::complex<int16_t>> flat(rows.size() * n), out(n);
    for (size_t c = 0; c < rows.size(); ++c) std::copy(rows[c].begin(), rows[c].end(), flat.begin() + c * n);
    srcdsp_detail::check(srcdsp_combine_step_host(flat.data(), n, rows.size(), out.data(), n, shift),
                         "combineCarriers");
    return out;
}

}  // namespace dsptl
#endif
