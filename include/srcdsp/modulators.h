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
 * Where the reference asserts (bits.size() against out.size(), :106 and :171)
 * the calls fail as the other drop-ins do (assert, or std::runtime_error
 * under NDEBUG).
 */
#ifndef SRCDSP_DROPIN_MODULATORS_H
#define SRCDSP_DROPIN_MODULATORS_H

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

}  // namespace dsptl
#endif
