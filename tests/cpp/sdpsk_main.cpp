// The drop-in dsptl::DemodulatorSdpsk<int16_t> (include/srcdsp/demodulators.h,
// an extension with no reference class) over the C ABI, linked with
// libsrcdsp_hip.so.  tests/test_sdpsk_capi.py compares out.bin with the numpy
// model.
//
//   sdpsk_main <in.bin> <out.bin> <D> <shift> <cut>
// in.bin: complex<int16_t> samples.  The soft bits come from one object stepped
// over [0, cut) and [cut, n) at `shift`; the bits from a copy taken after the
// first step (it continues the stream), the first part from a second object.
// out.bin: n soft bits, then n bits.  Exit status 6 when reset() or setShift()
// do not do what they say.
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "demodulators.h"

typedef std::vector<std::complex<int16_t>> samples_t;

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int16_t *x = (const int16_t *)raw.data();
    const size_t n = raw.size() / 4, cut = (size_t)std::atol(argv[5]);
    const unsigned D = (unsigned)std::atoi(argv[3]), shift = (unsigned)std::atoi(argv[4]);
    if (cut > n) return 3;
    samples_t a, b;
    for (size_t i = 0; i < n; ++i) (i < cut ? a : b).push_back(std::complex<int16_t>(x[2 * i], x[2 * i + 1]));

    dsptl::DemodulatorSdpsk<int16_t> soft_demod(D, 0), bits_demod(D, shift);
    soft_demod.setShift(shift);
    std::vector<int8_t> s0, s1;
    std::vector<uint8_t> b0, b1;
    soft_demod.step(a, s0);
    dsptl::DemodulatorSdpsk<int16_t> copy(soft_demod);  // D, shift and carry
    soft_demod.step(b, s1);
    bits_demod.step(a, b0);
    copy.step(b, b1);
    if (s0.size() != a.size() || s1.size() != b.size() || b0.size() != a.size() || b1.size() != b.size()) return 5;

    // reset(): the stream starts again
    std::vector<int8_t> again;
    soft_demod.reset();
    soft_demod.step(a, again);
    if (again != s0) return 6;

    std::ofstream out(argv[2], std::ios::binary);
    out.write((const char *)s0.data(), (std::streamsize)s0.size());
    out.write((const char *)s1.data(), (std::streamsize)s1.size());
    out.write((const char *)b0.data(), (std::streamsize)b0.size());
    out.write((const char *)b1.data(), (std::streamsize)b1.size());
    return out.good() ? 0 : 4;
}
