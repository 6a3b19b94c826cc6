// The carrier combiner's arithmetic (srcdsp_amd/csrc/combine_kernels.h: the one
// source of the kernel's per-sample code and of srcdsp_combine_step_host)
// compiled for the host, stand-alone, so that it can run under the address and
// undefined-behaviour sanitisers (tests/test_combine_capi.py).
//
//   combine_host <in.bin> <out.bin> <rows> <stride> <n> <shift> <in_place>
// in.bin: exactly (rows - 1) * stride + n complex<int16_t> samples, row c from
// sample c * stride.  out.bin gets the n combined samples; with in_place = 1
// they are written over row 0 and taken from there.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "combine_kernels.h"

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t rows = (size_t)std::atol(argv[3]), stride = (size_t)std::atol(argv[4]), n = (size_t)std::atol(argv[5]);
    const unsigned shift = (unsigned)std::atoi(argv[6]);
    const bool in_place = std::atoi(argv[7]) != 0;
    if (rows < 1 || rows > (size_t)srcdsp::kCombineMaxRows || shift > srcdsp::kCombineMaxShift) return 2;
    const size_t words = (rows - 1) * stride + n;
    if (raw.size() != 4 * words) return 3;
    // exactly sized copies, so that a read or write past either end is seen
    std::vector<uint32_t> in(words), y(in_place ? 0 : n);
    if (words) std::memcpy(in.data(), raw.data(), 4 * words);
    uint32_t *out = in_place ? in.data() : y.data();
    srcdsp::combine_host_run(in.data(), stride, rows, n, shift, out);
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char *)out, (std::streamsize)(4 * n));
    return o.good() ? 0 : 4;
}
