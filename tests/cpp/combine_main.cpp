// The drop-in dsptl::combineCarriers (include/srcdsp/modulators.h, an extension
// with no reference call) over the C ABI, linked with libsrcdsp_hip.so.
// tests/test_combine_capi.py compares out.bin with the numpy model.
//
//   combine_main <in.bin> <out.bin> <rows> <n> <shift>
// in.bin: rows x n complex<int16_t> samples, row after row.  Exit status 6 when
// rows of different sizes are not refused.
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

#include "modulators.h"

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int16_t *x = (const int16_t *)raw.data();
    const size_t rows = (size_t)std::atol(argv[3]), n = (size_t)std::atol(argv[4]);
    if (raw.size() != 4 * rows * n) return 3;
    std::vector<std::vector<std::complex<int16_t>>> in(rows, std::vector<std::complex<int16_t>>(n));
    for (size_t c = 0; c < rows; ++c)
        for (size_t i = 0; i < n; ++i) in[c][i] = std::complex<int16_t>(x[2 * (c * n + i)], x[2 * (c * n + i) + 1]);
    const std::vector<std::complex<int16_t>> y = dsptl::combineCarriers(in, (unsigned)std::atoi(argv[5]));
    if (y.size() != n) return 5;
    std::ofstream out(argv[2], std::ios::binary);
    for (const auto &s : y) {
        const int16_t v[2] = {s.real(), s.imag()};
        out.write((const char *)v, 4);
    }
#ifdef NDEBUG
    if (rows > 1) {  // rows of different sizes are refused
        in[1].push_back(std::complex<int16_t>(1, 1));
        try {
            (void)dsptl::combineCarriers(in, 0);
            return 6;
        } catch (const std::length_error &) {
        }
    }
#endif
    return out.good() ? 0 : 4;
}
