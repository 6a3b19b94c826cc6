// The drop-in dsptl::QStagger (include/srcdsp/modulators.h, an extension with
// no reference class) over the C ABI, linked with libsrcdsp_hip.so.  Only the
// public interface is driven; tests/test_stagger_capi.py compares out.bin with
// the numpy model.
//
//   stagger_main <D> <in.bin> <out.bin> <copy_before> <reset_before> <n0> [<n1> ...]
// in.bin: complex<int16_t> samples, stepped in calls of n0, n1, ... samples
// through the std::vector step().  From call copy_before on the stream goes on
// with a value copy; reset() comes before call reset_before (-1: never).
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "modulators.h"

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int16_t *x = (const int16_t *)raw.data();
    std::ofstream out(argv[3], std::ios::binary);
    const int copy_before = std::atoi(argv[4]), reset_before = std::atoi(argv[5]);
    dsptl::QStagger first((unsigned)std::atoi(argv[1]));
    dsptl::QStagger copy(1);
    dsptl::QStagger *g = &first;
    if (g->getDelay() != (unsigned)std::atoi(argv[1])) return 5;
    size_t pos = 0;
    for (int a = 6; a < argc; ++a) {
        const int c = a - 6;
        if (c == copy_before) {
            copy = first;
            g = &copy;
        }
        if (c == reset_before) g->reset();
        const size_t n = (size_t)std::atol(argv[a]);
        if (4 * (pos + n) > raw.size()) return 3;
        std::vector<std::complex<int16_t>> in(n), y(n);
        for (size_t i = 0; i < n; ++i) in[i] = std::complex<int16_t>(x[2 * (pos + i)], x[2 * (pos + i) + 1]);
        pos += n;
        g->step(in, y);
        for (const auto &s : y) {
            const int16_t v[2] = {s.real(), s.imag()};
            out.write((const char *)v, 4);
        }
    }
    return out.good() ? 0 : 4;
}
