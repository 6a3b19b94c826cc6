// The stagger's arithmetic (srcdsp_amd/csrc/stagger_kernels.h: the one source
// of the kernels' per-sample code and of the carry update) compiled for the
// host, stand-alone, so that it can run under the address and
// undefined-behaviour sanitisers (tests/test_stagger_capi.py).
//
//   stagger_host <D> <in.bin> <out.bin> <n0> [<n1> ...]
// in.bin: complex<int16_t> samples; the stream is stepped in calls of n0, n1,
// ... samples.  out.bin gets every call's output; stdout the carry after every
// call, one line each.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "stagger_kernels.h"

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const unsigned D = (unsigned)std::atoi(argv[1]);
    if (D < 1 || D > srcdsp::kStaggerMaxD) return 2;
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[3], std::ios::binary);
    // exactly D values, so that a read or write past the carry's end is seen
    std::vector<int16_t> carry(D, 0);
    size_t pos = 0;
    for (int a = 4; a < argc; ++a) {
        const size_t n = (size_t)std::atol(argv[a]);
        if (4 * (pos + n) > raw.size()) return 3;
        // exactly sized copies, so that a read or write past either end is seen
        std::vector<uint32_t> in(n), y(n);
        for (size_t i = 0; i < n; ++i) {
            const unsigned char *b = (const unsigned char *)raw.data() + 4 * (pos + i);
            in[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        pos += n;
        srcdsp::stagger_host_run(carry.data(), D, in.data(), n, y.data());
        out.write((const char *)y.data(), (std::streamsize)(4 * n));
        for (unsigned k = 0; k < D; ++k) std::printf("%d%c", (int)carry[k], k + 1 == D ? '\n' : ' ');
    }
    return out.good() ? 0 : 4;
}
