// The mappers' arithmetic (srcdsp_amd/csrc/mapper_kernels.h: the one source of
// the kernels' per-symbol code and of the scan's combine step) compiled for the
// host, stand-alone, so that it can run under the address and
// undefined-behaviour sanitisers (tests/test_mapper_capi.py).
//
//   mapper_host <case.bin> <out.bin> <tile_bits>
// case.bin and out.bin as tests/cpp/mapper_main.cpp reads and writes them; the
// stream of every call is cut into tiles of tile_bits, which exercises the
// scan's carry.  The state after every call goes to stdout.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "mapper_kernels.h"

template <class T>
static T get(std::ifstream &f) {
    T v{};
    f.read((char *)&v, sizeof v);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const int32_t kind = get<int32_t>(f), reset_before = get<int32_t>(f), copy_before = get<int32_t>(f);
    (void)copy_before;  // a copy of a value is the value
    std::vector<int32_t> len((size_t)get<int32_t>(f));
    for (auto &l : len) l = get<int32_t>(f);
    std::vector<uint8_t> bits;
    char b;
    while (f.read(&b, 1)) bits.push_back((uint8_t)b);
    const size_t tile = (size_t)std::atol(argv[3]);
    if (tile == 0 || (kind != srcdsp::MAPPER_SDPSK && kind != srcdsp::MAPPER_QPSK)) return 2;

    std::ofstream out(argv[2], std::ios::binary);
    uint32_t state = 0;
    size_t pos = 0;
    for (size_t c = 0; c < len.size(); ++c) {
        if ((int32_t)c == reset_before) state = 0;
        const size_t n = (size_t)len[c];
        if (pos + n > bits.size()) return 3;
        // exactly sized copies, so that a read or write past either end is seen
        const std::vector<uint8_t> in(bits.begin() + pos, bits.begin() + pos + n);
        pos += n;
        std::vector<uint32_t> sym(srcdsp::mapper_n_out(kind, n));
        state = srcdsp::mapper_host_run(kind, state, in.data(), n, sym.data(), tile);
        const int32_t ns = (int32_t)sym.size();
        out.write((const char *)&ns, 4);
        out.write((const char *)sym.data(), 4 * (size_t)ns);
        std::printf("%u\n", state);
    }
    return out.good() ? 0 : 4;
}
