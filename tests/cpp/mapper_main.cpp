// One source, two builds: the reference's SymbolMapperSdpsk<int16_t> /
// SymbolMapperQpsk<int16_t> (its modulators.h where it lies; made only where
// the reference is, by tests/golden/gen_mapper_golden.py, which also defines
// MAPPER_OPEN_STATE to record the private state) and the drop-in
// (-I include/srcdsp, linked with libsrcdsp_hip.so; made on the GPU box by
// tests/test_gpu_mapper.py).  Only the public interface is driven, and the two
// builds must write identical out.bin bytes.
//
//   mapper_main <case.bin> <out.bin> [<case.bin> <out.bin> ...]
// case.bin (little endian):
//   int32 kind                       0 SDPSK, 1 QPSK
//   int32 reset_before               reset() before this call (-1: never)
//   int32 copy_before                go on with a value copy from this call (-1: never)
//   int32 calls, int32 len[calls]    step() bit counts
//   uint8 bits to the end of the file
// out.bin gets per call: int32 symbols, then their int16 (re, im).  With
// MAPPER_OPEN_STATE, <out.bin>.state gets the int32 state after every call.
#include <cassert>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>
#ifdef MAPPER_OPEN_STATE
#define private public
#endif
#include "modulators.h"
#ifdef MAPPER_OPEN_STATE
#undef private
#endif

template <class T>
static T get(std::ifstream &f) {
    T v{};
    f.read((char *)&v, sizeof v);
    return v;
}

template <class Mapper>
static int run(std::ifstream &f, int div, const char *out_path) {
    const int32_t reset_before = get<int32_t>(f), copy_before = get<int32_t>(f);
    std::vector<int32_t> len((size_t)get<int32_t>(f));
    for (auto &l : len) l = get<int32_t>(f);
    std::vector<uint8_t> bits;
    char b;
    while (f.read(&b, 1)) bits.push_back((uint8_t)b);

    Mapper first;
    Mapper *mapper = &first;
    Mapper copy;
    std::ofstream out(out_path, std::ios::binary);
#ifdef MAPPER_OPEN_STATE
    std::ofstream st(std::string(out_path) + ".state", std::ios::binary);
#endif
    size_t pos = 0;
    for (size_t c = 0; c < len.size(); ++c) {
        if ((int32_t)c == copy_before) {
            copy = first;
            mapper = &copy;
        }
        if ((int32_t)c == reset_before) mapper->reset();
        if (pos + (size_t)len[c] > bits.size()) return 3;
        const std::vector<uint8_t> in(bits.begin() + pos, bits.begin() + pos + len[c]);
        pos += (size_t)len[c];
        std::vector<std::complex<int16_t>> sym((size_t)len[c] / div);
        mapper->step(in, sym);
        const int32_t ns = (int32_t)sym.size();
        out.write((const char *)&ns, 4);
        for (const auto &s : sym) {
            const int16_t v[2] = {s.real(), s.imag()};
            out.write((const char *)v, 4);
        }
#ifdef MAPPER_OPEN_STATE
        const int32_t state = mapper->state;
        st.write((const char *)&state, 4);
#endif
    }
    return out.good() ? 0 : 4;
}

static int run_case(const char *case_path, const char *out_path) {
    std::ifstream f(case_path, std::ios::binary);
    if (!f) return 2;
    const int32_t kind = get<int32_t>(f);
    if (kind == 0) return run<dsptl::SymbolMapperSdpsk<int16_t>>(f, 1, out_path);
    if (kind == 1) return run<dsptl::SymbolMapperQpsk<int16_t>>(f, 2, out_path);
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 3 || argc % 2 != 1) {
        std::fprintf(stderr, "usage: %s case.bin out.bin [case.bin out.bin ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; a += 2) {
        const int rc = run_case(argv[a], argv[a + 1]);
        if (rc) return rc;
    }
    return 0;
}
