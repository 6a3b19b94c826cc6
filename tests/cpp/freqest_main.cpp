// One source, two builds: the reference's estimateFreq<int16_t, L> (its
// headers where they lie; made only where the reference is, by
// tests/golden/gen_freqest_golden.py) and the drop-in (-I include/srcdsp,
// linked with libsrcdsp_hip.so; made on the GPU box by
// tests/test_freqest_dropin_cpp.py).  The two builds must write identical bytes.
//
//   freqest_main <case.bin> <out.bin> [<case.bin> <out.bin> ...]
// case.bin (little endian): int32 L, int32 n, then n int16 (re, im) samples.
// out.bin: the returned float.  L is one of the instantiations below.
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>
#include "dsptl_miscellaneous.h"
#include <cstdio>
#include <fstream>

static int run_case(const char *case_path, const char *out_path) {
    std::ifstream f(case_path, std::ios::binary);
    if (!f) return 2;
    int32_t L = 0, n = 0;
    f.read((char *)&L, 4);
    f.read((char *)&n, 4);
    std::vector<std::complex<int16_t>> x;
    int16_t v[2];
    while (f.read((char *)v, 4)) x.emplace_back(v[0], v[1]);
    if ((size_t)n != x.size()) return 3;
    float r = 0.f;
    switch (L) {
    case 1: r = estimateFreq<int16_t, 1>(x); break;
    case 2: r = estimateFreq<int16_t, 2>(x); break;
    case 3: r = estimateFreq<int16_t, 3>(x); break;
    case 4: r = estimateFreq<int16_t, 4>(x); break;
    case 8: r = estimateFreq<int16_t, 8>(x); break;
    case 32: r = estimateFreq<int16_t, 32>(x); break;
    default: return 5;
    }
    std::ofstream out(out_path, std::ios::binary);
    out.write((const char *)&r, 4);
    return out.good() ? 0 : 4;
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
