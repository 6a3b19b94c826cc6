// The library's per-pair arithmetic (srcdsp_amd/csrc/freqest_pair.h), the one
// source of the kernel, the host form and the join, as a stand-alone host
// program for the address and undefined-behaviour sanitisers
// (tests/test_freqest_capi.py).
//
//   freqest_host <case.bin> <out.bin> [<case.bin> <out.bin> ...]
// case.bin as tests/cpp/freqest_main.cpp reads it: int32 L, int32 n, n int16
// (re, im) samples.  out.bin: float freq, int64 sumI, int64 sumQ, int32 exact.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <vector>

#include "freqest_pair.h"

static int run_case(const char *case_path, const char *out_path) {
    std::ifstream f(case_path, std::ios::binary);
    if (!f) return 2;
    int32_t L = 0, n = 0;
    f.read((char *)&L, 4);
    f.read((char *)&n, 4);
    if (L < 1 || n < 0) return 5;
    std::vector<uint32_t> x((size_t)n);
    f.read((char *)x.data(), 4 * (std::streamsize)n);
    if (!f && n) return 3;
    const srcdsp::FreqAcc a = srcdsp::freqest_row_host(x.data(), x.size(), (size_t)L);
    const float freq = static_cast<float>(std::atan2((double)a.sq, (double)a.si) / L);
    const int64_t si = a.si, sq = a.sq;
    const int32_t exact = srcdsp::freqest_exact(n > L ? (uint64_t)(n - L) : 0, srcdsp::freqest_bound(a.hi, a.lo));
    std::ofstream out(out_path, std::ios::binary);
    out.write((const char *)&freq, 4);
    out.write((const char *)&si, 8);
    out.write((const char *)&sq, 8);
    out.write((const char *)&exact, 4);
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
