// corr_all_main.cpp -- dsptl::FixedPatternCorrelator<int16_t, int32_t, 32, 1>::stepAll
// (include/srcdsp/correlators.h, an extension member) over the C ABI, on a
// host vector and on the remainder after maxHits was reached.
//
//   corr_all_main pattern.bin in.bin maxHits
//
// Prints one line per call: consumed, then the indices; then the last
// detection's bit samples as getRefBitSamples() returns them and as stepAll did.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "correlators.h"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const size_t N = 32;
    std::array<std::complex<int32_t>, N> p;
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(p.data(), 8, N, f) != N) return 2;
    fclose(f);
    std::vector<std::complex<int16_t>> x;
    f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::complex<int16_t> s;
    while (fread(&s, 4, 1, f) == 1) x.push_back(s);
    fclose(f);
    dsptl::FixedPatternCorrelator<int16_t, int32_t, N, 1> c;
    c.setPattern(p);
    std::vector<int> idx;
    std::vector<std::vector<std::complex<int16_t>>> bits, last;
    size_t pos = 0;
    while (pos < x.size()) {
        std::vector<std::complex<int16_t>> rest(x.begin() + pos, x.end());
        const size_t used = c.stepAll(rest, atoi(argv[3]), idx, bits);
        printf("%zu", used);
        for (size_t k = 0; k < idx.size(); ++k) printf(" %d", idx[k]);
        printf("\n");
        if (!bits.empty()) last = bits;
        if (used == 0) return 3;
        pos += used;
    }
    const std::vector<std::complex<int16_t>> b = c.getRefBitSamples();
    for (size_t m = 0; m < N; ++m) printf("%d %d ", (int)b[m].real(), (int)b[m].imag());
    printf("\n");
    if (!last.empty())
        for (size_t m = 0; m < N; ++m) printf("%d %d ", (int)last.back()[m].real(), (int)last.back()[m].imag());
    printf("\n");
    return 0;
}
