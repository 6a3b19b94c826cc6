// One source, two builds: the reference's DemodulatorOqpsk<int16_t> (its
// headers where they lie, linked with its demodulators.cpp; made only where
// the reference is, by tests/golden/gen_demod_golden.py) and the drop-in
// (-I include/srcdsp, linked with libsrcdsp_hip.so; made on the GPU box by
// tests/test_demod_dropin_cpp.py).  Only the public interface is driven, and
// the two builds must write identical bytes.
//
//   demod_main <case.bin> <out.bin> [<case.bin> <out.bin> ...]
// case.bin (little endian):
//   int32 P, int8 bits[P]            sync pattern (P = 0: none)
//   int32 R, int16 ref[2 R]          reference vector (re, im)
//   int32 shift, float freq          setInputShift, setInitialFrequency
//   int32 reset_before               reset() again before this chunk (-1: never)
//   int32 chunks, int32 len[chunks]  step() call lengths
//   int16 (re, im) samples to the end of the file
// The object is configured, reset(), then given its input shift (reset()
// clears it, demodulators.cpp:296).  out.bin gets per call: int32 size of the
// returned vector, its int8 soft bits, int32 error, float getMeasuredFrequency().
#include <cmath>
#include <cassert>
#include <complex>
#include <cstdint>
#include <vector>
#include "demodulators.h"
#include <cstdio>
#include <fstream>

template <class T>
static T get(std::ifstream &f) {
    T v{};
    f.read((char *)&v, sizeof v);
    return v;
}

static int run_case(const char *case_path, const char *out_path) {
    std::ifstream f(case_path, std::ios::binary);
    if (!f) return 2;
    std::vector<int8_t> bits((size_t)get<int32_t>(f));
    for (auto &b : bits) b = get<int8_t>(f);
    std::vector<std::complex<int16_t>> ref((size_t)get<int32_t>(f));
    for (auto &r : ref) {
        const int16_t re = get<int16_t>(f), im = get<int16_t>(f);
        r = std::complex<int16_t>(re, im);
    }
    const int32_t shift = get<int32_t>(f);
    const float freq = get<float>(f);
    const int32_t reset_before = get<int32_t>(f);
    std::vector<int32_t> len((size_t)get<int32_t>(f));
    for (auto &l : len) l = get<int32_t>(f);
    std::vector<std::complex<int16_t>> x;
    int16_t v[2];
    while (f.read((char *)v, 4)) x.emplace_back(v[0], v[1]);

    dsptl::DemodulatorOqpsk<int16_t> demod;
    if (!bits.empty()) demod.setSyncPattern(bits);
    demod.setReference(ref);
    demod.setInitialFrequency(freq);
    demod.reset();
    demod.setInputShift(shift);

    std::ofstream out(out_path, std::ios::binary);
    size_t pos = 0;
    for (size_t c = 0; c < len.size(); ++c) {
        if ((int32_t)c == reset_before) demod.reset();
        if (pos + (size_t)len[c] > x.size()) return 3;
        std::vector<std::complex<int16_t>> in(x.begin() + pos, x.begin() + pos + len[c]);
        pos += (size_t)len[c];
        int32_t error = 0;
        const std::vector<int8_t> soft = demod.step(in, error);
        const int32_t ns = (int32_t)soft.size();
        const float mf = demod.getMeasuredFrequency();
        out.write((const char *)&ns, 4);
        out.write((const char *)soft.data(), ns);
        out.write((const char *)&error, 4);
        out.write((const char *)&mf, 4);
    }
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
