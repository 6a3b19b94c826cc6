// The kernel's per-sample arithmetic (srcdsp_amd/csrc/demod_kernels.h,
// demod_sample: one source for host and device) run on the host over a golden
// case, so the suite checks it against the reference without a GPU.
//
//   demod_lane_host <case.bin> <tables.bin> <out.bin>
// case.bin / out.bin: the formats of tests/cpp/demod_main.cpp; tables.bin:
// int16 sine[8192] then phase[128 * 128].  Plain g++, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "demod_kernels.h"

using namespace srcdsp;

template <class T>
static T get(std::ifstream &f) {
    T v{};
    f.read((char *)&v, sizeof v);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::ifstream f(argv[1], std::ios::binary), tf(argv[2], std::ios::binary);
    if (!f || !tf) return 2;
    std::vector<int16_t> tab(kDemodSine + kDemodPhase);
    tf.read((char *)tab.data(), 2 * tab.size());
    const int16_t *sine = tab.data(), *phase_lut = sine + kDemodSine;
    std::vector<int8_t> bits((size_t)get<int32_t>(f));
    for (auto &b : bits) b = get<int8_t>(f);
    std::vector<uint32_t> ref((size_t)get<int32_t>(f));
    for (auto &r : ref) r = get<uint32_t>(f);
    int shift = get<int32_t>(f);
    const float fr = get<float>(f);
    const int freq = (int)std::round((double)(fr * (float)4096) / 3.141592653589793238462643383279502884);
    const int32_t reset_before = get<int32_t>(f);
    std::vector<int32_t> len((size_t)get<int32_t>(f));
    for (auto &l : len) l = get<int32_t>(f);
    std::vector<uint32_t> x;
    uint32_t w;
    while (f.read((char *)&w, 4)) x.push_back(w);

    const unsigned P = (unsigned)bits.size();
    DemodLane s{};
    auto reset = [&] {
        s = DemodLane{};
        if (P) {
            s.bit1 = 2 * bits[P - 1] - 1;
            s.bit2 = 2 * bits[P - 2] - 1;
        }
    };
    reset();  // demod_main: reset(), then setInputShift
    std::ofstream out(argv[3], std::ios::binary);
    size_t pos = 0;
    for (size_t c = 0; c < len.size(); ++c) {
        if ((int32_t)c == reset_before) {
            reset();
            shift = 0;
        }
        const long n = len[c];
        const int32_t ns = s.bit_cnt == 0 && P ? (int32_t)(n - P) : (int32_t)n;
        std::vector<int8_t> soft((size_t)ns, 0);
        int cnt = 0;
        s.err_acc = 0;
        s.acc_freq = 0;
        const long acc_from = n >= 32 ? n - 32 : n;
        for (long k = 0; k < n; ++k) {
            const uint32_t rw = (size_t)k < ref.size() ? ref[k] : 0u;
            int sv = 0;
            if (demod_sample(s, x[pos + k], rw, P, shift, freq, k >= acc_from, sine, phase_lut, &sv))
                soft[cnt++] = (int8_t)sv;
        }
        pos += (size_t)n;
        const int32_t error = (int32_t)s.err_acc;
        const float mf = static_cast<float>((s.acc_freq >> 5) * 3.141592653589793238462643383279502884 / 4096);
        out.write((const char *)&ns, 4);
        out.write((const char *)soft.data(), ns);
        out.write((const char *)&error, 4);
        out.write((const char *)&mf, 4);
    }
    return out.good() ? 0 : 4;
}
