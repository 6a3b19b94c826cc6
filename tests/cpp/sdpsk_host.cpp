// The SDPSK demodulator's arithmetic (srcdsp_amd/csrc/sdpsk_kernels.h: the one
// source of the kernel's per-sample code and of srcdsp_sdpsk_step_host)
// compiled for the host, stand-alone, so that it can run under the address and
// undefined-behaviour sanitisers (tests/test_sdpsk_capi.py).
//
//   sdpsk_host <in.bin> <out.bin> <D> <shift> <chunk>...
// in.bin: D carry samples, then exactly the sum of the chunks complex<int16_t>
// samples.  The stream is stepped chunk by chunk, every chunk on exactly sized
// buffers.  out.bin gets the soft bits of the whole stream, then its bits, then
// the last carry (D samples).
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "sdpsk_kernels.h"

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const unsigned D = (unsigned)std::atoi(argv[3]), shift = (unsigned)std::atoi(argv[4]);
    if (D < 1 || D > srcdsp::kSdpskMaxD || shift > srcdsp::kSdpskMaxShift) return 2;
    std::vector<size_t> chunks;
    size_t total = 0;
    for (int k = 5; k < argc; ++k) {
        chunks.push_back((size_t)std::atol(argv[k]));
        total += chunks.back();
    }
    if (raw.size() != 4 * (D + total)) return 3;
    std::vector<uint32_t> carry(D);  // exactly D: a read or write past the carry is seen
    std::memcpy(carry.data(), raw.data(), 4 * D);
    std::vector<int8_t> soft_all;
    std::vector<uint8_t> bits_all;
    size_t at = D;
    for (size_t n : chunks) {
        std::vector<uint32_t> in(n);
        std::vector<int8_t> soft(n);
        std::vector<uint8_t> bits(n);
        if (n) std::memcpy(in.data(), raw.data() + 4 * at, 4 * n);
        at += n;
        srcdsp::sdpsk_host_run(carry.data(), D, shift, in.data(), n, soft.data(), bits.data());
        soft_all.insert(soft_all.end(), soft.begin(), soft.end());
        bits_all.insert(bits_all.end(), bits.begin(), bits.end());
    }
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char *)soft_all.data(), (std::streamsize)soft_all.size());
    o.write((const char *)bits_all.data(), (std::streamsize)bits_all.size());
    o.write((const char *)carry.data(), (std::streamsize)(4 * D));
    return o.good() ? 0 : 4;
}
