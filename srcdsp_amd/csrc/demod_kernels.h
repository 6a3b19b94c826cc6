// demod_kernels.h -- dsptl::DemodulatorOqpsk<int16_t>::step
// (demodulators.cpp:150-284) as a bank of independent recurrences: one lane
// per burst, 64 bursts per workgroup (one wave).
//
// The per-sample arithmetic (demod_sample) is written once for host and
// device, in the widths the reference computes in: int16 members, int32
// intermediates, every cast to int16 a two's complement wrap.  The kernel
// around it never waits on HBM inside the recurrence:
//   * both lookup tables (sine 8192, phase 128 x 128, int16: 48 KiB) are copied
//     into LDS once per workgroup, so the three dependent look-ups per sample
//     cost LDS latency;
//   * the input comes in tiles of kDemodTile samples x 64 rows, read with
//     coalesced row loads (lanes along the row, 256 B per row) into registers
//     one tile ahead, then transposed through an LDS tile of row stride
//     kDemodTile + 1 words: lane r reads bank (r + k) mod 64, no conflict;
//   * soft bits are collected per row in LDS and written in row-contiguous
//     runs at the row's own running count.
#pragma once
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace srcdsp {

constexpr int kDemodLanes = 64;  // bursts per workgroup
constexpr int kDemodTile = 64;   // samples per row and tile (tests/golden/demod_golden.json "tile")
constexpr int kDemodSine = 8192, kDemodAmp = 128, kDemodPhase = kDemodAmp * kDemodAmp;
constexpr int kDemodTableWords = (kDemodSine + kDemodPhase) / 2;  // int16 pairs
constexpr int kDemodSoftStride = kDemodTile + 4;                   // bytes; 17 words, odd: no bank conflict
// LDS of a workgroup: tables | input tile | soft tile | row offsets and counts
constexpr int kDemodLdsBytes = 2 * (kDemodSine + kDemodPhase) + 4 * kDemodLanes * (kDemodTile + 1) +
                               kDemodLanes * kDemodSoftStride + kDemodLanes * (8 + 8 + 4);

// the words of a handle's state, and of the packed row a step returns
// (StateVar demodulators.h:76-88, then error and accumulatedFrequency)
enum { DS_BITCNT = 0, DS_MOD2, DS_PHASE, DS_BIT1, DS_BIT2, DS_IPREV, DS_QPREV, DS_ERROR, DS_ACCFREQ, DS_WORDS };

// one channel of a launch: a row of the device table uploaded once per call,
// which the channels' reference samples follow (packed (Iref, Qref) words)
struct DemodChan {
    long in_off;    // first sample of the row, from the launch's input pointer
    long soft_off;  // first soft bit of the row, from the launch's soft pointer
    long soft_len;  // n_soft of the row: positions past the last soft bit written are zeroed
    int ref_off, ref_len;  // the row's reference samples, as many as its preamble reads in this call
    int P, shift, freq;
    int32_t st[7];  // StateVar at the start of the call, DS_BITCNT .. DS_QPREV
};

struct DemodLane {
    uint32_t bit_cnt;
    int mod2, phase, bit1, bit2, i_prev, q_prev;
    uint32_t err_acc;
    int acc_freq;
};

__host__ __device__ inline int demod_i16(int v) { return (int)(int16_t)(uint16_t)(unsigned)v; }

// quickPhase (demodulators.cpp:61-92).  The halving loop, (v + 1) / 2 until
// both components are < 128, is k rounds of a ceiling division by 2, i.e.
// ceil(v / 2^k) with the smallest k that brings the larger one under 128.
// -32768 has no int16 abs: the reference's loop then runs on a negative value
// and its table index goes negative (undefined); here the same loop runs and
// the address is clamped.
template <class Tab>
__host__ __device__ inline int demod_quick_phase(int re, int im, const Tab &phase_lut) {
    const bool q2 = re <= 0 && im > 0, q3 = re < 0 && im <= 0, q4 = re >= 0 && im < 0;
    re = demod_i16(re < 0 ? -re : re);
    im = demod_i16(im < 0 ? -im : im);
    if (re >= 0 && im >= 0) {
        const unsigned m = (unsigned)(re > im ? re : im);
        int k = m < (unsigned)kDemodAmp ? 0 : 25 - __builtin_clz(m);  // m >> k < 128 <= m >> (k - 1)
        if ((m + (1u << k) - 1u) >> k >= (unsigned)kDemodAmp) ++k;     // the ceiling reached 128
        re = (re + (1 << k) - 1) >> k;
        im = (im + (1 << k) - 1) >> k;
    } else {
        while (re >= kDemodAmp || im >= kDemodAmp) {
            re = demod_i16((re + 1) / 2);
            im = demod_i16((im + 1) / 2);
        }
    }
    int addr = kDemodAmp * im + re;
    addr = addr < 0 ? 0 : (addr > kDemodPhase - 1 ? kDemodPhase - 1 : addr);
    int p = phase_lut[addr];
    if (q2) p = 4096 - p;
    else if (q3) p = p - 4096;
    else if (q4) p = -p;
    return p;
}

// One sample of step()'s loop (:186-271).  w: the packed input sample; rw: the
// packed reference sample Iref[k], Qref[k] (read only in the preamble).
// Returns true when a soft bit was produced (*soft).  freq within +-4096
// keeps phase + step + 8192 positive, so the reference's % is the mask.
template <class Tab>
__host__ __device__ inline bool demod_sample(DemodLane &s, uint32_t w, uint32_t rw, unsigned P, int shift, int freq,
                                             bool acc, const Tab &sine, const Tab &phase_lut, int *soft) {
    ++s.bit_cnt;
    const bool pre = P != 0 && s.bit_cnt < P;
    const uint32_t v = pre ? rw : w;
    const int i0 = (int)(int16_t)(v & 0xffffu) >> shift, q0 = ((int32_t)v >> 16) >> shift;
    // phaseShift (:107-120)
    const int sn = sine[s.phase], cs = sine[(s.phase + 2048) & 8191];
    const int I = demod_i16((i0 * cs + q0 * sn + 16384) >> 15);
    const int Q = demod_i16((q0 * cs - i0 * sn + 16384) >> 15);
    int re_e, im_e;
    bool out = false;
    if (pre) {
        re_e = I;
        im_e = Q;
    } else if (P != 0 && s.bit_cnt == P) {
        re_e = im_e = 0;
    } else {
        int samp, re_s, im_s, bit0;
        if (s.mod2 == 0) {  // eye opening in the I branch
            samp = I;
            bit0 = samp > 0 ? 1 : -1;
            re_s = demod_i16(13107 * (s.bit2 + bit0));
            im_s = demod_i16(19333 * s.bit1);
        } else {
            samp = Q;
            bit0 = samp > 0 ? 1 : -1;
            re_s = demod_i16(19333 * s.bit1);
            im_s = demod_i16(13107 * (s.bit2 + bit0));
        }
        *soft = samp > 127 ? 127 : (samp < -128 ? -128 : samp);
        out = true;
        s.bit2 = s.bit1;
        s.bit1 = bit0;
        // the reference divides (truncation toward zero), it does not shift
        re_e = demod_i16((s.i_prev * re_s + s.q_prev * im_s + 16384) / 32768);
        im_e = demod_i16((s.q_prev * re_s - s.i_prev * im_s + 16384) / 32768);
    }
    s.i_prev = I;
    s.q_prev = Q;
    const int err = demod_quick_phase(re_e, im_e, phase_lut);
    s.err_acc += (uint32_t)(err > 0 ? err : -err);
    const int step = demod_i16(freq + demod_i16((8000 * err + 32768) / 65536));
    if (acc) s.acc_freq += step;
    s.phase = (s.phase + step + 8192) & 8191;
    s.mod2 ^= 1;
    return out;
}

}  // namespace srcdsp
