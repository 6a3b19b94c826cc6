"""Plain-Python restatement of dsptl::DemodulatorOqpsk<int16_t>
(demodulators.h:53-130, demodulators.cpp:34-308): the oracle of the demodulator
tests for shapes the goldens (tests/golden/demod_golden.*) do not hold.
tests/test_demod_model_golden.py pins it to the reference bit for bit.

Integer arithmetic is written out with the widths the reference computes in
(int16 members, int32 intermediates), so every wrap is explicit.  Samples are
(n, 2) int16 arrays, one complex sample per bit."""
from __future__ import annotations

import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TWO_PI, ONE_PI, HALF_PI, MAX_AMP = 8192, 4096, 2048, 128
G1, G2, B0 = 19333, 13107, 8000       # demodulators.h:107-110
NBR_FREQ_SAMPLES, FREQ_SHIFT = 32, 5  # demodulators.h:112-114
PI = 3.141592653589793238462643383279502884197169399375105820974944592307816406286


def i16(v: int) -> int:
    """static_cast<int16_t> of an int (two's complement wrap)."""
    return ((v + 32768) & 0xFFFF) - 32768


def tdiv(a: int, b: int) -> int:
    """C++ integer division: truncates toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


_TABLES = None


def tables():
    """(sineLUT[8192], phaseLUT[128 * 128]) as int16 (demodulators.cpp:39-55)."""
    global _TABLES
    if _TABLES is None:
        sine = np.array([int(math.sin(i * (PI / float(ONE_PI))) * 32767) for i in range(TWO_PI)], np.int16)
        ph = np.zeros(MAX_AMP * MAX_AMP, np.int16)
        for im in range(MAX_AMP):
            for re in range(MAX_AMP):
                v = math.atan2(im, re) * ONE_PI / PI
                ph[im * MAX_AMP + re] = int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)  # round(): half away
        _TABLES = (sine, ph)
    return _TABLES


def freq_word(f) -> int:
    """setInitialFrequency's conversion (demodulators.h:64): the product in
    float, the division and round() in double."""
    v = float(np.float32(f) * np.float32(ONE_PI)) / PI
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def word_freq(w: int) -> np.float32:
    """A float that setInitialFrequency converts to the word w."""
    f = np.float32(w * PI / ONE_PI)
    assert freq_word(f) == w
    return f


class DemodModel:
    def __init__(self):
        self.sine, self.phase_lut = (t.tolist() for t in tables())
        self.pattern: list[int] = []
        self.iref: list[int] = []
        self.qref: list[int] = []
        self.freq = 0        # intialFreqEst (indeterminate in the reference until set; 0 here as in the C ABI)
        self.init_phase = 0  # stored, never used
        self.acc_freq = 0
        self.reset()

    def copy(self):
        c = DemodModel.__new__(DemodModel)
        c.__dict__.update(self.__dict__)
        for k in ("pattern", "iref", "qref"):
            setattr(c, k, list(getattr(self, k)))
        return c

    def set_sync_pattern(self, bits):
        self.pattern = [int(b) for b in bits]

    def set_reference(self, ref):
        r = np.asarray(ref, np.int16).reshape(-1, 2)
        self.iref, self.qref = r[:, 0].tolist(), r[:, 1].tolist()

    def set_initial_frequency(self, f):
        self.freq = freq_word(f)

    def set_input_shift(self, s: int):
        self.shift = int(s)

    def reset(self):  # demodulators.cpp:293-308
        self.bit_cnt = self.mod2 = self.phase = self.bit1 = self.bit2 = self.i_prev = self.q_prev = 0
        self.shift = 0
        if self.pattern:
            self.bit1 = 2 * self.pattern[-1] - 1
            self.bit2 = 2 * self.pattern[-2] - 1

    def measured_frequency(self) -> np.float32:  # demodulators.h:72
        return np.float32((self.acc_freq >> FREQ_SHIFT) * PI / ONE_PI)

    def state(self):
        """The tuple srcdsp_demod_get_state returns."""
        return (self.bit_cnt, self.mod2, self.phase, self.bit1, self.bit2, self.i_prev, self.q_prev, self.freq,
                self.acc_freq, self.shift)

    def quick_phase(self, re: int, im: int) -> int:  # demodulators.cpp:61-92
        q2, q3, q4 = re <= 0 and im > 0, re < 0 and im <= 0, re >= 0 and im < 0
        re, im = i16(abs(re)), i16(abs(im))
        while re >= MAX_AMP or im >= MAX_AMP:
            re, im = i16(tdiv(re + 1, 2)), i16(tdiv(im + 1, 2))
        # -32768 has no int16 abs: the reference's index goes negative there
        # (undefined); the kernel clamps the address, and so does the model
        addr = min(max(MAX_AMP * im + re, 0), MAX_AMP * MAX_AMP - 1)
        p = self.phase_lut[addr]
        if q2:
            p = i16(ONE_PI - p)
        elif q3:
            p = i16(p - ONE_PI)
        elif q4:
            p = i16(-p)
        return p

    def rotate(self, re: int, im: int, phase: int):  # phaseShift, demodulators.cpp:107-120
        assert 0 <= phase < TWO_PI
        s, c = self.sine[phase], self.sine[(phase + HALF_PI) % TWO_PI]
        return i16((re * c + im * s + 16384) >> 15), i16((im * c - re * s + 16384) >> 15)

    def step(self, x):
        """(soft bits int8, error): demodulators.cpp:150-284."""
        x = np.asarray(x, np.int16).reshape(-1, 2)
        xi, xq = x[:, 0].tolist(), x[:, 1].tolist()
        n, P = len(xi), len(self.pattern)
        if self.bit_cnt == 0 and P:
            assert n > P  # :171
            soft = [0] * (n - P)
        else:
            soft = [0] * n
        cnt, err_acc = 0, 0
        start = n - NBR_FREQ_SAMPLES  # through int, then unsigned: negative -> never reached
        self.acc_freq = 0
        bit_cnt, mod2, phase = self.bit_cnt, self.mod2, self.phase
        bit1, bit2, ip, qp = self.bit1, self.bit2, self.i_prev, self.q_prev
        sh = self.shift
        for k in range(n):
            bit_cnt = (bit_cnt + 1) & 0xFFFFFFFF
            if P and bit_cnt < P:
                I, Q = self.rotate(self.iref[k] >> sh, self.qref[k] >> sh, phase)
                re_e, im_e = I, Q
            else:
                I, Q = self.rotate(xi[k] >> sh, xq[k] >> sh, phase)
                if P and bit_cnt == P:
                    re_e = im_e = 0
                else:
                    if mod2 == 0:
                        samp = I
                        bit0 = 2 * (samp > 0) - 1
                        re_s, im_s = i16(G2 * (bit2 + bit0)), i16(G1 * bit1)
                    else:
                        samp = Q
                        bit0 = 2 * (samp > 0) - 1
                        re_s, im_s = i16(G1 * bit1), i16(G2 * (bit2 + bit0))
                    samp = min(max(samp, -128), 127)
                    bit2, bit1 = bit1, bit0
                    soft[cnt] = samp
                    cnt += 1
                    re_e = i16(tdiv(ip * re_s + qp * im_s + 16384, 32768))
                    im_e = i16(tdiv(qp * re_s - ip * im_s + 16384, 32768))
            ip, qp = I, Q
            err = self.quick_phase(re_e, im_e)
            err_acc = (err_acc + abs(err)) & 0xFFFFFFFF
            step = i16(self.freq + i16(tdiv(B0 * err + 32768, 65536)))
            if start >= 0 and k >= start:
                self.acc_freq += step
            phase = (phase + step + TWO_PI) % TWO_PI
            mod2 = (mod2 + 1) % 2
        self.bit_cnt, self.mod2, self.phase = bit_cnt, mod2, phase
        self.bit1, self.bit2, self.i_prev, self.q_prev = bit1, bit2, ip, qp
        if err_acc >= 1 << 31:
            err_acc -= 1 << 32
        return np.array(soft, np.int8), err_acc


# ------------------------------------------------------------- test signals
def oqpsk_samples(bits, scale: float, omega: float = 0.0, theta: float = 0.0, prev_bit: int = 1,
                  next_bit: int = 1) -> np.ndarray:
    """One sample per bit of the signal the demodulator itself reconstructs
    (demodulators.cpp:217-235): at an even bit interval I = g1 b[j] and
    Q = g2 (b[j-1] + b[j+1]), at an odd one the branches swap; b = +-1.
    Scaled, then rotated by theta + omega j.  (n, 2) int16."""
    b = [2 * int(v) - 1 for v in bits]
    ext = [prev_bit] + b + [next_bit]
    out = np.zeros((len(b), 2), np.int16)
    for j in range(len(b)):
        eye, side = G1 * ext[j + 1], G2 * (ext[j] + ext[j + 2])
        z = complex(eye, side) if j % 2 == 0 else complex(side, eye)
        z *= scale * complex(math.cos(theta + omega * j), math.sin(theta + omega * j))
        out[j] = (int(round(z.real)), int(round(z.imag)))
    return out


def carrier_samples(n: int, amp: float, omega: float = 0.0, theta: float = 0.0) -> np.ndarray:
    """The sync word's bit samples with the modulation removed: a bare carrier."""
    j = np.arange(n)
    return np.stack([np.round(amp * np.cos(theta + omega * j)), np.round(amp * np.sin(theta + omega * j))],
                    1).astype(np.int16)


# ------------------------------------------------------------------ goldens
def load_golden():
    g = os.path.join(HERE, "golden")
    with open(os.path.join(g, "demod_golden.json")) as f:
        return json.load(f), np.load(os.path.join(g, "demod_golden.npz"))


def golden_case_model(case, arr) -> DemodModel:
    """A model configured as tests/cpp/demod_main.cpp configures its object."""
    k = case["key"]
    m = DemodModel()
    if case["P"]:
        m.set_sync_pattern(arr[k + "_bits"])
    m.set_reference(arr[k + "_ref"])
    m.set_initial_frequency(np.float32(arr[k + "_freq"][0]))
    m.reset()
    m.set_input_shift(case["shift"])
    return m
