"""The SDPSK demodulator's yardstick.  With v = carry ++ x, a = x[i], b = v[i]:
tq = im(a) re(b) - re(a) im(b); soft = clamp(tq >> shift, -128, 127)
(limitScale<int8_t, int32_t>, dsp_complex.h:45-63); bit = tq > 0; the new
carry is the last D samples of v."""
import numpy as np


def tq_of(a, b):
    """Im(a conj(b)) of int16 [..., 2] arrays, in int64 (it fits int32)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return a[..., 1] * b[..., 0] - a[..., 0] * b[..., 1]


def soft_of(tq, shift):
    return np.clip(np.asarray(tq, np.int64) >> shift, -128, 127).astype(np.int8)


class SdpskModel:
    def __init__(self, D=1, shift=0, carry=None):
        self.D, self.shift = int(D), int(shift)
        self.carry = np.zeros((self.D, 2), np.int16) if carry is None else np.array(carry, np.int16).reshape(self.D, 2)

    def reset(self):
        self.carry[:] = 0

    def copy(self):
        return SdpskModel(self.D, self.shift, self.carry)

    def step(self, x):
        """x int16 [n, 2] -> (soft int8 [n], bits uint8 [n])."""
        x = np.asarray(x, np.int16).reshape(-1, 2)
        n = len(x)
        v = np.concatenate([self.carry, x])
        tq = tq_of(x, v[:n])
        self.carry = v[n:n + self.D].copy()
        return soft_of(tq, self.shift), (tq > 0).astype(np.uint8)
