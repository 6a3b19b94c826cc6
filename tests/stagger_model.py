"""numpy model of the OQPSK Q-rail stagger (srcdsp_stagger_*; an extension with
no reference class): a delay line of D samples on the imaginary rail of
complex<int16_t> samples.  With v = carry ++ im(in):

    out[i] = (re(in[i]), v[i])      i.e. im(in[i - D]), or carry[i] for i < D
    carry' = v[n .. n + D)          also when n < D

plus the offset transmit chain composed of the reference's own operators
(the mapper model, the oracle's interpolator and mixer) around it, and the
loader of the goldens recorded from the reference build
(tests/golden/gen_oqpsk_golden.py)."""
from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class StaggerModel:
    def __init__(self, D: int, carry=None):
        assert 1 <= D <= 64
        self.D = D
        self.carry = np.zeros(D, np.int16) if carry is None else np.array(carry, np.int16).reshape(D)

    def copy(self):
        return StaggerModel(self.D, self.carry)

    def reset(self):
        self.carry[:] = 0

    def step(self, x) -> np.ndarray:
        x = np.asarray(x, np.int16).reshape(-1, 2)
        n = len(x)
        v = np.concatenate([self.carry, x[:, 1]])
        out = np.stack([x[:, 0], v[:n]], 1).astype(np.int16)
        self.carry = v[n:n + self.D].copy()
        return out


def offset_chain(o, mapper, taps, L, stagger, freq, calls, N=4096, variant=0, end=None):
    """The four operators one after the other, per call (bits, flush): the
    mapper model, the oracle's FilterUpsamplingFir and Mixer, the stagger model
    between them.  Returns the concatenated output, int16 [n, 2]; `end` (a
    dict) receives the mixer's (phase, frequency word) after the last call."""
    up = o.up(variant, L, taps)
    mixer = o.mixer(N)
    mixer.reset(freq)
    ys = []
    for bits, flush in calls:
        y = np.asarray(up.step(mapper.step(bits), flush)).reshape(-1, 2)
        ys.append(np.asarray(mixer.step(stagger.step(y))).reshape(-1, 2))
    if end is not None:
        end["mixer"] = tuple(mixer.state()[:2])
    return np.concatenate(ys)


def load_golden():
    g = os.path.join(HERE, "golden")
    with open(os.path.join(g, "oqpsk_golden.json")) as f:
        return json.load(f), np.load(os.path.join(g, "oqpsk_golden.npz"))
