"""Python model of the reference symbol mappers (modulators.h): SymbolMapperSdpsk
(:82-131) and SymbolMapperQpsk (:147-198) for T = int16_t, written from the
reference's loops (not from the kernels' closed form), plus the loaders of the
goldens recorded from the reference itself (tests/golden/gen_mapper_golden.py)."""
from __future__ import annotations

import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SDPSK, QPSK = 0, 1
A = 8192  # ModAmplitude<int16_t> (modulators.h:34-39)
SDPSK_MAP = np.array([(A, A), (-A, A), (-A, -A), (A, -A)], np.int16)   # :93-96
QPSK_MAP = np.array([(-A, -A), (-A, A), (A, -A), (A, A)], np.int16)    # :158-161


class MapperModel:
    def __init__(self, kind: int, state: int = 0):
        self.kind, self.state = kind, state

    def reset(self):
        self.state = 0

    def n_out(self, n_bits: int) -> int:
        return n_bits // 2 if self.kind == QPSK else n_bits

    def step(self, bits) -> np.ndarray:
        b = np.asarray(bits, np.uint8).reshape(-1) > 0  # `bits[i] > 0` on a uint8_t
        if self.kind == QPSK:
            assert b.size % 2 == 0
            st = (b[0::2].astype(np.int64) << 1) | b[1::2].astype(np.int64)
            if st.size:
                self.state = int(st[-1])
            return QPSK_MAP[st].reshape(-1, 2)
        # state += bit ? 1 : 3; state %= 4, one bit after the other (:110-111)
        st = (self.state + np.cumsum(np.where(b, 1, 3), dtype=np.int64)) % 4
        if st.size:
            self.state = int(st[-1])
        return SDPSK_MAP[st].reshape(-1, 2)


def step_loop(kind: int, state: int, bits):
    """The reference's loops literally, one bit at a time (a cross-check of the
    vectorised model above on short inputs)."""
    out = []
    b = [int(v) for v in np.asarray(bits, np.uint8).reshape(-1)]
    if kind == QPSK:
        for i in range(len(b) // 2):
            state = ((1 if b[2 * i] > 0 else 0) << 1) | (1 if b[2 * i + 1] > 0 else 0)
            out.append(QPSK_MAP[state])
    else:
        for v in b:
            state += 1 if v > 0 else 3
            state %= 4
            out.append(SDPSK_MAP[state])
    return np.array(out, np.int16).reshape(-1, 2), state


def load_golden():
    g = os.path.join(HERE, "golden")
    with open(os.path.join(g, "mapper_golden.json")) as f:
        return json.load(f), np.load(os.path.join(g, "mapper_golden.npz"))


def case_bin(kind, reset_before, copy_before, calls, bits) -> bytes:
    """The case file of tests/cpp/mapper_main.cpp."""
    b = struct.pack("<iiii", kind, reset_before, copy_before, len(calls))
    return b + np.asarray(calls, "<i4").tobytes() + np.ascontiguousarray(bits, np.uint8).tobytes()


def parse_out(blob: bytes, n_calls: int):
    """Per call the symbols mapper_main wrote, int16 [n, 2]."""
    out, pos = [], 0
    for _ in range(n_calls):
        (ns,) = struct.unpack_from("<i", blob, pos)
        out.append(np.frombuffer(blob, np.int16, 2 * ns, pos + 4).reshape(-1, 2))
        pos += 4 + 4 * ns
    assert pos == len(blob)
    return out


def golden_calls(case, arr):
    """(bits, symbols, state) of every call of a mapper golden case."""
    k = case["key"]
    bits, sym, pos, spos = arr[k + "_bits"], arr[k + "_sym"], 0, 0
    for n, st in zip(case["calls"], case["states"]):
        ns = n // 2 if case["kind"] == QPSK else n
        yield bits[pos:pos + n], sym[spos:spos + ns], st
        pos += n
        spos += ns
