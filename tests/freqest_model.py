"""Plain-Python restatement of estimateFreq<int16_t, L>
(dsptl_miscellaneous.h:43-58): the oracle of the frequency estimator tests for
shapes the goldens (tests/golden/freqest_golden.*) do not hold.
tests/test_freqest_model_golden.py pins it to the reference bit for bit.

Both terms of a pair are ints in the reference; termI overflows at
x[i] = x[i+L] = (-32768, -32768) only, where the model takes the two's
complement wrap (-2^31) as the library does.  The sums are exact integers, the
float is float32(atan2(sumQ, sumI) / L) with both sums converted to double, and
``exact`` tells that (n - L) * T < 2^53, T the largest |term|: then no partial
sum of the reference's double accumulation was rounded.  Samples are (n, 2)
int16 arrays."""
from __future__ import annotations

import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def terms(x, L: int):
    """(termI, termQ) of every pair as int64 arrays, termI wrapped to int32."""
    x = np.asarray(x, np.int16).reshape(-1, 2).astype(np.int64)
    if len(x) <= L:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a, b = x[:len(x) - L], x[L:]
    ti = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    tq = a[:, 1] * b[:, 0] - a[:, 0] * b[:, 1]
    ti = ((ti + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    assert tq.size == 0 or (int(tq.min()) >= -(1 << 31) and int(tq.max()) < 1 << 31)
    return ti, tq


def estimate(x, L: int):
    """(freq float32, (sumI, sumQ) Python ints, exact bool)."""
    ti, tq = terms(x, L)
    si, sq = int(ti.sum()), int(tq.sum())  # |sum| < 2^31 * 2^31: no int64 overflow
    T = max(int(np.abs(ti).max()), int(np.abs(tq).max())) if ti.size else 0
    return np.float32(math.atan2(float(sq), float(si)) / L), (si, sq), ti.size * T < 1 << 53


def bits(f) -> int:
    return int(np.array([f], np.float32).view(np.uint32)[0])


def load_golden():
    g = os.path.join(HERE, "golden")
    with open(os.path.join(g, "freqest_golden.json")) as f:
        return json.load(f), np.load(os.path.join(g, "freqest_golden.npz"))
