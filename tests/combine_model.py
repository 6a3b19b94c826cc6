"""The carrier combiner's yardstick: the exact sum of the rows, the arithmetic
shift right, the clamp to int16, per component (limitScale<complex<int16_t>,
complex<int32_t>>, dsp_complex.h:83-108, over a sum)."""
import numpy as np


def combine(rows, shift=0):
    """rows: int16 [C, n, 2] (or a list of [n, 2]); int16 [n, 2]."""
    total = np.asarray(rows, np.int16).astype(np.int64).sum(axis=0)
    return np.clip(total >> shift, -32768, 32767).astype(np.int16)
